// k_refit.hip -- the device side of the refit of the 3D lines against cameras and their 2D segments (host
// side: l3d_refit.hip; the projection, the association, the scan and the solver are k_project.hip's stage 1,
// k_associate.hip, k_scan.hip and k_lineopt.hip, unchanged).  The arithmetic is the contract of §28, fp64 in the order
// written there (the library is built with -ffp-contract=off), so that tests/refit_model.py follows it operation for
// operation.  No atomics, no inline assembly, one lane per element throughout.
//   k_refit_flag     one lane per 2D segment: 1 iff its association names a record and it accepted one record only (or
//                    ambiguous segments are used); k_scan turns the flags into ranks in place.
//   k_refit_compact  one lane per 2D segment: an observation files its flat 2D segment and its line at its rank, so the
//                    list is in flat (camera, segment) order.
//   k_refit_obs      one lane per observation of a solved line, in CSR order: the LoObs of l3d_lineopt.h -- the end
//                    points widened, the unit normal (-dy, dx) of the direction as the line bundling forms it, the
//                    camera, found by bisection of the cameras' first segments.
//   k_refit_spans    one lane per observation of a solved line: refit_span of l3d_refit.h along the written-back carrier
//                    of its line, found by bisection of the CSR.
#include "l3d_refit.h"

namespace l3d {
namespace {

constexpr uint32_t kRefitBlock = 256;

__global__ __launch_bounds__(kRefitBlock) void k_refit_flag(RefitCompactArgs a) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= a.n_seg) return;
    const AssocOut o = a.assoc[i];
    a.flag[i] = (o.record >= 0 && (o.n_accepted == 1u || a.use_ambiguous)) ? 1u : 0u;
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_compact(RefitCompactArgs a) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= a.n_seg) return;
    const uint32_t rank = a.flag[i];
    if (a.flag[i + 1] == rank) return;
    a.obs_seg[rank] = i;
    a.obs_line[rank] = a.assoc[i].line;
}

// the last k in [0, n) with table[k] <= v (table ascending, table[0] <= v)
__device__ __forceinline__ uint32_t last_not_above(const uint32_t* table, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (table[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_obs(RefitObsArgs a) {
    const uint32_t r = blockIdx.x * kRefitBlock + threadIdx.x;
    if (r >= a.n_obs) return;
    const uint32_t flat = a.obs_seg[a.perm[r]];
    const float4 sg = a.segs[flat];
    const double p1x = (double)sg.x, p1y = (double)sg.y, p2x = (double)sg.z, p2y = (double)sg.w;
    double dx = p2x - p1x, dy = p2y - p1y;
    const double n = sqrt(dx * dx + dy * dy);
    if (n > 0.0) { dx /= n; dy /= n; }
    // a camera without segments shares its first segment with the next one: the last of them is the owner
    a.obs[r] = LoObs{p1x, p1y, p2x, p2y, -dy, dx, last_not_above(a.seg_begin, a.n_cams, flat), 0u};
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_spans(RefitObsArgs a) {
    const uint32_t r = blockIdx.x * kRefitBlock + threadIdx.x;
    if (r >= a.n_obs) return;
    const uint32_t l = last_not_above(a.res_off, a.n_lines, r);
    const LoObs o = a.obs[r];
    const double* mu = a.carrier + 6 * (size_t)l;
    const double M[3] = {mu[0], mu[1], mu[2]}, u[3] = {mu[3], mu[4], mu[5]};
    a.spans[r] = refit_span(a.cams[o.cam], o.p1x, o.p1y, o.p2x, o.p2y, M, u);
}

}  // namespace

hipError_t launch_refit_flag(const RefitCompactArgs& a, hipStream_t st) {
    if (!a.n_seg) return hipSuccess;
    hipLaunchKernelGGL(k_refit_flag, dim3((a.n_seg + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_refit_compact(const RefitCompactArgs& a, hipStream_t st) {
    if (!a.n_seg) return hipSuccess;
    hipLaunchKernelGGL(k_refit_compact, dim3((a.n_seg + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_refit_obs(const RefitObsArgs& a, hipStream_t st) {
    if (!a.n_obs) return hipSuccess;
    hipLaunchKernelGGL(k_refit_obs, dim3((a.n_obs + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_refit_spans(const RefitObsArgs& a, hipStream_t st) {
    if (!a.n_obs) return hipSuccess;
    hipLaunchKernelGGL(k_refit_spans, dim3((a.n_obs + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
