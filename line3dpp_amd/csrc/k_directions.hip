// k_directions.hip -- the directions the lines of a 3D model run in: a unit direction per segment, and every direction
// scored against every segment (stages 1 and 2; host side: l3d_directions.hip, the selection:
// l3d_directions.h).  No counterpart in the reference.
//   k_dir_units   one lane per segment: e = P2 - P1, E2 = e.e, D = e / sqrt(E2) for a live segment and 0 for a point; the
//                 32-byte record carries §25's weight word beside D.
//   k_dir_score   k_compare's tiling: a workgroup = a tile of kCmpTile = 256 hypotheses x one slice of the segments, block =
//                 tile * n_slices + slice; the slice passes through LDS in chunks of kCmpChunk = 256 records (8 KiB), every
//                 lane walks the chunk with broadcast reads and adds up its inliers, |D_h x D_s|^2 <= max_sin2:
//                 cells[h * n_slices + slice] = {weight, count, 0}.  Hypothesis h is segment h.
// The cells of a hypothesis are added by k_pl_merge (k_planes.hip), whose layout they share.  The weights are integers
// whose total stays below 2^53 (stage 0 on the host), so the sums are associative: no slicing and no order of workgroups
// changes a bit.  No atomics, no cross-lane traffic; a lane beyond the last hypothesis takes part in every barrier and
// writes nothing.
#include "l3d_kernels.h"

namespace l3d {
namespace {

constexpr uint32_t kDirWords = sizeof(DirUnit) / 8;    // 64-bit words per record

__global__ __launch_bounds__(256) void k_dir_units(DirArgs a) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n) return;
    const double* v = a.segs + 6 * (size_t)s;
    const double ex = v[3] - v[0], ey = v[4] - v[1], ez = v[5] - v[2];
    const double E2 = (ex * ex + ey * ey) + ez * ez;
    const bool live = E2 > 0.0;
    const double len = sqrt(E2);
    DirUnit o;
    o.D[0] = live ? ex / len : 0.0; o.D[1] = live ? ey / len : 0.0; o.D[2] = live ? ez / len : 0.0;
    o.w = a.weight[s];
    a.units[s] = o;
}

__global__ __launch_bounds__(kCmpTile) void k_dir_score(DirArgs a) {
    __shared__ unsigned long long s_u[kCmpChunk * kDirWords];      // the chunk's records, word by word
    const uint32_t tile = blockIdx.x / a.n_slices, slice = blockIdx.x - tile * a.n_slices;
    const uint32_t h = tile * kCmpTile + threadIdx.x;
    const bool in_range = h < a.n;
    DirUnit me{{0.0, 0.0, 0.0}, 0ull};
    if (in_range) me = a.units[h];
    const bool live = in_range && (me.w & kPlLiveBit) != 0ull;
    const double hx = me.D[0], hy = me.D[1], hz = me.D[2];
    const double ms = a.max_sin2;
    const unsigned long long* units = (const unsigned long long*)a.units;
    uint32_t r_begin, r_end;
    cmp_slice_range(a.n, slice, a.slice_chunks, r_begin, r_end);
    unsigned long long weight = 0ull;
    uint32_t count = 0u;
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += kCmpChunk) {
        const uint32_t n = min(kCmpChunk, r_end - r0);
        __syncthreads();                               // the previous chunk has been read
        for (uint32_t i = threadIdx.x; i < kDirWords * n; i += kCmpTile) s_u[i] = units[kDirWords * (size_t)r0 + i];
        __syncthreads();
        if (!live) continue;                           // (after the barriers)
        for (uint32_t k = 0; k < n; ++k) {
            const unsigned long long w = s_u[kDirWords * k + 3];
            if (!(w & kPlLiveBit)) continue;           // a point segment (uniform over the workgroup)
            const double dx = __longlong_as_double((long long)s_u[kDirWords * k]);
            const double dy = __longlong_as_double((long long)s_u[kDirWords * k + 1]);
            const double dz = __longlong_as_double((long long)s_u[kDirWords * k + 2]);
            const double cx = hy * dz - hz * dy, cy = hz * dx - hx * dz, cz = hx * dy - hy * dx;
            const double x2 = (cx * cx + cy * cy) + cz * cz;
            if (x2 <= ms) { weight += w & ~kPlLiveBit; ++count; }
        }
    }
    if (in_range) a.cells[(size_t)h * a.n_slices + slice] = PlCell{weight, count, 0u};
}

}  // namespace

hipError_t launch_dir_units(const DirArgs& a, hipStream_t st) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(k_dir_units, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_dir_score(const DirArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_dir_score, dim3(((a.n + kCmpTile - 1) / kCmpTile) * a.n_slices), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
