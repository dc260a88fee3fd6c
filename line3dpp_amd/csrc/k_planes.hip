// k_planes.hip -- the planes the lines of a 3D model lie in: a plane per junction, and every plane scored against every
// segment (stages 1 and 2; host side: l3d_planes.hip, the selection: l3d_planes.h).  No counterpart in the
// reference.  The junctions are k_wireframe.hip's records, left on the device.
//   k_pl_hypotheses  one lane per junction: J = the midpoint of the closest points, N = (ea x eb) / |ea x eb|; dead (N = 0)
//                    unless the squared length of the cross product is positive and finite.
//   k_pl_score       k_compare's tiling: a workgroup = a tile of kCmpTile = 256 hypotheses x one slice of the segments,
//                    block = tile * n_slices + slice; the slice passes through LDS in chunks of kCmpChunk = 256 (48 bytes of
//                    end points and the 8-byte weight word each), every lane walks the chunk with broadcast reads and adds
//                    up its inliers: cells[h * n_slices + slice] = {weight, count, 0}.
//   k_pl_merge       one lane per hypothesis adds its cells: scores[h]; §26's k_dir_score fills the same cells and shares it.
// The weights are integers whose total stays below 2^53 (stage 0 on the host), so the sums are associative: no slicing
// and no order of workgroups changes a bit.  No atomics, no cross-lane traffic; a lane beyond the last hypothesis takes
// part in every barrier and writes nothing.
#include "l3d_kernels.h"

namespace l3d {
namespace {

__global__ __launch_bounds__(256) void k_pl_hypotheses(PlArgs a) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= a.n_h) return;
    const WfJunction r = a.junctions[h];
    const double* va = a.segs + 6 * (size_t)r.a;
    const double* vb = a.segs + 6 * (size_t)r.b;
    const double eax = va[3] - va[0], eay = va[4] - va[1], eaz = va[5] - va[2];
    const double ebx = vb[3] - vb[0], eby = vb[4] - vb[1], ebz = vb[5] - vb[2];
    PlHypothesis o;
    o.J[0] = ((va[0] + r.sa * eax) + (vb[0] + r.sb * ebx)) * 0.5;
    o.J[1] = ((va[1] + r.sa * eay) + (vb[1] + r.sb * eby)) * 0.5;
    o.J[2] = ((va[2] + r.sa * eaz) + (vb[2] + r.sb * ebz)) * 0.5;
    const double mx = eay * ebz - eaz * eby, my = eaz * ebx - eax * ebz, mz = eax * eby - eay * ebx;
    const double m2 = (mx * mx + my * my) + mz * mz;
    const bool live = m2 > 0.0 && m2 <= 1.7976931348623157e308;      // positive and finite (a NaN fails both)
    const double len = sqrt(m2);
    o.N[0] = live ? mx / len : 0.0; o.N[1] = live ? my / len : 0.0; o.N[2] = live ? mz / len : 0.0;
    if (!live) { o.J[0] = 0.0; o.J[1] = 0.0; o.J[2] = 0.0; }
    o.a = r.a; o.b = r.b; o.live = live ? 1u : 0u; o.pad = 0u;
    a.hyp[h] = o;
}

// the n <= kCmpChunk segments from r0 on staged into LDS, coalesced, by the whole workgroup (cmp_stage_chunk with the
// weight words in the place of the line indices)
__device__ __forceinline__ void pl_stage_chunk(double* s_p, unsigned long long* s_w, const PlArgs& a, uint32_t r0, uint32_t n) {
    __syncthreads();                                                             // the previous chunk has been read
    for (uint32_t i = threadIdx.x; i < 6 * n; i += kCmpTile) s_p[i] = a.segs[6 * (size_t)r0 + i];
    if (threadIdx.x < n) s_w[threadIdx.x] = a.weight[r0 + threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(kCmpTile) void k_pl_score(PlArgs a) {
    __shared__ double s_p[kCmpChunk * 6];              // (P1, P2) of the chunk's segments
    __shared__ unsigned long long s_w[kCmpChunk];      // their weight words
    const uint32_t tile = blockIdx.x / a.n_slices, slice = blockIdx.x - tile * a.n_slices;
    const uint32_t h = tile * kCmpTile + threadIdx.x;
    const bool in_range = h < a.n_h;
    PlHypothesis me{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0u, 0u, 0u, 0u};
    if (in_range) me = a.hyp[h];
    const bool live = in_range && me.live != 0u;
    const double nx = me.N[0], ny = me.N[1], nz = me.N[2], jx = me.J[0], jy = me.J[1], jz = me.J[2];
    const double md = a.max_distance;
    uint32_t r_begin, r_end;
    cmp_slice_range(a.n, slice, a.slice_chunks, r_begin, r_end);
    unsigned long long weight = 0ull;
    uint32_t count = 0u;
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += kCmpChunk) {
        const uint32_t n = min(kCmpChunk, r_end - r0);
        pl_stage_chunk(s_p, s_w, a, r0, n);
        if (!live) continue;                           // (after the barriers)
        for (uint32_t k = 0; k < n; ++k) {
            const unsigned long long w = s_w[k];
            if (!(w & kPlLiveBit)) continue;           // a point segment (uniform over the workgroup)
            const double* v = s_p + 6 * k;
            const double h1 = (nx * (v[0] - jx) + ny * (v[1] - jy)) + nz * (v[2] - jz);
            const double h2 = (nx * (v[3] - jx) + ny * (v[4] - jy)) + nz * (v[5] - jz);
            if (fabs(h1) <= md && fabs(h2) <= md) { weight += w & ~kPlLiveBit; ++count; }
        }
    }
    if (in_range) a.cells[(size_t)h * a.n_slices + slice] = PlCell{weight, count, 0u};
}

// (launched for the directions of §26 as well: their cells have this layout)
__global__ __launch_bounds__(256) void k_pl_merge(const PlCell* cells, PlCell* scores, uint32_t n_h, uint32_t n_slices) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= n_h) return;
    const PlCell* c = cells + (size_t)h * n_slices;
    PlCell sum{0ull, 0u, 0u};
    for (uint32_t s = 0; s < n_slices; ++s) { sum.weight += c[s].weight; sum.count += c[s].count; }
    scores[h] = sum;
}

}  // namespace

hipError_t launch_pl_hypotheses(const PlArgs& a, hipStream_t st) {
    if (!a.n_h) return hipSuccess;
    hipLaunchKernelGGL(k_pl_hypotheses, dim3((a.n_h + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pl_score(const PlArgs& a, hipStream_t st) {
    if (!a.n_h || !a.n || !a.n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_pl_score, dim3(((a.n_h + kCmpTile - 1) / kCmpTile) * a.n_slices), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pl_merge(const PlCell* cells, PlCell* scores, uint32_t n_h, uint32_t n_slices, hipStream_t st) {
    if (!n_h || !n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_pl_merge, dim3((n_h + 255) / 256), dim3(256), 0, st, cells, scores, n_h, n_slices);
    return hipGetLastError();
}

}  // namespace l3d
