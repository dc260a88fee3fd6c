// k_merge.hip -- the accepted pairs of a 3D line model against itself, as a list (host side: l3d_merge.hip).
// No counterpart in the reference.  A pair (q, r) is accepted iff line(q) != line(r) and steps 1-6 of §18 accept it
// (cmp_pair of l3d_kernels.h, the very function k_compare runs).  Where k_compare keeps one best reference per query,
// this stage hands out every accepted pair, in ascending (q, r) order, in two walks over k_compare's tiling:
//   k_merge_count  a workgroup = a tile of kCmpTile = 256 queries x one slice of the references, block = tile * n_slices
//                  + slice; the slice passes through LDS in chunks of kCmpChunk = 256 (13 KiB), every lane walks the
//                  chunk with broadcast reads and counts its accepted references: counts[q * n_slices + slice].
//   (k_scan.hip)   the exclusive scan of the counts, in place: query-major, slice-minor -- the order of the list.
//   k_merge_write  the same walk again; a lane writes its pairs from its offset on.  Every walk ascends, so the list is
//                  in (q, r) order whatever the slicing.  A workgroup whose 256 counts are all zero returns before it
//                  loads a chunk -- most of them: duplicates are few and lie in few (tile, slice) cells.
//   k_merge_check  the counts are 32-bit and so is the scan; every count is below 2^30, so the scan has wrapped iff it
//                  descends somewhere.  Launched only for models of more than 65 536 segments (n (n - 1) pairs at most).
// No atomics, no cross-lane traffic but __syncthreads_or; a lane beyond the last query takes part in every barrier and
// writes nothing.
#include "l3d_kernels.h"

namespace l3d {
namespace {

// WRITE = false: count; WRITE = true: the same walk, writing from the scanned offset on
template <bool WRITE>
__device__ __forceinline__ void merge_walk(const MrgArgs& a) {
    __shared__ double s_p[kCmpChunk * 6];          // (P1, P2) of the chunk's references
    __shared__ uint32_t s_line[kCmpChunk];
    const uint32_t tile = blockIdx.x / a.n_slices, slice = blockIdx.x - tile * a.n_slices;
    const uint32_t q = tile * kCmpTile + threadIdx.x;
    const bool in_range = q < a.n;
    const size_t cell = (size_t)q * a.n_slices + slice;
    uint32_t at = 0, end = 0;                      // WRITE: this lane's pairs are pairs[at, end)
    if (WRITE) {
        if (in_range) { at = a.counts[cell]; end = a.counts[cell + 1]; }
        if (!__syncthreads_or(end != at)) return;  // (uniform)
    }
    const CmpQuery me = cmp_query(a.segs + 6 * (size_t)(in_range ? q : 0), in_range ? a.line[q] : 0u, in_range);
    uint32_t n_acc = 0;
    uint32_t r_begin, r_end;
    cmp_slice_range(a.n, slice, a.slice_chunks, r_begin, r_end);
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += kCmpChunk) {
        const uint32_t n = min(kCmpChunk, r_end - r0);
        cmp_stage_chunk(s_p, s_line, a.segs, a.line, r0, n);
        for (uint32_t k = 0; k < n; ++k) {
            cmp_pair(me, s_p + 6 * k, s_line[k], true, a.max_d2, a.min_cos2, a.min_overlap, [&](double, double) {
                if (WRITE) {
                    if (at < a.n_pairs) a.pairs[at] = MrgPair{q, r0 + k};        // (always: the walk is the count's, at < end <= n_pairs)
                    ++at;
                } else {
                    ++n_acc;
                }
            });
        }
    }
    if (!WRITE && in_range) a.counts[cell] = n_acc;
}

__global__ __launch_bounds__(kCmpTile) void k_merge_count(MrgArgs a) { merge_walk<false>(a); }
__global__ __launch_bounds__(kCmpTile) void k_merge_write(MrgArgs a) { merge_walk<true>(a); }

__global__ __launch_bounds__(256) void k_merge_check(MrgArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)a.n * a.n_slices && a.counts[i + 1] < a.counts[i]) *a.wrapped = 1u;
}

uint32_t grid_of(const MrgArgs& a) { return ((a.n + kCmpTile - 1) / kCmpTile) * a.n_slices; }

}  // namespace

hipError_t launch_merge_count(const MrgArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_merge_count, dim3(grid_of(a)), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_merge_write(const MrgArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_merge_write, dim3(grid_of(a)), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_merge_check(const MrgArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    const size_t cells = (size_t)a.n * a.n_slices;
    hipLaunchKernelGGL(k_merge_check, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
