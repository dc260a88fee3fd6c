// k_wireframe.hip -- the junctions of a 3D line model: the pairs of segments that meet, as a list (stage 1;
// host side: l3d_wireframe.hip, the graph: l3d_wireframe.h).  No counterpart in the reference.  A pair a < b is a
// junction iff both are live, line(a) != line(b) and wf_pair below accepts it with a in the first role.  k_merge's two
// walks over k_compare's tiling:
//   k_wf_count   a workgroup = a tile of kCmpTile = 256 queries x one slice of the references, block = tile * n_slices +
//                slice; the slice passes through LDS in chunks of kCmpChunk = 256 (cmp_stage_chunk), every lane walks the
//                chunk with broadcast reads and counts its junctions: counts[q * n_slices + slice].
//   (k_scan.hip) the exclusive scan of the counts, in place: query-major, slice-minor -- the order of the list.
//   k_wf_write   the same walk again; a lane writes its records from its offset on.  Every walk ascends, so the list is in
//                (a, b) order whatever the slicing.  A workgroup whose 256 counts are all zero returns before it loads a
//                chunk.
//   k_wf_check   the counts are 32-bit and so is the scan; every count is below 2^30, so the scan has wrapped iff it
//                descends somewhere.  Launched only for models of more than 92 682 segments (n (n - 1) / 2 pairs at most).
// THE TRIANGULAR WALK: only a < b is evaluated.  A workgroup whose slice ends at or below its tile's first query -- its
// last reference r_end - 1 <= the first query -- has no such pair: it leaves before it stages a chunk, the count pass
// after writing its zeros (the scan reads every cell).  In the others a lane skips the references r <= q.
// No atomics, no cross-lane traffic but __syncthreads_or; a lane beyond the last query takes part in every barrier and
// writes nothing.
#include "l3d_kernels.h"

namespace l3d {
namespace {

static_assert(kCmpTile == kCmpChunk, "the triangular walk takes a tile's first query for the start of a chunk");

// the quantities of the first segment of a pair, computed once per lane
struct WfQuery { double px, py, pz, ex, ey, ez, A, La; uint32_t line; bool live; };
__device__ __forceinline__ WfQuery wf_query(const double* v, uint32_t line, bool in_range) {
    WfQuery q{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, false};
    if (in_range) {
        q.px = v[0]; q.py = v[1]; q.pz = v[2];
        q.ex = v[3] - q.px; q.ey = v[4] - q.py; q.ez = v[5] - q.pz;
        q.line = line;
    }
    q.A = q.ex * q.ex + q.ey * q.ey + q.ez * q.ez;
    q.La = sqrt(q.A);
    q.live = in_range && q.A > 0.0;
    return q;
}

// Stage 1 of DESIGN §24 for the pair (q, the segment r6 = (P1, P2)); calls accept(sa, sb, gap2) iff it is a junction.  A
// pair is accepted iff all the tests hold, so their order changes nothing; every test is written so that a NaN fails it.
template <class Accept>
__device__ __forceinline__ void wf_pair(const WfQuery& q, const double* r6, uint32_t r_line, double max_d2, double max_extension,
                                        double min_sin2, Accept&& accept) {
    const double bx = r6[0], by = r6[1], bz = r6[2];
    const double fx = r6[3] - bx, fy = r6[4] - by, fz = r6[5] - bz;              // eb
    const double C = fx * fx + fy * fy + fz * fz;
    if (!(C > 0.0)) return;                                                      // (uniform over the workgroup)
    if (!q.live || r_line == q.line) return;
    const double B = q.ex * fx + q.ey * fy + q.ez * fz;
    const double AC = q.A * C;
    const double den = AC - B * B;
    if (!(den > 0.0 && den >= min_sin2 * AC)) return;
    const double wx = q.px - bx, wy = q.py - by, wz = q.pz - bz;
    const double D = q.ex * wx + q.ey * wy + q.ez * wz;
    const double E = fx * wx + fy * wy + fz * wz;
    const double sa = (B * E - C * D) / den, sb = (q.A * E - B * D) / den;
    const double Lb = sqrt(C);
    const double ta = sa * q.La, tb = sb * Lb;
    if (!(ta >= -max_extension && ta <= q.La + max_extension && tb >= -max_extension && tb <= Lb + max_extension)) return;
    const double gx = (q.px + sa * q.ex) - (bx + sb * fx), gy = (q.py + sa * q.ey) - (by + sb * fy), gz = (q.pz + sa * q.ez) - (bz + sb * fz);
    const double gap2 = gx * gx + gy * gy + gz * gz;
    if (!(gap2 <= max_d2)) return;
    accept(sa, sb, gap2);
}

// WRITE = false: count; WRITE = true: the same walk, writing from the scanned offset on
template <bool WRITE>
__device__ __forceinline__ void wf_walk(const WfArgs& a) {
    __shared__ double s_p[kCmpChunk * 6];          // (P1, P2) of the chunk's references
    __shared__ uint32_t s_line[kCmpChunk];
    const uint32_t tile = blockIdx.x / a.n_slices, slice = blockIdx.x - tile * a.n_slices;
    const uint32_t q = tile * kCmpTile + threadIdx.x;
    const bool in_range = q < a.n;
    const size_t cell = (size_t)q * a.n_slices + slice;
    uint32_t r_begin, r_end;
    cmp_slice_range(a.n, slice, a.slice_chunks, r_begin, r_end);
    if (r_end <= tile * kCmpTile + 1) {            // the triangular exit (uniform): no reference above the tile's first query
        if (!WRITE && in_range) a.counts[cell] = 0;
        return;
    }
    uint32_t at = 0, end = 0;                      // WRITE: this lane's records are out[at, end)
    if (WRITE) {
        if (in_range) { at = a.counts[cell]; end = a.counts[cell + 1]; }
        if (!__syncthreads_or(end != at)) return;  // (uniform)
    }
    const WfQuery me = wf_query(a.segs + 6 * (size_t)(in_range ? q : 0), in_range ? a.line[q] : 0u, in_range);
    uint32_t n_acc = 0;
    // (a slice of several chunks: those below the tile's first query hold no reference for it; both are multiples of 256)
    for (uint32_t r0 = max(r_begin, tile * kCmpTile); r0 < r_end; r0 += kCmpChunk) {
        const uint32_t n = min(kCmpChunk, r_end - r0);
        cmp_stage_chunk(s_p, s_line, a.segs, a.line, r0, n);
        for (uint32_t k = 0; k < n; ++k) {
            if (r0 + k <= q) continue;             // a < b only (the lanes beyond the last query: every reference)
            wf_pair(me, s_p + 6 * k, s_line[k], a.max_d2, a.max_extension, a.min_sin2, [&](double sa, double sb, double gap2) {
                if (WRITE) {
                    if (at < a.n_out) a.out[at] = WfJunction{q, r0 + k, sa, sb, gap2};   // (always: the walk is the count's, at < end <= n_out)
                    ++at;
                } else {
                    ++n_acc;
                }
            });
        }
    }
    if (!WRITE && in_range) a.counts[cell] = n_acc;
}

__global__ __launch_bounds__(kCmpTile) void k_wf_count(WfArgs a) { wf_walk<false>(a); }
__global__ __launch_bounds__(kCmpTile) void k_wf_write(WfArgs a) { wf_walk<true>(a); }

__global__ __launch_bounds__(256) void k_wf_check(WfArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)a.n * a.n_slices && a.counts[i + 1] < a.counts[i]) *a.wrapped = 1u;
}

uint32_t grid_of(const WfArgs& a) { return ((a.n + kCmpTile - 1) / kCmpTile) * a.n_slices; }

}  // namespace

hipError_t launch_wf_count(const WfArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_wf_count, dim3(grid_of(a)), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_wf_write(const WfArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    hipLaunchKernelGGL(k_wf_write, dim3(grid_of(a)), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_wf_check(const WfArgs& a, hipStream_t st) {
    if (!a.n || !a.n_slices) return hipSuccess;
    const size_t cells = (size_t)a.n * a.n_slices;
    hipLaunchKernelGGL(k_wf_check, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
