// k_compare.hip -- two 3D line models compared segment by segment (host side: l3d_compare.hip).  No
// counterpart in the reference.  The arithmetic is the contract of §18, fp64 in the order written there (the library is
// built with -ffp-contract=off), so that tests/compare_model.py follows it operation for operation.
//   k_compare        the unit of work is (a TILE of kCmpTile = 256 consecutive queries) x (one SLICE of the references):
//                    one workgroup of four waves, one lane per query; block = tile * n_slices + slice.  A model has a few
//                    thousand segments -- a dozen tiles on 256 compute units -- so the references are cut into slices of
//                    slice_chunks chunks and every slice walks in a workgroup of its own.  The slice's references pass
//                    through LDS in chunks of kCmpChunk = 256 (end points 12 KiB, line indices 1 KiB), loaded coalesced
//                    by the whole workgroup; every lane walks the chunk with broadcast reads (all lanes read the same
//                    address: no bank conflict) and keeps (bits(D2), index, frac) of its best and its count in registers
//                    -- no atomics, no cross-lane traffic; the ascending walk makes the smaller index win equal distances
//                    inside a slice.  A reference that is a point is skipped by the whole workgroup; the tests are
//                    ordered cheapest first (same line, angle without a division, distance with one, overlap with
//                    three): a pair is accepted iff all hold, so the order changes nothing.  Lanes beyond the last query
//                    take part in every barrier and write nothing.  With one slice the kernel writes the final record,
//                    with more a CmpPartial per (query, slice).
//   k_compare_merge  one lane per query reads its partials in ascending slice order and replaces its best only on
//                    strictly smaller bits: the lower slice, and so the lower index, wins equal distances, whatever the
//                    slicing.  It adds the counts and writes the final record.
#include "l3d_kernels.h"

namespace l3d {
namespace {

__global__ __launch_bounds__(kCmpTile) void k_compare(CmpArgs a) {
    __shared__ double s_p[kCmpChunk * 6];          // (P1, P2) of the chunk's references
    __shared__ uint32_t s_line[kCmpChunk];
    const uint32_t tile = blockIdx.x / a.n_slices, slice = blockIdx.x - tile * a.n_slices;
    const uint32_t q = tile * kCmpTile + threadIdx.x;
    const bool in_range = q < a.n_q;
    const CmpQuery me = cmp_query(a.q + 6 * (size_t)(in_range ? q : 0), in_range ? a.q_line[q] : 0u, in_range);
    unsigned long long best_bits = ~0ull;
    uint32_t best_r = 0xFFFFFFFFu, n_acc = 0;
    double best_frac = 0.0;
    uint32_t r_begin, r_end;
    cmp_slice_range(a.n_r, slice, a.slice_chunks, r_begin, r_end);
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += kCmpChunk) {
        const uint32_t n = min(kCmpChunk, r_end - r0);
        cmp_stage_chunk(s_p, s_line, a.r, a.r_line, r0, n);
        for (uint32_t k = 0; k < n; ++k) {
            // steps 1-6: l3d_kernels.h
            cmp_pair(me, s_p + 6 * k, s_line[k], a.exclude_same_line != 0, a.max_d2, a.min_cos2, a.min_overlap, [&](double D2, double frac) {
                ++n_acc;
                const unsigned long long bits = (unsigned long long)__double_as_longlong(D2);
                if (bits < best_bits) { best_bits = bits; best_r = r0 + k; best_frac = frac; }
            });
        }
    }
    if (!in_range) return;
    if (a.n_slices > 1) {
        a.part[(size_t)q * a.n_slices + slice] = CmpPartial{best_bits, best_r, n_acc, best_frac, 0.0};
        return;
    }
    CmpOut o{-1, 0xFFFFFFFFu, 0u, 0.0f, 0.0};
    if (n_acc) {
        o.segment = (int32_t)best_r; o.line = a.r_line[best_r]; o.n_accepted = n_acc;
        o.overlap = (float)best_frac; o.d2 = __longlong_as_double((long long)best_bits);
    }
    a.out[q] = o;
}

__global__ __launch_bounds__(kCmpTile) void k_compare_merge(CmpArgs a) {
    const uint32_t q = blockIdx.x * kCmpTile + threadIdx.x;
    if (q >= a.n_q) return;
    const CmpPartial* part = a.part + (size_t)q * a.n_slices;
    unsigned long long best_bits = ~0ull;
    uint32_t best_r = 0xFFFFFFFFu, n_acc = 0;
    double best_frac = 0.0;
    for (uint32_t s = 0; s < a.n_slices; ++s) {
        const CmpPartial p = part[s];
        n_acc += p.n_accepted;
        if (p.n_accepted && p.bits < best_bits) { best_bits = p.bits; best_r = p.index; best_frac = p.frac; }
    }
    CmpOut o{-1, 0xFFFFFFFFu, 0u, 0.0f, 0.0};
    if (n_acc) {
        o.segment = (int32_t)best_r; o.line = a.r_line[best_r]; o.n_accepted = n_acc;
        o.overlap = (float)best_frac; o.d2 = __longlong_as_double((long long)best_bits);
    }
    a.out[q] = o;
}

}  // namespace

hipError_t launch_compare(const CmpArgs& a, hipStream_t st) {
    if (!a.n_q || !a.n_slices) return hipSuccess;
    const uint32_t n_tiles = (a.n_q + kCmpTile - 1) / kCmpTile;
    hipLaunchKernelGGL(k_compare, dim3(n_tiles * a.n_slices), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_compare_merge(const CmpArgs& a, hipStream_t st) {
    if (!a.n_q || a.n_slices < 2) return hipSuccess;
    hipLaunchKernelGGL(k_compare_merge, dim3((a.n_q + kCmpTile - 1) / kCmpTile), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
