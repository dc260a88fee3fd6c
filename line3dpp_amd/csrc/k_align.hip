// k_align.hip -- the device side of the alignment of two 3D line models (host side: l3d_align.hip).  No
// counterpart in the reference.  The arithmetic is the contract of §23, fp64 in the order written there (the library is
// built with -ffp-contract=off), so that tests/align_model.py follows it operation for operation.  No atomics, no
// inline assembly.
//   k_align_transform  one lane per segment: both end points under y = scale * R(q) x + t, by sim_rotation and
//                      sim_point of l3d_dev.h -- the functions l3d_transform_segments runs on the host.
//   k_align_normal     a tile of kCmpTile = 256 consecutive queries per workgroup of four waves, one lane per query, as
//                      k_compare.  A matched lane forms its term of kAlnTerms = 37 doubles in registers -- H (28), b (7),
//                      cost, count: term(P1) + term(P2) --, an unmatched lane and a lane past n_q hold 37 times +0.0.
//                      The tile's sum is a fixed tree: inside a wave v[i] = v[i] + v[i + stride] for stride 32 .. 1 by
//                      __shfl_down, the four wave sums through LDS as (W0 + W1) + (W2 + W3).  The host adds the tiles in
//                      ascending order, so no sum depends on scheduling or on the slicing of the comparison before it.
#include "l3d_kernels.h"

namespace l3d {
namespace {

__global__ __launch_bounds__(kCmpTile) void k_align_transform(AlnTransformArgs a) {
    const uint32_t i = blockIdx.x * kCmpTile + threadIdx.x;
    if (i >= a.n) return;
    double R[9];
    sim_rotation(a.q, R);
    const double* x = a.in + 6 * (size_t)i;
    double* y = a.out + 6 * (size_t)i;
    sim_point(a.scale, R, a.t, x, y);
    sim_point(a.scale, R, a.t, x + 3, y + 3);
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The term of one end point x of a matched query: reference (B, d, L2), centre c.  kFirst: v = term, else v = v + term.
template <bool kFirst>
__device__ __forceinline__ void aln_point(const double* x, const double* B, const double* d, double L2, const double* c, double* v) {
    const double w[3] = {x[0] - B[0], x[1] - B[1], x[2] - B[2]};
    const double sw = dot3(d, w) / L2;
    const double r[3] = {w[0] - d[0] * sw, w[1] - d[1] * sw, w[2] - d[2] * sw};
    const double z[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]};
    // the columns: e_i x z (rotation), z (scale), e_i (translation)
    const double a[7][3] = {{0.0, -z[2], z[1]}, {z[2], 0.0, -z[0]}, {-z[1], z[0], 0.0}, {z[0], z[1], z[2]},
                            {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double g[7][3];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double s = dot3(d, a[i]) / L2;
        g[i][0] = a[i][0] - d[0] * s; g[i][1] = a[i][1] - d[1] * s; g[i][2] = a[i][2] - d[2] * s;
    }
    int k = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = i; j < 7; ++j, ++k) {
            const double h = dot3(g[i], g[j]);
            v[k] = kFirst ? h : v[k] + h;
        }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double b = dot3(g[i], r);
        v[28 + i] = kFirst ? b : v[28 + i] + b;
    }
    const double cost = dot3(r, r);
    v[35] = kFirst ? cost : v[35] + cost;
}

__global__ __launch_bounds__(kCmpTile) void k_align_normal(AlnNormalArgs a) {
    __shared__ double s_w[4][kAlnTerms];
    const uint32_t q = blockIdx.x * kCmpTile + threadIdx.x;
    double v[kAlnTerms];
#pragma unroll
    for (uint32_t k = 0; k < kAlnTerms; ++k) v[k] = 0.0;
    if (q < a.n_q) {
        const int32_t seg = a.match[q].segment;
        if (seg >= 0 && (uint32_t)seg < a.n_r) {
            const double* rp = a.r + 6 * (size_t)seg;
            const double* xp = a.q + 6 * (size_t)q;
            const double B[3] = {rp[0], rp[1], rp[2]};
            const double d[3] = {rp[3] - B[0], rp[4] - B[1], rp[5] - B[2]};
            const double L2 = dot3(d, d);
            const double x1[3] = {xp[0], xp[1], xp[2]}, x2[3] = {xp[3], xp[4], xp[5]};
            aln_point<true>(x1, B, d, L2, a.c, v);
            aln_point<false>(x2, B, d, L2, a.c, v);
            v[36] = 1.0;
        }
    }
    // inside the wave: stride 32, 16, 8, 4, 2, 1 (a lane whose partner lies past the wave gets its own value back; only
    // the lanes below the stride are read afterwards)
#pragma unroll
    for (uint32_t stride = 32; stride >= 1; stride >>= 1)
#pragma unroll
        for (uint32_t k = 0; k < kAlnTerms; ++k) v[k] = v[k] + __shfl_down(v[k], stride);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
#pragma unroll
        for (uint32_t k = 0; k < kAlnTerms; ++k) s_w[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < kAlnTerms) {
        const uint32_t k = threadIdx.x;
        a.tiles[(size_t)blockIdx.x * kAlnTerms + k] = (s_w[0][k] + s_w[1][k]) + (s_w[2][k] + s_w[3][k]);
    }
}

}  // namespace

hipError_t launch_align_transform(const AlnTransformArgs& a, hipStream_t st) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(k_align_transform, dim3((a.n + kCmpTile - 1) / kCmpTile), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_align_normal(const AlnNormalArgs& a, hipStream_t st) {
    if (!a.n_q) return hipSuccess;
    hipLaunchKernelGGL(k_align_normal, dim3((a.n_q + kCmpTile - 1) / kCmpTile), dim3(kCmpTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
