// k_bundle.hip -- the device side of the joint bundle of cameras and 3D lines (host side: l3d_bundle.hip; the
// projection, the association, the observation list and the spans are §28's, unchanged).  No counterpart in the reference.
// The arithmetic is the contract of §29, fp64 in the order written there (the library is built with -ffp-contract=off), so
// that tests/bundle_model.py follows it operation for operation.  No atomics, no inline assembly.  A CELL is a (line,
// camera) pair with at least one observation; cells are numbered by (line, camera).
//   k_bundle_cells   one lane per cell: the image line of the carrier in the camera and the ten columns of §29.4 once,
//                    then the cell's observations in order, every one of the 67 sums from +0.0, left to right.  A held
//                    line's cell leaves its line parts at +0.0.
//   k_bundle_lines   one lane per eligible line: H_ll and b_l over the line's cells in ascending order, mu times the
//                    diagonal added, the 4 x 4 Cholesky factor in §23's order; a pivot that is not finite and > 0 holds
//                    the line for the step (line_ok = 0).  Else W = L^-1 H_cl^T per cell and v = L^-1 b_l.
//   k_bundle_reduce  one wave per ordered pair (a, b) of free cameras, four pairs per workgroup; the pairs with a > b
//                    leave at once.  Lane j takes the cells j, j + 64, .. of camera a, looks the cell of the same line in
//                    camera b up in the slot table and adds W_a^T W_b (36); on a = b also H_cc, b_c (27) over ALL the
//                    camera's cells and W^T v (6).  Then the tree of §23 inside the wave, stride 32 .. 1; lane 0 writes.
//   k_bundle_update  one lane per eligible line: delta_l = L^-T (-v - sum over the cells of W delta_c) and the trial
//                    carrier; a line held for the step keeps its carrier.
//   k_bundle_cost    one lane per observation: rho(s) at the trial cameras and carriers, tiles of 256 by the tree of
//                    k_pose_normal.  The host adds the tiles in ascending order.
#include "l3d_bundle.h"

namespace l3d {
namespace {

// the sums of one cell; kLine: the line is eligible and its four columns take part
template <bool kLine>
__device__ __forceinline__ void cell_sums(const BundleArgs& a, uint32_t cell, const PoseCam& pc, const double* AB, double* acc) {
    constexpr int NC = kLine ? 10 : 6;
    d3 Y1, Y2;
    double lam[3], nu;
    if (!bundle_image_line(pc, AB, Y1, Y2, lam, nu)) return;
    const d3 Nc = cross(Y1, Y2), Dc = Y2 - Y1;
    const double N[3] = {Nc.x, Nc.y, Nc.z}, D[3] = {Dc.x, Dc.y, Dc.z};
    // the columns: e_i x N (rotation), e_i x D (translation); (R e_j) x Y2 for A and Y1 x (R e_j) for B
    double dN[NC][3] = {{0.0, -N[2], N[1]}, {N[2], 0.0, -N[0]}, {-N[1], N[0], 0.0},
                        {0.0, -D[2], D[1]}, {D[2], 0.0, -D[0]}, {-D[1], D[0], 0.0}};
    if (kLine) {
        double e1[3], e2[3];
        bundle_basis(AB, e1, e2);
        const d3 r1 = mul33(pc.R, d3{e1[0], e1[1], e1[2]}), r2 = mul33(pc.R, d3{e2[0], e2[1], e2[2]});
        const d3 c6 = cross(r1, Y2), c7 = cross(r2, Y2), c8 = cross(Y1, r1), c9 = cross(Y1, r2);
        dN[NC - 4][0] = c6.x; dN[NC - 4][1] = c6.y; dN[NC - 4][2] = c6.z;
        dN[NC - 3][0] = c7.x; dN[NC - 3][1] = c7.y; dN[NC - 3][2] = c7.z;
        dN[NC - 2][0] = c8.x; dN[NC - 2][1] = c8.y; dN[NC - 2][2] = c8.z;
        dN[NC - 1][0] = c9.x; dN[NC - 1][1] = c9.y; dN[NC - 1][2] = c9.z;
    }
    const double nu3 = (nu * nu) * nu;
    double dl[NC][3], B[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        bundle_kt(pc.M, dN[i], dl[i]);
        B[i] = (lam[0] * dl[i][0] + lam[1] * dl[i][1]) / nu3;
    }
    for (uint32_t r = a.cell_off[cell]; r < a.cell_off[cell + 1]; ++r) {
        const LoObs o = a.obs[r];
        const double up = (lam[0] * o.p1x + lam[1] * o.p1y) + lam[2], uq = (lam[0] * o.p2x + lam[1] * o.p2y) + lam[2];
        const double rp = up / nu, rq = uq / nu;
        double Jp[NC], Jq[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            Jp[i] = ((dl[i][0] * o.p1x + dl[i][1] * o.p1y) + dl[i][2]) / nu - up * B[i];
            Jq[i] = ((dl[i][0] * o.p2x + dl[i][1] * o.p2y) + dl[i][2]) / nu - uq * B[i];
        }
        double rho, w;
        lo_huber(rp * rp + rq * rq, rho, w);
        int k = kBcCC;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + w * (Jp[i] * Jp[j] + Jq[i] * Jq[j]);
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[kBcBC + i] = acc[kBcBC + i] + w * (Jp[i] * rp + Jq[i] * rq);
        if (kLine) {
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[kBcCL + 4 * i + j] = acc[kBcCL + 4 * i + j] + w * (Jp[i] * Jp[NC - 4 + j] + Jq[i] * Jq[NC - 4 + j]);
            k = kBcLL;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j, ++k)
                    acc[k] = acc[k] + w * (Jp[NC - 4 + i] * Jp[NC - 4 + j] + Jq[NC - 4 + i] * Jq[NC - 4 + j]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[kBcBL + i] = acc[kBcBL + i] + w * (Jp[NC - 4 + i] * rp + Jq[NC - 4 + i] * rq);
        }
        acc[kBcRho] = acc[kBcRho] + rho;
        acc[kBcCount] = acc[kBcCount] + 1.0;
    }
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_cells(BundleArgs a) {
    const uint32_t cell = blockIdx.x * kBundleBlock + threadIdx.x;
    if (cell >= a.n_cells) return;
    const uint32_t l = a.cell_line[cell];
    const PoseCam pc = a.cams[a.cell_cam[cell]];
    const double* ab = a.AB + 6 * (size_t)l;
    const double AB[6] = {ab[0], ab[1], ab[2], ab[3], ab[4], ab[5]};
    double acc[kBundleCell];
#pragma unroll
    for (uint32_t k = 0; k < kBundleCell; ++k) acc[k] = 0.0;
    if (a.is_eligible[l]) cell_sums<true>(a, cell, pc, AB, acc);
    else cell_sums<false>(a, cell, pc, AB, acc);
    double* out = a.cells + (size_t)kBundleCell * cell;
#pragma unroll
    for (uint32_t k = 0; k < kBundleCell; ++k) out[k] = acc[k];
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_lines(BundleArgs a) {
    const uint32_t e = blockIdx.x * kBundleBlock + threadIdx.x;
    if (e >= a.n_eligible) return;
    const uint32_t l = a.eligible[e];
    const uint32_t c0 = a.line_cell_off[l], c1 = a.line_cell_off[l + 1];
    double H[10], b[4];
#pragma unroll
    for (int k = 0; k < 10; ++k) H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = 0.0;
    for (uint32_t c = c0; c < c1; ++c) {
        const double* s = a.cells + (size_t)kBundleCell * c;
#pragma unroll
        for (int k = 0; k < 10; ++k) H[k] = H[k] + s[kBcLL + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = b[k] + s[kBcBL + k];
    }
    // H(i, j), i <= j, at H[row[i] + (j - i)]; the diagonal damped; the factor column by column (§23's loops)
    constexpr int row[4] = {0, 4, 7, 9};
    double L[4][4];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double h = H[row[j]];
        double p = h + a.mu * h;
#pragma unroll
        for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
        if (!(p > 0.0) || !(fabs(p) <= 1.7976931348623157e308)) ok = false;
        L[j][j] = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double v = H[row[j] + (i - j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    a.line_ok[l] = ok ? 1u : 0u;
    if (!ok) return;
    BundleFactor f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) f.L[i * (i + 1) / 2 + j] = L[i][j];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * f.v[k];
        f.v[i] = v / L[i][i];
    }
    a.factor[l] = f;
    for (uint32_t c = c0; c < c1; ++c) {
        const double* s = a.cells + (size_t)kBundleCell * c + kBcCL;
        double* W = a.W + 24 * (size_t)c;
#pragma unroll
        for (int col = 0; col < 6; ++col) {
            double y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double v = s[4 * col + i];
#pragma unroll
                for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
                y[i] = v / L[i][i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) W[4 * col + i] = y[i];
        }
    }
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_reduce(BundleArgs a) {
    const uint32_t pair = blockIdx.x * (kBundleBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (pair >= a.n_free * a.n_free) return;
    const uint32_t fa = pair / a.n_free, fb = pair - fa * a.n_free;
    if (fa > fb) return;                         // (the whole wave)
    const bool diag = fa == fb;
    const uint32_t ca = a.free_cam[fa], cb = a.free_cam[fb];
    double ww[36], hc[27], wv[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) ww[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 27; ++k) hc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) wv[k] = 0.0;
    for (uint32_t k = a.cam_cell_off[ca] + lane; k < a.cam_cell_off[ca + 1]; k += 64) {
        const uint32_t cell = a.cam_cells[k], l = a.cell_line[cell];
        if (diag) {
            const double* s = a.cells + (size_t)kBundleCell * cell;
#pragma unroll
            for (int t = 0; t < 27; ++t) hc[t] = hc[t] + s[t];
        }
        if (!a.line_ok[l]) continue;
        const double* Wa = a.W + 24 * (size_t)cell;
        if (diag) {
            const double* v = a.factor[l].v;
#pragma unroll
            for (int i = 0; i < 6; ++i)
                wv[i] = wv[i] + (((Wa[4 * i] * v[0] + Wa[4 * i + 1] * v[1]) + Wa[4 * i + 2] * v[2]) + Wa[4 * i + 3] * v[3]);
        }
        const int32_t other = diag ? (int32_t)cell : a.slot[(size_t)l * a.n_cams + cb];
        if (other < 0) continue;
        const double* Wb = a.W + 24 * (size_t)other;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j)
                ww[6 * i + j] = ww[6 * i + j] +
                                (((Wa[4 * i] * Wb[4 * j] + Wa[4 * i + 1] * Wb[4 * j + 1]) + Wa[4 * i + 2] * Wb[4 * j + 2]) + Wa[4 * i + 3] * Wb[4 * j + 3]);
    }
    // inside the wave: stride 32, 16, 8, 4, 2, 1 (only the lanes below the stride are read afterwards)
#pragma unroll
    for (uint32_t stride = 32; stride >= 1; stride >>= 1) {
#pragma unroll
        for (int k = 0; k < 36; ++k) ww[k] = ww[k] + __shfl_down(ww[k], stride);
        if (diag) {
#pragma unroll
            for (int k = 0; k < 27; ++k) hc[k] = hc[k] + __shfl_down(hc[k], stride);
#pragma unroll
            for (int k = 0; k < 6; ++k) wv[k] = wv[k] + __shfl_down(wv[k], stride);
        }
    }
    if (lane != 0) return;
    double* out = a.blocks + 36 * (size_t)pair;
    if (diag) {
        constexpr int row[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double h = i <= j ? hc[row[i] + (j - i)] : hc[row[j] + (i - j)];
                out[6 * i + j] = (i == j ? h + a.mu * h : h) - ww[6 * i + j];
            }
            a.rhs[6 * (size_t)fa + i] = hc[21 + i] - wv[i];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 36; ++k) out[k] = 0.0 - ww[k];
    }
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_update(BundleArgs a) {
    const uint32_t e = blockIdx.x * kBundleBlock + threadIdx.x;
    if (e >= a.n_eligible) return;
    const uint32_t l = a.eligible[e];
    const double* ab = a.AB + 6 * (size_t)l;
    const double AB[6] = {ab[0], ab[1], ab[2], ab[3], ab[4], ab[5]};
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    double* out = a.AB_trial + 6 * (size_t)l;
    if (a.line_ok[l]) {
        const BundleFactor f = a.factor[l];
        double t[4] = {-f.v[0], -f.v[1], -f.v[2], -f.v[3]};
        for (uint32_t c = a.line_cell_off[l]; c < a.line_cell_off[l + 1]; ++c) {
            const int32_t fc = a.cam_free[a.cell_cam[c]];
            if (fc < 0) continue;
            const double* W = a.W + 24 * (size_t)c;
            const double* dc = a.delta_c + 6 * (size_t)fc;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] = t[r] - W[4 * i + r] * dc[i];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double v = t[i];
#pragma unroll
            for (int k = i + 1; k < 4; ++k) v = v - f.L[k * (k + 1) / 2 + i] * x[k];
            x[i] = v / f.L[i * (i + 1) / 2 + i];
        }
        double e1[3], e2[3];
        bundle_basis(AB, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out[k] = AB[k] + (x[0] * e1[k] + x[1] * e2[k]);
            out[3 + k] = AB[3 + k] + (x[2] * e1[k] + x[3] * e2[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = AB[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a.delta_l[4 * (size_t)l + k] = x[k];
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_cost(BundleArgs a) {
    __shared__ double s_w[kBundleBlock / 64];
    const uint32_t r = blockIdx.x * kBundleBlock + threadIdx.x;
    double v = 0.0;
    if (r < a.n_obs) {
        const uint32_t l = bundle_last_not_above(a.obs_off, a.n_lines, r);
        const LoObs o = a.obs[r];
        const double* ab = a.AB_trial + 6 * (size_t)l;
        const double AB[6] = {ab[0], ab[1], ab[2], ab[3], ab[4], ab[5]};
        v = bundle_rho(a.cams_trial[o.cam], AB, o);
    }
#pragma unroll
    for (uint32_t stride = 32; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) a.tiles[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

}  // namespace

hipError_t launch_bundle_cells(const BundleArgs& a, hipStream_t st) {
    if (!a.n_cells) return hipSuccess;
    hipLaunchKernelGGL(k_bundle_cells, dim3((a.n_cells + kBundleBlock - 1) / kBundleBlock), dim3(kBundleBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_bundle_lines(const BundleArgs& a, hipStream_t st) {
    if (!a.n_eligible) return hipSuccess;
    hipLaunchKernelGGL(k_bundle_lines, dim3((a.n_eligible + kBundleBlock - 1) / kBundleBlock), dim3(kBundleBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_bundle_reduce(const BundleArgs& a, hipStream_t st) {
    if (!a.n_free) return hipSuccess;
    const uint32_t pairs = a.n_free * a.n_free, per = kBundleBlock / 64;
    hipLaunchKernelGGL(k_bundle_reduce, dim3((pairs + per - 1) / per), dim3(kBundleBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_bundle_update(const BundleArgs& a, hipStream_t st) {
    if (!a.n_eligible) return hipSuccess;
    hipLaunchKernelGGL(k_bundle_update, dim3((a.n_eligible + kBundleBlock - 1) / kBundleBlock), dim3(kBundleBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_bundle_cost(const BundleArgs& a, hipStream_t st) {
    if (!a.n_obs) return hipSuccess;
    hipLaunchKernelGGL(k_bundle_cost, dim3((a.n_obs + kBundleBlock - 1) / kBundleBlock), dim3(kBundleBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
