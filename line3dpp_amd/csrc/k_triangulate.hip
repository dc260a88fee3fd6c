// k_triangulate.hip -- linear homogeneous triangulation of tie points from their observations: what main_pix4d.cpp does
// per feature before it can compute a median depth (linearHomTriangulation, main_pix4d.cpp:34-69, in the OpenMP loop of
// :354-372).  One lane per point, fp64 throughout:
//   per observation (camera c, pixel (x, y)) the two rows (0, -1, y) P_c and (1, 0, -x) P_c; M = A^T A, ten sums of the
//   symmetric 4x4 in observation order;
//   the singular vector of M for its smallest singular value by cyclic Jacobi rotations on the 4x4 in registers (the
//   reference takes JacobiSVD(AtA).matrixV().col(3); M is symmetric, so its singular vectors are its eigenvectors and its
//   singular values their magnitudes); one correction of that vector from its residual M w - lambda w, the product M w
//   taken as if in twice the working precision: the rotations leave an error of eps |M| / gap in w, which is 1e-10 of the
//   scene where M is close to rank 2 (three observations by one camera), the corrected w is good to the last
//   bits of a double; X = w[0:3] / w[3], the sign of w cancels;
//   valid = more than two observations and norm(X) > L3D_EPS (:362-370): a NaN is invalid, an infinite X is valid.
// The projection matrices sit in LDS when they fit (12 doubles per camera, kTriLdsBytes), otherwise they are read through
// the cache.  The solve touches no memory: every index into the 4x4s is a compile-time constant after unrolling.
#include "l3d_kernels.h"

namespace l3d {
namespace {

constexpr int kTriSweeps = 30;      // cyclic sweeps at most; a 4x4 is diagonal to working precision after 5 to 7

// upper triangle of the symmetric matrix: element (i, j) for any order of i, j
#define TRI_A(i, j) a[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]
#define TRI_M(i, j) m[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]

// one Jacobi rotation in the (P, Q) plane (Rutishauser's form: t from the smaller root, updates by s and tau)
template <int P, int Q>
__device__ __forceinline__ void tri_rotate(double (&a)[4][4], double (&v)[4][4], int sweep) {
    const double apq = a[P][Q];
    const double g = 100.0 * fabs(apq);
    // after the first sweeps an element that no longer registers beside either diagonal entry is dropped
    if (sweep > 3 && fabs(a[P][P]) + g == fabs(a[P][P]) && fabs(a[Q][Q]) + g == fabs(a[Q][Q])) {
        a[P][Q] = 0.0;
        return;
    }
    if (apq == 0.0) return;
    const double h = a[Q][Q] - a[P][P];
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j != P && j != Q) {
            const double x = TRI_A(j, P), y = TRI_A(j, Q);
            TRI_A(j, P) = x - s * (y + x * tau);
            TRI_A(j, Q) = y + s * (x - y * tau);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double x = v[j][P], y = v[j][Q];
        v[j][P] = x - s * (y + x * tau);
        v[j][Q] = y + s * (x - y * tau);
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_triangulate(TriArgs t) {
    extern __shared__ double s_P[];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < 12u * t.n_cameras; i += blockDim.x) s_P[i] = t.P[i];
        __syncthreads();
    }
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n_points) return;
    const uint64_t o0 = t.off[i], o1 = t.off[i + 1];
    double X[3] = {0.0, 0.0, 0.0};
    bool valid = false;
    if (o1 - o0 > 2) {
        double a[4][4], v[4][4], m[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) { a[r][c] = 0.0; v[r][c] = r == c ? 1.0 : 0.0; }
        for (uint64_t o = o0; o < o1; ++o) {
            const double* Pc = (LDS ? (const double*)s_P : t.P) + 12 * (size_t)t.cam[o];
            const double x = t.xy[2 * o], y = t.xy[2 * o + 1];
            double r1[4], r2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r1[k] = y * Pc[8 + k] - Pc[4 + k];        // (0, -1, y) P
                r2[k] = Pc[k] - x * Pc[8 + k];            // (1, 0, -x) P
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = r; c < 4; ++c) a[r][c] += r1[r] * r1[c] + r2[r] * r2[c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) m[r][c] = a[r][c];   // M itself, for the residual
        for (int sweep = 0; sweep < kTriSweeps; ++sweep) {
            const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
            if (!(off > 0.0)) break;                      // diagonal -- or a NaN, which no rotation mends
            tri_rotate<0, 1>(a, v, sweep); tri_rotate<0, 2>(a, v, sweep); tri_rotate<0, 3>(a, v, sweep);
            tri_rotate<1, 2>(a, v, sweep); tri_rotate<1, 3>(a, v, sweep); tri_rotate<2, 3>(a, v, sweep);
        }
        // the column of the diagonal entry of smallest magnitude (= the smallest singular value of M)
        double best = fabs(a[0][0]), w[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
        int kb = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const bool take = fabs(a[k][k]) < best;
            best = take ? fabs(a[k][k]) : best;
            kb = take ? k : kb;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = take ? v[j][k] : w[j];
        }
        // one correction of w from its residual.  r = M w as hi + lo, every product with its rounding error (fma) and every
        // sum with its own (Ogita, Rump & Oishi's Dot2); lambda = w.r / w.w; rho = r - lambda w; then to first order
        // w -= sum over the other columns j of v_j (v_j . rho) / (a_jj - lambda).  A column whose a_jj equals lambda adds nothing.
        double rho[4], rl[4], lam = 0.0, ww = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double hi = 0.0, lo = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double x = TRI_M(r, c), p = x * w[c], e = fma(x, w[c], -p);
                const double t = hi + p, bb = t - hi;
                lo += ((hi - (t - bb)) + (p - bb)) + e;
                hi = t;
            }
            rho[r] = hi; rl[r] = lo;
            lam += w[r] * (hi + lo);
            ww += w[r] * w[r];
        }
        lam /= ww;
#pragma unroll
        for (int r = 0; r < 4; ++r) rho[r] = (rho[r] - lam * w[r]) + rl[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double num = (v[0][j] * rho[0] + v[1][j] * rho[1]) + (v[2][j] * rho[2] + v[3][j] * rho[3]);
            const double den = a[j][j] - lam;
            const double c = (j != kb && den != 0.0) ? num / den : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) w[r] -= c * v[r][j];
        }
        // (a NaN in M ends the sweeps at once with v = I: the residual is NaN and so is X, invalid)
        X[0] = w[0] / w[3]; X[1] = w[1] / w[3]; X[2] = w[2] / w[3];
        valid = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) > kEps;   // false for a NaN
        if (!valid) { X[0] = 0.0; X[1] = 0.0; X[2] = 0.0; }
    }
    t.X[3 * i] = X[0]; t.X[3 * i + 1] = X[1]; t.X[3 * i + 2] = X[2];
    t.valid[i] = valid ? 1 : 0;
}

#undef TRI_A
#undef TRI_M

}  // namespace

hipError_t launch_triangulate(const TriArgs& t, hipStream_t st) {
    if (!t.n_points) return hipSuccess;
    const uint32_t blocks = (uint32_t)((t.n_points + 255) / 256);
    const size_t lds = 96 * (size_t)t.n_cameras;
    if (lds <= kTriLdsBytes) hipLaunchKernelGGL(k_triangulate<true>, dim3(blocks), dim3(256), lds, st, t);
    else hipLaunchKernelGGL(k_triangulate<false>, dim3(blocks), dim3(256), 0, st, t);
    return hipGetLastError();
}

}  // namespace l3d
