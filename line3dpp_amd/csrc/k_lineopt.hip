// k_lineopt.hip -- the line bundling kernel (l3d_lineopt.h): one launch runs every Levenberg-Marquardt iteration of
// every line, fp64 throughout.
//
// Work shape.  Residual counts per line are small and skewed, so lanes map to residuals: a line with at most
// 16 residuals gets a 16-lane group (4 lines per wave), a longer one a whole wave that loops over its residuals in chunks
// of 64; the wide lines come first, both classes longest first.  Each lane evaluates its residuals (value and 2x4
// Jacobian by forward-mode derivatives), the 10 entries of J^T J, the 4 of J^T r and the cost are summed over the group
// with xor shuffles (every lane ends with the same bits: a + b == b + a), and the damped 4x4 system is solved
// redundantly in every lane, so the group's control flow is uniform and needs no LDS or barrier.
//
// Solver, per line, in the reference solver's default setting where it carries over:
//   * robust loss by the Triggs correction; Huber has rho'' <= 0 everywhere, where the correction keeps only the
//     scaling of residual and Jacobian by sqrt(rho') (the curvature term is applied only where rho'' > 0);
//   * Jacobi column scaling 1 / (1 + |J_j|), fixed at the start point;
//   * LM diagonal diag(J^T J) clamped to [1e-6, 1e32], divided by the trust radius (initially 1e4); an accepted step
//     with gain ratio q divides the radius by max(1/3, 1 - (2q - 1)^3) (at most 1e16) and resets the decrease factor
//     to 2; a rejected step divides the radius by the factor and doubles it; steps are accepted for q > 1e-3;
//   * stopping: max-norm of the gradient <= 1e-10, |cost change| <= 1e-6 cost, |step| <= 1e-8 (|x| + 1e-8),
//     max_iter iterations (accepted and rejected), or a trust radius below 1e-32.
// A step whose model decrease is not positive, whose system is not positive definite or whose evaluation fails is a
// rejected step.  A line whose start point cannot be evaluated keeps its parameters.
#include "l3d_ctx.h"
#include "l3d_lineopt.h"

namespace l3d {
namespace {

constexpr int kAcc = 16;   // J^T J (10, upper triangle row by row), J^T r (4), cost, failed residuals

template <int W>
__device__ __forceinline__ void lo_eval(const LoArgs& a, uint32_t r0, uint32_t r1, uint32_t lane, const double x[4], double acc[kAcc]) {
    for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
    for (uint32_t ri = r0 + lane; ri < r1; ri += W) {
        const LoObs o = a.obs[ri];
        Jet4 r[2];
        if (!lo_residual(x, a.cams[o.cam], o, r)) { acc[15] += 1.0; continue; }
        double rho, rho1;
        lo_huber(r[0].a * r[0].a + r[1].a * r[1].a, rho, rho1);
        const double w = sqrt(rho1);
        double J[2][4], f[2];
        for (int i = 0; i < 2; ++i) { f[i] = w * r[i].a; for (int j = 0; j < 4; ++j) J[i][j] = w * r[i].v[j]; }
        int k = 0;
        for (int p = 0; p < 4; ++p)
            for (int q = p; q < 4; ++q) acc[k++] += J[0][p] * J[0][q] + J[1][p] * J[1][q];
        for (int p = 0; p < 4; ++p) acc[10 + p] += J[0][p] * f[0] + J[1][p] * f[1];
        acc[14] += 0.5 * rho;
    }
    for (int m = W / 2; m >= 1; m >>= 1)
        for (int k = 0; k < kAcc; ++k) acc[k] += __shfl_xor(acc[k], m, W);
}

__device__ __forceinline__ int hidx(int p, int q) {   // (p <= q) -> index into the packed upper triangle
    return p * 4 - p * (p - 1) / 2 + (q - p);
}

// Cholesky solve of the (symmetric positive definite) A y = rhs; false when A is not
__device__ __forceinline__ bool chol4(const double A[4][4], const double rhs[4], double y[4]) {
    double L[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[i][i] = sqrt(s);
            } else L[i][j] = s / L[j][j];
        }
    double z[4];
    for (int i = 0; i < 4; ++i) { double s = rhs[i]; for (int k = 0; k < i; ++k) s -= L[i][k] * z[k]; z[i] = s / L[i][i]; }
    for (int i = 3; i >= 0; --i) { double s = z[i]; for (int k = i + 1; k < 4; ++k) s -= L[k][i] * y[k]; y[i] = s / L[i][i]; }
    return true;
}

__device__ __forceinline__ double gmax(const double* g) {
    return fmax(fmax(fabs(g[0]), fabs(g[1])), fmax(fabs(g[2]), fabs(g[3])));
}

template <int W>
__device__ void lo_solve(const LoArgs& a, uint32_t line, uint32_t lane) {
    const uint32_t r0 = a.res_off[line], r1 = a.res_off[line + 1];
    double x[4] = {a.x0[4 * line], a.x0[4 * line + 1], a.x0[4 * line + 2], a.x0[4 * line + 3]};
    double cur[kAcc], acc[kAcc];
    lo_eval<W>(a, r0, r1, lane, x, cur);
    const double cost0 = cur[14];
    uint32_t it = 0, status = LO_NONE;
    if (cur[15] != 0.0 || !isfinite(cost0)) status = LO_OTHER;
    double s[4];
    for (int j = 0; j < 4; ++j) s[j] = 1.0 / (1.0 + sqrt(cur[hidx(j, j)]));
    double radius = 1e4, decf = 2.0;
    if (status == LO_NONE && gmax(cur + 10) <= 1e-10) status = LO_GRADIENT;
    while (status == LO_NONE) {
        if (it >= a.max_iter) { status = LO_MAX_ITER; break; }
        ++it;
        double A[4][4], D[4][4], b[4], y[4];
        for (int p = 0; p < 4; ++p) {
            b[p] = s[p] * cur[10 + p];
            for (int q = 0; q < 4; ++q) A[p][q] = D[p][q] = s[p] * cur[p <= q ? hidx(p, q) : hidx(q, p)] * s[q];
            D[p][p] += fmin(fmax(A[p][p], 1e-6), 1e32) / radius;
        }
        const double nb[4] = {-b[0], -b[1], -b[2], -b[3]};
        bool valid = chol4(D, nb, y);
        double mcc = 0.0;
        if (valid) {
            double yAy = 0.0, yb = 0.0;
            for (int p = 0; p < 4; ++p) {
                yb += y[p] * b[p];
                double t = 0.0;
                for (int q = 0; q < 4; ++q) t += A[p][q] * y[q];
                yAy += y[p] * t;
            }
            mcc = -(yb + 0.5 * yAy);
            valid = mcc > 0.0 && isfinite(mcc);
        }
        if (valid) {
            double step[4], xn[4], ns = 0.0, nx = 0.0;
            for (int j = 0; j < 4; ++j) { step[j] = s[j] * y[j]; xn[j] = x[j] + step[j]; ns += step[j] * step[j]; nx += x[j] * x[j]; }
            if (sqrt(ns) <= 1e-8 * (sqrt(nx) + 1e-8)) { status = LO_PARAMETER; break; }
            lo_eval<W>(a, r0, r1, lane, xn, acc);
            if (acc[15] == 0.0 && isfinite(acc[14])) {
                const double dc = cur[14] - acc[14];
                const bool ftol = fabs(dc) <= 1e-6 * cur[14];
                const double q = dc / mcc;
                if (q > 1e-3) {
                    for (int j = 0; j < 4; ++j) x[j] = xn[j];
                    for (int k = 0; k < kAcc; ++k) cur[k] = acc[k];
                    const double t = 2.0 * q - 1.0;
                    radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
                    decf = 2.0;
                    if (ftol) { status = LO_FUNCTION; break; }
                    if (gmax(cur + 10) <= 1e-10) { status = LO_GRADIENT; break; }
                    continue;
                }
                if (ftol) { status = LO_FUNCTION; break; }
            }
        }
        radius /= decf;
        decf *= 2.0;
        if (radius < 1e-32) { status = LO_OTHER; break; }
    }
    if (lane == 0) {
        LoOut o;
        for (int j = 0; j < 4; ++j) o.x[j] = x[j];
        o.cost0 = cost0; o.cost1 = cur[14]; o.iters = it; o.status = status;
        a.out[line] = o;
    }
}

// one wave per 64 lanes of the block; a wave takes one wide line or four narrow ones
__global__ __launch_bounds__(256) void k_lineopt(LoArgs a) {
    const uint32_t wave = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (wave < a.n_wide) {
        lo_solve<64>(a, a.order[wave], lane);
        return;
    }
    const uint32_t k = (wave - a.n_wide) * 4 + lane / 16;
    if (k < a.n_narrow) lo_solve<16>(a, a.order[a.n_wide + k], lane % 16);
}

// test hook: the evaluator on its own, one thread per residual
__global__ __launch_bounds__(256) void k_lineopt_eval(uint32_t n, const double* x, const LoCam* cams, const LoObs* obs,
                                                      double* res, double* jac, double* rho, int32_t* ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double xl[4] = {x[0], x[1], x[2], x[3]};
    Jet4 r[2];
    const bool good = lo_residual(xl, cams[i], obs[i], r);
    double rh = 0.0, rho1;
    lo_huber(r[0].a * r[0].a + r[1].a * r[1].a, rh, rho1);
    for (int k = 0; k < 2; ++k) {
        res[2 * i + k] = r[k].a;
        for (int j = 0; j < 4; ++j) jac[8 * i + 4 * k + j] = r[k].v[j];
    }
    rho[i] = rh;
    ok[i] = good ? 1 : 0;
}

}  // namespace

hipError_t launch_lineopt(const LoArgs& a, hipStream_t st) {
    const uint32_t waves = a.n_wide + (a.n_narrow + 3) / 4;
    if (!waves) return hipSuccess;
    hipLaunchKernelGGL(k_lineopt, dim3((waves + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d

// Test hook: the kernel's own evaluator for line parameters x[4] and n observations, obs [n x 6] = (p1x, p1y, p2x, p2y,
// nx, ny), cams [n x 16] = (R row-major, C, fx, fy, px, py).  residuals [2n], jacobians [8n] (2x4 row-major per
// residual, d r / d (omega, sx, sy, sz), before the loss), ok [n] (0: the evaluation failed, residual 0), *cost =
// 1/2 sum rho(|r_i|^2).
extern "C" int l3d_line_opt_eval(int device, uint32_t n, const double x[4], const double* obs, const double* cams,
                                 double* cost, double* residuals, double* jacobians, int32_t* ok) {
    if (!x || !obs || !cams || !cost || !residuals || !jacobians || !ok || !n) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = set_device(device)) return rc;
    std::vector<LoCam> hc(n);
    std::vector<LoObs> ho(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double* c = cams + 16 * (size_t)i;
        for (int k = 0; k < 9; ++k) hc[i].R[k] = c[k];
        for (int k = 0; k < 3; ++k) hc[i].C[k] = c[9 + k];
        hc[i].fx = c[12]; hc[i].fy = c[13]; hc[i].px = c[14]; hc[i].py = c[15];
        const double* o = obs + 6 * (size_t)i;
        ho[i] = LoObs{o[0], o[1], o[2], o[3], o[4], o[5], i, 0};
    }
    const size_t b_c = n * sizeof(LoCam), b_o = n * sizeof(LoObs), b_r = 2 * (size_t)n * 8, b_j = 8 * (size_t)n * 8, b_h = (size_t)n * 8;
    DevBuf<char> buf;
    L3D_HIP_CHECK(buf.reserve(32 + b_c + b_o + b_r + b_j + b_h + 4 * (size_t)n));
    char* d = buf.p;
    double* dx = (double*)d;
    LoCam* dc = (LoCam*)(d + 32);
    LoObs* dob = (LoObs*)(d + 32 + b_c);
    double* dr = (double*)(d + 32 + b_c + b_o);
    double* dj = (double*)(d + 32 + b_c + b_o + b_r);
    double* dh = (double*)(d + 32 + b_c + b_o + b_r + b_j);
    int32_t* dk = (int32_t*)(d + 32 + b_c + b_o + b_r + b_j + b_h);
    std::vector<double> rho(n);
    hipError_t e = hipMemcpy(dx, x, 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dc, hc.data(), b_c, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dob, ho.data(), b_o, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_lineopt_eval, dim3((n + 255) / 256), dim3(256), 0, 0, n, dx, dc, dob, dr, dj, dh, dk);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(residuals, dr, b_r, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(jacobians, dj, b_j, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rho.data(), dh, b_h, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ok, dk, 4 * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("l3d_line_opt_eval: ") + hipGetErrorString(e));
    double s = 0.0;
    for (uint32_t i = 0; i < n; ++i) s += rho[i];
    *cost = 0.5 * s;
    return L3D_OK;
}
