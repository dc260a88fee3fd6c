// l3d_lineopt.h -- line bundling (Line3D::optimizeClusters -> LineOptimizer::optimize, optimization.cc:8-303), shared
// by the host stage (l3d_lineopt.hip) and the kernel (k_lineopt.hip).
//
// The problem is the reference's: every camera and every intrinsic block is held constant (optimization.cc:172-182)
// and each residual block touches exactly one line's 4 Cayley parameters (:163-165), so the global robust least-squares
// problem splits into one independent 4-parameter problem per 3D line.  Each is solved by its own Levenberg-Marquardt
// iteration on the device (k_lineopt.hip), with the reference solver's defaults where they carry over.  The reference
// runs ONE trust region and ONE stopping test for the whole problem, so per-line iterates and stopping points do not
// match a run of the reference bit for bit: the contract is the cost function below and a per-line local optimum of it.
//
// Residual of one 2D segment (LineReprojectionError, optimization.h): the Plücker line (l, m) rebuilt from
// x = (omega, s), moved into the camera (m - C x l, then rotated), projected with cof(K) to an image line; the signed
// distances of the segment's two end points to that line, weighted by aw = exp(2 * angle) where angle is the angle
// between the image line's normal and the segment's normal, folded to <= pi/2.  The rotation uses R directly: the
// reference goes through RotationMatrixToAngleAxis / AngleAxisRotatePoint, which differs from R * m at rounding level.
// Cost: 1/2 sum rho(|r_i|^2), rho = Huber(2): s for s <= 4, 4 sqrt(s) - 4 beyond (HuberLoss(2.0) in ScaledLoss(1.0)).
//
// Derivative of the angle weight where acos has none: at |dotp| >= 1 the weight is 1 and its derivative is taken as 0
// (angle = 0 is the minimum of the folded angle; the reference's autodiff gives an infinite or NaN derivative there).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace l3d {

struct LoCam {      // one view in the translated frame: R (row-major), C, and the entries of K
    double R[9];
    double C[3];
    double fx, fy, px, py;
};
struct LoObs {      // one residual 2D segment: float end points promoted to double, normal of its direction, its view
    double p1x, p1y, p2x, p2y, nx, ny;
    uint32_t cam, pad;
};
struct LoOut {      // per line: final parameters, robust cost before / after, iterations, stopping rule
    double x[4];
    double cost0, cost1;
    uint32_t iters, status;
};
// stopping rules (LoOut::status)
enum { LO_NONE = 0, LO_GRADIENT = 1, LO_FUNCTION = 2, LO_PARAMETER = 3, LO_MAX_ITER = 4, LO_OTHER = 5 };
constexpr uint32_t kLoNarrow = 16;     // lines with at most this many residuals go to 16-lane groups (4 per wave)

// forward-mode derivative in the 4 line parameters
struct Jet4 {
    double a, v[4];
};
__host__ __device__ inline Jet4 jc(double a) { return Jet4{a, {0, 0, 0, 0}}; }
__host__ __device__ inline Jet4 operator+(const Jet4& x, const Jet4& y) { return Jet4{x.a + y.a, {x.v[0] + y.v[0], x.v[1] + y.v[1], x.v[2] + y.v[2], x.v[3] + y.v[3]}}; }
__host__ __device__ inline Jet4 operator-(const Jet4& x, const Jet4& y) { return Jet4{x.a - y.a, {x.v[0] - y.v[0], x.v[1] - y.v[1], x.v[2] - y.v[2], x.v[3] - y.v[3]}}; }
__host__ __device__ inline Jet4 operator-(const Jet4& x) { return Jet4{-x.a, {-x.v[0], -x.v[1], -x.v[2], -x.v[3]}}; }
__host__ __device__ inline Jet4 operator*(const Jet4& x, const Jet4& y) {
    return Jet4{x.a * y.a, {x.a * y.v[0] + x.v[0] * y.a, x.a * y.v[1] + x.v[1] * y.a, x.a * y.v[2] + x.v[2] * y.a, x.a * y.v[3] + x.v[3] * y.a}};
}
__host__ __device__ inline Jet4 operator*(double s, const Jet4& x) { return Jet4{s * x.a, {s * x.v[0], s * x.v[1], s * x.v[2], s * x.v[3]}}; }
__host__ __device__ inline Jet4 operator/(const Jet4& x, const Jet4& y) {
    const double q = x.a / y.a, iy = 1.0 / y.a;
    return Jet4{q, {(x.v[0] - q * y.v[0]) * iy, (x.v[1] - q * y.v[1]) * iy, (x.v[2] - q * y.v[2]) * iy, (x.v[3] - q * y.v[3]) * iy}};
}
__host__ __device__ inline Jet4 jsqrt(const Jet4& x) {
    const double r = sqrt(x.a), h = 0.5 / r;
    return Jet4{r, {h * x.v[0], h * x.v[1], h * x.v[2], h * x.v[3]}};
}
__host__ __device__ inline Jet4 jexp(const Jet4& x) {
    const double e = exp(x.a);
    return Jet4{e, {e * x.v[0], e * x.v[1], e * x.v[2], e * x.v[3]}};
}

// LineReprojectionError::operator() for one residual: false = the evaluation fails (r = 0)
__host__ __device__ inline bool lo_residual(const double x[4], const LoCam& cam, const LoObs& o, Jet4 r[2]) {
    const Jet4 omega{x[0], {1, 0, 0, 0}}, sx{x[1], {0, 1, 0, 0}}, sy{x[2], {0, 0, 1, 0}}, sz{x[3], {0, 0, 0, 1}};
    const Jet4 nm = (sx * sx + sy * sy) + sz * sz;
    const Jet4 div = jc(1.0) / (jc(1.0) + nm);
    Jet4 l[3], m[3];
    l[0] = div * ((jc(1.0) - nm) + 2.0 * (sx * sx));
    l[1] = div * (2.0 * sz + 2.0 * (sy * sx));
    l[2] = div * (-2.0 * sy + 2.0 * (sz * sx));
    m[0] = (omega * div) * (-2.0 * sz + 2.0 * (sx * sy));
    m[1] = (omega * div) * ((jc(1.0) - nm) + 2.0 * (sy * sy));
    m[2] = (omega * div) * (2.0 * sx + 2.0 * (sz * sy));
    r[0] = jc(0.0); r[1] = jc(0.0);
    if (fabs(x[0]) < 1e-12) return false;
    // m - C x l
    m[0] = m[0] - (cam.C[1] * l[2] - cam.C[2] * l[1]);
    m[1] = m[1] + (cam.C[0] * l[2] - cam.C[2] * l[0]);
    m[2] = m[2] - (cam.C[0] * l[1] - cam.C[1] * l[0]);
    Jet4 q[3];
    for (int i = 0; i < 3; ++i) q[i] = (cam.R[3 * i] * m[0] + cam.R[3 * i + 1] * m[1]) + cam.R[3 * i + 2] * m[2];
    const Jet4 pl0 = cam.fy * q[0], pl1 = cam.fx * q[1];
    const Jet4 pl2 = ((-cam.fy * cam.px) * q[0] - (cam.fx * cam.py) * q[1]) + (cam.fx * cam.fy) * q[2];
    const Jet4 d = jsqrt(pl0 * pl0 + pl1 * pl1);
    if (d.a < 1e-12) return false;
    Jet4 aw = jc(1.0);
    const Jet4 dotp = (pl0 / d) * jc(o.nx) + (pl1 / d) * jc(o.ny);
    if (fabs(dotp.a) < 1.0) {
        double angle = acos(dotp.a);
        double dang = -1.0 / sqrt(1.0 - dotp.a * dotp.a);
        if (angle > 1.5707963267948966) { angle = 3.141592653589793 - angle; dang = -dang; }
        Jet4 a{angle, {dang * dotp.v[0], dang * dotp.v[1], dang * dotp.v[2], dang * dotp.v[3]}};
        aw = jexp(2.0 * a);
    }   // |dotp| == 1: angle 0 (or pi, folded to 0), weight 1, derivative 0; |dotp| > 1 or NaN: acos fails, weight 1
    r[0] = (((pl0 * jc(o.p1x) + pl1 * jc(o.p1y)) + pl2) / d) * aw;
    r[1] = (((pl0 * jc(o.p2x) + pl1 * jc(o.p2y)) + pl2) / d) * aw;
    return true;
}

// Huber(2) of s = |r|^2: rho, rho' ; rho'' is 0 inside and negative outside
__host__ __device__ inline void lo_huber(double s, double& rho, double& rho1) {
    if (s > 4.0) { const double r = sqrt(s); rho = 4.0 * r - 4.0; rho1 = 2.0 / r; }
    else { rho = s; rho1 = 1.0; }
}

// launcher (k_lineopt.hip): one launch solves every line of `order` (n_wide one-wave lines first, then n_narrow lines
// in 16-lane groups; both longest first)
struct LoArgs {
    const LoCam* cams;
    const LoObs* obs;
    const double* x0;          // [4 * lines]
    const uint32_t* res_off;   // [lines + 1]
    const uint32_t* order;     // [n_wide + n_narrow] line indices
    uint32_t n_wide, n_narrow, max_iter;
    LoOut* out;                // [lines]
};
hipError_t launch_lineopt(const LoArgs& a, hipStream_t st);

}  // namespace l3d
