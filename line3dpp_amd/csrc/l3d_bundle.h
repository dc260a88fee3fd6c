// l3d_bundle.h -- cameras and 3D lines bundled jointly, shared by the host stage (l3d_bundle.hip) and the
// kernels (k_bundle.hip): the layout of a cell's sums, the basis of a line's four parameters and the image line of a
// carrier in a camera, each as one function for the device and the host, and the kernels' arguments.  fp64 in the order
// §29 writes it.
#pragma once
#include "l3d_refit.h"

namespace l3d {

constexpr uint32_t kBundleBlock = 256;
// a cell's sums: w J_c J_c^T (21, upper triangle row by row), w J_c r (6), w J_c J_l^T (24: [camera column][line column]),
// w J_l J_l^T (10), w J_l r (4), rho and the count
constexpr uint32_t kBcCC = 0, kBcBC = 21, kBcCL = 27, kBcLL = 51, kBcBL = 61, kBcRho = 65, kBcCount = 66, kBundleCell = 67;
constexpr uint32_t kBundleMaxFree = 512;         // free cameras of a call: the reduced system is dense
// a line's factor of a step: L (lower triangle row by row: L00, L10, L11, L20 ..) of H_ll + mu diag H_ll, and v = L^-1 b_l
struct BundleFactor { double L[10], v[4]; };
static_assert(sizeof(BundleFactor) == 112 && sizeof(PoseCam) == 136, "bundle record layout");

// the last k in [0, n) with table[k] <= v (table ascending, table[0] <= v)
__host__ __device__ inline uint32_t bundle_last_not_above(const uint32_t* table, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (table[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// The basis of a carrier AB = (A, B): u = B - A, k the index of the smallest |u_k| (the first on ties),
// e1 = (u x e_k) / |u x e_k|, e2 = (u x e1) / |u x e1|
__host__ __device__ inline void bundle_basis(const double* AB, double e1[3], double e2[3]) {
    const double u[3] = {AB[3] - AB[0], AB[4] - AB[1], AB[5] - AB[2]};
    int k = 0;
    if (fabs(u[1]) < fabs(u[k])) k = 1;
    if (fabs(u[2]) < fabs(u[k])) k = 2;
    const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    const double c[3] = {u[1] * ek[2] - u[2] * ek[1], u[2] * ek[0] - u[0] * ek[2], u[0] * ek[1] - u[1] * ek[0]};
    const double n1 = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    for (int i = 0; i < 3; ++i) e1[i] = c[i] / n1;
    const double f[3] = {u[1] * e1[2] - u[2] * e1[1], u[2] * e1[0] - u[0] * e1[2], u[0] * e1[1] - u[1] * e1[0]};
    const double n2 = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    for (int i = 0; i < 3; ++i) e2[i] = f[i] / n2;
}

// K^-T v for an upper-triangular K with K22 = 1: M = (m00, m10, m11, m20, m21) (§27's)
__host__ __device__ inline void bundle_kt(const double* M, const double* v, double* l) {
    l[0] = M[0] * v[0];
    l[1] = M[1] * v[0] + M[2] * v[1];
    l[2] = (M[3] * v[0] + M[4] * v[1]) + v[2];
}

// The image line lam = K^-T (Y1 x Y2) of the carrier in the camera and its norm nu = sqrt(lam0^2 + lam1^2);
// false: nu is not finite and > 0 (the observation takes no part)
__host__ __device__ inline bool bundle_image_line(const PoseCam& pc, const double* AB, d3& Y1, d3& Y2, double lam[3], double& nu) {
    const d3 t{pc.t[0], pc.t[1], pc.t[2]};
    Y1 = mul33(pc.R, d3{AB[0], AB[1], AB[2]}) + t;
    Y2 = mul33(pc.R, d3{AB[3], AB[4], AB[5]}) + t;
    const d3 Nc = cross(Y1, Y2);
    const double N[3] = {Nc.x, Nc.y, Nc.z};
    bundle_kt(pc.M, N, lam);
    nu = sqrt(lam[0] * lam[0] + lam[1] * lam[1]);
    return nu > 0.0 && fabs(nu) <= 1.7976931348623157e308;
}

// rho(s) of one observation at a camera and a carrier: s = r_P^2 + r_Q^2 under lo_huber; +0.0 where it takes no part
__host__ __device__ inline double bundle_rho(const PoseCam& pc, const double* AB, const LoObs& o) {
    d3 Y1, Y2;
    double lam[3], nu;
    if (!bundle_image_line(pc, AB, Y1, Y2, lam, nu)) return 0.0;
    const double rp = ((lam[0] * o.p1x + lam[1] * o.p1y) + lam[2]) / nu;
    const double rq = ((lam[0] * o.p2x + lam[1] * o.p2y) + lam[2]) / nu;
    double rho, w;
    lo_huber(rp * rp + rq * rq, rho, w);
    return rho;
}

// the kernels' tables (k_bundle.hip); every index is the call's own (cameras and lines as given)
struct BundleArgs {
    uint32_t n_cams, n_lines, n_obs, n_cells, n_eligible, n_free;
    const PoseCam* cams;           // [n_cams] the poses the launch works in, about the model's centre
    const PoseCam* cams_trial;     // [n_cams] k_bundle_cost's
    const LoObs* obs;              // [n_obs] line after line (k_refit_obs)
    const uint32_t* obs_off;       // [n_lines + 1]
    const uint32_t* cell_off;      // [n_cells + 1] a cell's observations
    const uint32_t* cell_line;     // [n_cells]
    const uint32_t* cell_cam;      // [n_cells]
    const uint32_t* line_cell_off; // [n_lines + 1] a line's cells
    const uint32_t* eligible;      // [n_eligible] the eligible lines, ascending
    const uint32_t* is_eligible;   // [n_lines]
    const uint32_t* cam_cell_off;  // [n_cams + 1] the second CSR: a camera's cells, in ascending line
    const uint32_t* cam_cells;     // [n_cells]
    const int32_t* slot;           // [n_lines x n_cams] the cell of (line, camera); -1: none
    const uint32_t* free_cam;      // [n_free] the free cameras with a cell, ascending
    const int32_t* cam_free;       // [n_cams] a camera's place among them; -1: fixed, or without a cell
    const double* AB;              // [n_lines x 6] the carriers in force, about the model's centre
    double* AB_trial;              // [n_lines x 6] k_bundle_update
    double mu;
    double* cells;                 // [n_cells x kBundleCell] k_bundle_cells
    uint32_t* line_ok;             // [n_lines] k_bundle_lines: 1 where the line's factor stands (0 for every held line)
    BundleFactor* factor;          // [n_lines] k_bundle_lines
    double* W;                     // [n_cells x 24] k_bundle_lines: L^-1 H_cl^T as [camera column][row]
    double* blocks;                // [n_free x n_free x 36] k_bundle_reduce: the block of the pair (a <= b)
    double* rhs;                   // [n_free x 6] k_bundle_reduce
    const double* delta_c;         // [n_free x 6] the cameras' step
    double* delta_l;               // [n_lines x 4] k_bundle_update: the lines' step (0 where the line is held)
    double* tiles;                 // [ceil(n_obs / 256)] k_bundle_cost
};
hipError_t launch_bundle_cells(const BundleArgs& a, hipStream_t st);
hipError_t launch_bundle_lines(const BundleArgs& a, hipStream_t st);
hipError_t launch_bundle_reduce(const BundleArgs& a, hipStream_t st);
hipError_t launch_bundle_update(const BundleArgs& a, hipStream_t st);
hipError_t launch_bundle_cost(const BundleArgs& a, hipStream_t st);   // at cams_trial and AB_trial

}  // namespace l3d
