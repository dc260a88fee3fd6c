// l3d_triangulate.hip -- host side of what the Pix4D, OpenMVG and mavmap front ends need beyond the readers:
//   l3d_triangulate_points: main_pix4d.cpp's triangulation of every tie point (linearHomTriangulation, :34-69, loop
//   :354-372) in one launch of k_triangulate (k_triangulate.hip): one packed upload, one launch, one download;
//   the static members of Line3D those mains and callers with projection matrices rely on: rotationFromRPY
//   (line3D.cc:2714-2727), rotationFromQ (:2730-2754), decomposeProjectionMatrix (:2784-2853).  Host arithmetic.
#include "l3d_ctx.h"

#include <cmath>

using namespace l3d;

namespace {
size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

// Eigen::AngleAxisd(angle, unit axis k).toRotationMatrix(): the diagonal entry of the axis is (1 - c) * 1 * 1 + c, the
// two others 0 + c, the off-diagonal pair 0 -+ s
M3 axis_rotation(int k, double angle) {
    const double s = std::sin(angle), c = std::cos(angle);
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    M3 R{{0, 0, 0, 0, 0, 0, 0, 0, 0}};
    R.m[4 * k] = (1.0 - c) + c;
    R.m[4 * i] = c; R.m[4 * j] = c;
    R.m[3 * i + j] = -s; R.m[3 * j + i] = s;
    return R;
}
}  // namespace

extern "C" {

int l3d_triangulate_points(int device, uint32_t n_cameras, const double* P12, uint64_t n_points, const uint64_t* obs_offsets,
                           const uint32_t* obs_camera, const double* obs_xy, double* X3, uint8_t* valid) {
    if (!n_points) return L3D_OK;
    if (!obs_offsets || !X3 || !valid) return fail(L3D_ERR_ARG, "null argument");
    if (obs_offsets[0] != 0) return fail(L3D_ERR_ARG, "obs_offsets[0] is not 0");
    for (uint64_t i = 0; i < n_points; ++i)
        if (obs_offsets[i + 1] < obs_offsets[i]) return fail(L3D_ERR_ARG, "obs_offsets decrease");
    const uint64_t n_obs = obs_offsets[n_points];
    if (n_obs && (!obs_camera || !obs_xy || !P12)) return fail(L3D_ERR_ARG, "null argument");
    for (uint64_t o = 0; o < n_obs; ++o)
        if (obs_camera[o] >= n_cameras) return fail(L3D_ERR_ARG, "observation of a camera >= n_cameras");
    if (n_points >= (1ull << 32) || n_obs >= (1ull << 32)) return fail(L3D_ERR_LIMIT, "more than 2^32 points or observations");
    if (int rc = set_device(device)) return rc;
    // one packed upload: projection matrices | CSR | cameras | pixels; then the results: positions | flags
    const size_t b_P = 96 * (size_t)n_cameras, b_off = 8 * ((size_t)n_points + 1), b_cam = 4 * (size_t)n_obs, b_xy = 16 * (size_t)n_obs;
    const size_t o_P = 0, o_off = up64(o_P + b_P), o_cam = up64(o_off + b_off), o_xy = up64(o_cam + b_cam);
    const size_t in_bytes = o_xy + b_xy, o_X = up64(in_bytes), o_val = o_X + 24 * (size_t)n_points;
    const size_t total = o_val + (size_t)n_points;
    PinnedBuf<char> hb; DevBuf<char> db;
    if (hb.reserve(total) != hipSuccess || db.reserve(total) != hipSuccess)
        return fail(L3D_ERR_HIP, "l3d_triangulate_points: allocation failed");
    char* h = hb.p; char* d = db.p;
    if (b_P) std::memcpy(h + o_P, P12, b_P);
    std::memcpy(h + o_off, obs_offsets, b_off);
    if (n_obs) { std::memcpy(h + o_cam, obs_camera, b_cam); std::memcpy(h + o_xy, obs_xy, b_xy); }
    const TriArgs a{(const double*)(d + o_P), n_cameras, n_points, (const uint64_t*)(d + o_off), (const uint32_t*)(d + o_cam),
                    (const double*)(d + o_xy), (double*)(d + o_X), (uint8_t*)(d + o_val)};
    hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, 0);
    if (e == hipSuccess) e = launch_triangulate(a, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_X, d + o_X, total - o_X, hipMemcpyDeviceToHost, 0);
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("l3d_triangulate_points: ") + hipGetErrorString(e));
    std::memcpy(X3, h + o_X, 24 * (size_t)n_points);
    std::memcpy(valid, h + o_val, (size_t)n_points);
    return L3D_OK;
}

int l3d_rotation_from_rpy(double roll, double pitch, double yaw, double R9[9]) {
    if (!R9) return fail(L3D_ERR_ARG, "null argument");
    const M3 R = m3_mul(m3_mul(axis_rotation(2, yaw), axis_rotation(1, pitch)), axis_rotation(0, roll));   // Rz * Ry * Rx
    std::memcpy(R9, R.m, sizeof(R.m));
    return L3D_OK;
}

int l3d_rotation_from_q(double qw, double qx, double qy, double qz, double R9[9]) {
    if (!R9) return fail(L3D_ERR_ARG, "null argument");
    const double n = qw * qw + qx * qx + qy * qy + qz * qz;
    const double s = std::fabs(n) < kEps ? 0.0 : 2.0 / n;
    const double wx = s * qw * qx, wy = s * qw * qy, wz = s * qw * qz;
    const double xx = s * qx * qx, xy = s * qx * qy, xz = s * qx * qz;
    const double yy = s * qy * qy, yz = s * qy * qz, zz = s * qz * qz;
    R9[0] = 1.0 - (yy + zz); R9[1] = xy - wz;         R9[2] = xz + wy;
    R9[3] = xy + wz;         R9[4] = 1.0 - (xx + zz); R9[5] = yz - wx;
    R9[6] = xz - wy;         R9[7] = yz + wx;         R9[8] = 1.0 - (xx + yy);
    return L3D_OK;
}

int l3d_decompose_projection_matrix(const double P12[12], double K9[9], double R9[9], double t3[3]) {
    if (!P12 || !K9 || !R9 || !t3) return fail(L3D_ERR_ARG, "null argument");
    M3 K{{P12[0], P12[1], P12[2], P12[4], P12[5], P12[6], P12[8], P12[9], P12[10]}};
    // RQ decomposition by three Givens rotations (Hartley & Zisserman, as line3D.cc:2797-2833 takes it)
    double h = std::sqrt(K.m[7] * K.m[7] + K.m[8] * K.m[8]);
    double s = K.m[7] / h, c = -K.m[8] / h;
    const M3 Rx{{1, 0, 0, 0, c, -s, 0, s, c}};
    K = m3_mul(K, Rx);
    h = std::sqrt(K.m[6] * K.m[6] + K.m[8] * K.m[8]);
    s = K.m[6] / h; c = -K.m[8] / h;
    const M3 Ry{{c, 0, -s, 0, 1, 0, s, 0, c}};
    K = m3_mul(K, Ry);
    h = std::sqrt(K.m[3] * K.m[3] + K.m[4] * K.m[4]);
    s = K.m[3] / h; c = -K.m[4] / h;
    const M3 Rz{{c, -s, 0, s, c, 0, 0, 0, 1}};
    K = m3_mul(K, Rz);
    M3 Sign{{1, 0, 0, 0, 1, 0, 0, 0, 1}};                         // :2835-2841: signs of the columns
    for (int i = 0; i < 3; ++i)
        if (K.m[4 * i] < 0) Sign.m[4 * i] = -1;
    K = m3_mul(K, Sign);
    const M3 R = m3_t(m3_mul(m3_mul(m3_mul(Rx, Ry), Rz), Sign));
    const M3 Ki = m3_inv(K);
    for (int i = 0; i < 3; ++i) t3[i] = (Ki.m[3 * i] * P12[3] + Ki.m[3 * i + 1] * P12[7]) + Ki.m[3 * i + 2] * P12[11];
    const double f = 1.0 / K.m[8];                                // :2851
    for (int i = 0; i < 9; ++i) { K9[i] = K.m[i] * f; R9[i] = R.m[i]; }
    return L3D_OK;
}

}  // extern "C"
