// k_undistort.hip -- Line3D::undistortImage (line3D.cc:83-109) on the GPU for a batch of images: OpenCV's
// initUndistortRectifyMap with CV_16SC2 maps followed by remap(INTER_LINEAR, BORDER_CONSTANT 0), as DESIGN §12 defines
// them.  k_undistort takes grid.y = image, so a whole batch is one launch.  The map is computed in registers from the
// per-image constants and the column table (both in the batch arena) and never stored: every destination pixel costs
// rounded double + and * only, in the order of §12 (the library builds with -ffp-contract=off), then the 15-bit
// fixed-point bilinear gather.  A thread writes kPix adjacent pixels of the packed image with 4-byte stores.
// k_undistort_model is the same walk for COLMAP's camera models beyond the five coefficients: only the map
// entry differs, chosen by the image's model, which is uniform over a workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "../../include/l3dpp_hip.h"
#include "l3d_lsd.h"

namespace l3d {
namespace {

constexpr uint32_t kPix = 4;             // destination pixels per thread, adjacent in the packed image

// cvRound as x86 cvtsd2si: half to even; NaN or outside int32 -> INT_MIN
__device__ __forceinline__ int cv_round(double t) {
    return (t >= -2147483648.5 && t < 2147483647.5) ? (int)rint(t) : INT_MIN;
}

// one entry of the CV_16SC2 map with its fractions: source pixel (sx, sy), a and b in 1/32 px
struct MapEntry { int sx, sy, a, b; };

__device__ __forceinline__ MapEntry map_entry(const UndImage& I, double xj, double y) {
    const double x = xj * I.w;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = (2 * x) * y;
    const double kr = 1 + ((I.k3 * r2 + I.k2) * r2 + I.k1) * r2;
    const double xd = x * kr + I.p1 * _2xy + I.p2 * (r2 + 2 * x2);
    const double yd = y * kr + I.p1 * (r2 + 2 * y2) + I.p2 * _2xy;
    int iu = INT_MIN, iv = INT_MIN;          // xd or yd not finite: u = v = NaN
    if (isfinite(xd) && isfinite(yd)) {
        iu = cv_round((I.fx * xd + I.cx) * 32);
        iv = cv_round((I.fy * yd + I.cy) * 32);
    }
    return MapEntry{(int16_t)(iu >> 5), (int16_t)(iv >> 5), iu & 31, iv & 31};
}

// the map entry of DESIGN §15: x, y of the output camera, the model's closed-form distortion, u, v of the input camera.
// Every operation is a rounded double in the order written there.  The choices that depend on the pixel (r against
// DBL_EPSILON, r2 against 1e-4) are selects, so a wave does not diverge; the choice of the model is a scalar branch.
__device__ __forceinline__ MapEntry map_entry(const UndModelImage& I, double xj, double y) {
    const double x = xj * I.w;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2;
    double xd, yd;
    if (I.model == L3D_CAM_FULL_OPENCV) {
        const double _2xy = (2 * x) * y;
        const double kr = (1 + ((I.k3 * r2 + I.k2) * r2 + I.k1) * r2) / (1 + ((I.q[2] * r2 + I.q[1]) * r2 + I.q[0]) * r2);
        xd = x * kr + I.p1 * _2xy + I.p2 * (r2 + 2 * x2);
        yd = y * kr + I.p1 * (r2 + 2 * y2) + I.p2 * _2xy;
    } else if (I.model == L3D_CAM_FOV) {
        const double om = I.q[0], om2 = I.q[1], T = I.q[2];
        double s;
        if (om2 < 1e-4) {
            s = (om2 * r2) / 3 - om2 / 12 + 1;
        } else {
            const double r = sqrt(r2);
            const double far = atan(r * (2 * T)) / (r * om);
            const double near = (-2 * T * (4 * r2 * T * T - 3)) / (3 * om);
            s = r2 < 1e-4 ? near : far;
        }
        xd = x * s;
        yd = y * s;
    } else {                                 // OPENCV_FISHEYE, RADIAL_FISHEYE, SIMPLE_RADIAL_FISHEYE
        const double r = sqrt(r2);
        const double th = atan(r), th2 = th * th;
        const double thd = th * (1 + (((I.q[3] * th2 + I.q[2]) * th2 + I.q[1]) * th2 + I.q[0]) * th2);
        const double s = r > DBL_EPSILON ? thd / r : 1.0;
        xd = x * s;
        yd = y * s;
    }
    int iu = INT_MIN, iv = INT_MIN;
    if (isfinite(xd) && isfinite(yd)) {
        iu = cv_round((I.fx * xd + I.cx) * 32);
        iv = cv_round((I.fy * yd + I.cy) * 32);
    }
    return MapEntry{(int16_t)(iu >> 5), (int16_t)(iv >> 5), iu & 31, iv & 31};
}

// remap of one destination pixel: C channels to out[0..C), every channel with the same weights
template <int C>
__device__ __forceinline__ void remap_pixel(const UndImage& I, const MapEntry& m, uint8_t* out) {
    const int W = (int)I.cols, H = (int)I.rows;
    const int w00 = (32 - m.a) * (32 - m.b) * 32, w10 = m.a * (32 - m.b) * 32;
    const int w01 = (32 - m.a) * m.b * 32, w11 = m.a * m.b * 32;
    const long long rs = (long long)W * C;
    if (m.sx >= 0 && m.sx <= W - 2 && m.sy >= 0 && m.sy <= H - 2) {
        const uint8_t* p = I.src + m.sy * rs + (long long)m.sx * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int v = p[c] * w00 + p[C + c] * w10 + p[rs + c] * w01 + p[rs + C + c] * w11;
            out[c] = (uint8_t)min(max((v + 16384) >> 15, 0), 255);
        }
    } else if (m.sx >= W || m.sx < -1 || m.sy >= H || m.sy < -1) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = 0;
    } else {
        // on the border: a neighbour inside the image contributes its pixel, one outside contributes 0
        const bool x0 = m.sx >= 0, x1 = m.sx + 1 < W, y0 = m.sy >= 0, y1 = m.sy + 1 < H;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            int v = 0;
            if (y0 && x0) v += I.src[m.sy * rs + (long long)m.sx * C + c] * w00;
            if (y0 && x1) v += I.src[m.sy * rs + (long long)(m.sx + 1) * C + c] * w10;
            if (y1 && x0) v += I.src[(m.sy + 1) * rs + (long long)m.sx * C + c] * w01;
            if (y1 && x1) v += I.src[(m.sy + 1) * rs + (long long)(m.sx + 1) * C + c] * w11;
            out[c] = (uint8_t)min(max((v + 16384) >> 15, 0), 255);
        }
    }
}

// destination pixels p0 .. p0 + kPix - 1 of the packed image (they may run into the next row)
template <int C, class Rec>
__device__ __forceinline__ void undistort_pixels(const Rec& I, uint32_t p0) {
    const uint32_t n_pix = I.cols * I.rows, n = min(kPix, n_pix - p0);
    uint32_t i = p0 / I.cols, j = p0 - i * I.cols;
    double y = ((double)i * I.ir4 + I.ir5) * I.w;
    uint8_t px[kPix * C];
#pragma unroll
    for (uint32_t k = 0; k < kPix; ++k) {
        if (k < n) {
            remap_pixel<C>(I, map_entry(I, I.xtab[j], y), px + k * C);
            if (++j == I.cols) {
                j = 0;
                ++i;
                y = ((double)i * I.ir4 + I.ir5) * I.w;
            }
        }
    }
    uint8_t* d = I.dst + (size_t)p0 * C;     // 4-byte aligned when kPix is: the arena's blocks are of 256
    if (kPix % 4 == 0 && n == kPix) {
#pragma unroll
        for (uint32_t q = 0; q < kPix * C / 4; ++q)
            ((uint32_t*)d)[q] = (uint32_t)px[4 * q] | ((uint32_t)px[4 * q + 1] << 8) | ((uint32_t)px[4 * q + 2] << 16) |
                                ((uint32_t)px[4 * q + 3] << 24);
    } else {
        for (uint32_t k = 0; k < n * C; ++k) d[k] = px[k];
    }
}

__global__ __launch_bounds__(256) void k_undistort(const UndImage* imgs) {
    const UndImage& I = imgs[blockIdx.y];
    const uint32_t p0 = (blockIdx.x * blockDim.x + threadIdx.x) * kPix;
    if (p0 >= I.cols * I.rows) return;
    if (I.channels == 3) undistort_pixels<3>(I, p0);
    else undistort_pixels<1>(I, p0);
}

__global__ __launch_bounds__(256) void k_undistort_model(const UndModelImage* imgs) {
    const UndModelImage& I = imgs[blockIdx.y];
    const uint32_t p0 = (blockIdx.x * blockDim.x + threadIdx.x) * kPix;
    if (p0 >= I.cols * I.rows) return;
    if (I.channels == 3) undistort_pixels<3>(I, p0);
    else undistort_pixels<1>(I, p0);
}

}  // namespace

hipError_t launch_undistort(const UndImage* d_imgs, uint32_t n, uint32_t max_pix, hipStream_t st) {
    const uint32_t T = 256, per_block = T * kPix;
    for (uint32_t first = 0; first < n; first += 65535) {       // grid.y is at most 65535
        const uint32_t m = std::min<uint32_t>(n - first, 65535);
        hipLaunchKernelGGL(k_undistort, dim3((max_pix + per_block - 1) / per_block, m), dim3(T), 0, st, d_imgs + first);
    }
    return hipGetLastError();
}

hipError_t launch_undistort_model(const UndModelImage* d_imgs, uint32_t n, uint32_t max_pix, hipStream_t st) {
    const uint32_t T = 256, per_block = T * kPix;
    for (uint32_t first = 0; first < n; first += 65535) {
        const uint32_t m = std::min<uint32_t>(n - first, 65535);
        hipLaunchKernelGGL(k_undistort_model, dim3((max_pix + per_block - 1) / per_block, m), dim3(T), 0, st, d_imgs + first);
    }
    return hipGetLastError();
}

}  // namespace l3d
