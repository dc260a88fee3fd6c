// l3d_lsd.h -- line-segment detection (Line3D::detectLineSegments, line3D.cc:243-370, with the LSD of
// lsd/lsd_opencv.cpp in its LSD_REFINE_ADV form).  Shared by k_lsd.hip (kernels) and l3d_lsd.hip (host).
// DESIGN §11 states the contract and the definitions chosen for fastAtan2, the blur and the resamples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

namespace l3d {

constexpr float kLsdNotDef = -1024.0f;    // NOTDEF of lsd_opencv.cpp, on the float degree map
constexpr double kLsdScale = 0.8;         // SCALE
constexpr double kLsdLogEps = 0.0;        // LOG_EPS
constexpr double kLsdDensityTh = 0.7;     // DENSITY_TH
constexpr int kLsdTaps = 7;               // GaussianBlur ksize: 1 + 2 ceil(0.75 sqrt(6 ln 10))

// one image of a detection batch; every pointer is device memory inside the batch's arena
struct LsdImage {
    const uint8_t* src;            // input pixels, rows x (cols * channels), packed
    uint32_t cols, rows, channels;
    uint32_t gw, gh;               // grey image handed to LSD (after the max-width downscale)
    uint32_t sw, sh;               // after the 0.8 resample
    uint32_t down;                 // 1: the 8U downscale runs (gw x gh from cols x rows)
    double down_scale;             // 1 / s of the downscale (s = max_image_width / max_dim, float)
    uint8_t* gray;                 // cols x rows
    uint8_t* small;                // gw x gh (== gray without the downscale)
    double* tmp;                   // gw x gh, the row pass of the blur
    double* blur;                  // gw x gh
    float* deg;                    // sw x sh: fastAtan2 degrees, kLsdNotDef where the gradient is undefined
    double* mod;                   // sw x sh: gradient norm
    uint8_t* used;                 // sw x sh
    int2* reg;                     // sw x sh region points
    float4* out;                   // raw LSD segments in detection order, (x1, y1, x2, y2) of the full LSD input
    uint32_t out_cap;
    double log_nt;                 // LOG_NT of the walk (host libm)
    int min_reg_size;
};

// per-image results of the device stages
struct LsdResult {
    uint32_t n;                    // raw segments found (may exceed out_cap: then `overflow`)
    uint32_t overflow;
    unsigned long long max_grad_bits;   // ll_angle's max_grad as the bits of a non-negative double (0: none defined)
    uint32_t seeds;                // regions grown from a seed
    uint32_t nfa_evals;            // rect_nfa evaluations
};

struct LsdConst {
    double gauss[kLsdTaps];        // getGaussianKernel(7, 0.6 / 0.8) in double
    double rho;                    // gradient threshold QUANT / sin(prec)
    double prec, p;                // pi * ANG_TH / 180, ANG_TH / 180
};

extern std::atomic<uint64_t> g_lsd_images_detected;   // l3d_lsd.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_lsd_cache_loads;

hipError_t launch_lsd(const LsdImage* d_imgs, uint32_t n, uint32_t max_src_pix, uint32_t max_small_pix,
                      uint32_t max_scaled_pix, const LsdConst& k, LsdResult* d_res, hipStream_t st);

// one image of an undistortion batch (Line3D::undistortImage); every pointer is device memory inside the
// batch's arena.  The per-image constants are the host's, in double: k_undistort.hip computes the map from them.
struct UndImage {
    const uint8_t* src;            // rows x (cols * channels), packed
    uint8_t* dst;                  // the same shape
    const double* xtab;            // column table X[0..cols): X[0] = ir2, X[j+1] = X[j] + ir0
    uint32_t cols, rows, channels;
    double w;                      // 1 / ir8
    double ir4, ir5;               // row value Y[i] = i * ir4 + ir5
    double fx, fy, cx, cy;
    double k1, k2, k3, p1, p2;
};

hipError_t launch_undistort(const UndImage* d_imgs, uint32_t n, uint32_t max_pix, hipStream_t st);

// one image of an undistortion batch by camera model.  The UndImage part: w, ir4, ir5 and xtab are of the
// OUTPUT image's camera matrix, fx, fy, cx, cy of the input's; k1, k2, k3, p1, p2 are FULL_OPENCV's.  model is an
// L3D_CAM_* value, the same for a whole workgroup (grid.y = image).
struct UndModelImage : UndImage {
    uint32_t model;
    double q[4];                   // FULL_OPENCV: k4 k5 k6; the fisheye family: k1 k2 k3 k4; FOV: omega, omega^2, tan(omega / 2)
};

hipError_t launch_undistort_model(const UndModelImage* d_imgs, uint32_t n, uint32_t max_pix, hipStream_t st);

}  // namespace l3d
