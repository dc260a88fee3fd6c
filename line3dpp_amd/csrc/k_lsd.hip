// k_lsd.hip -- line-segment detection on the GPU: the LSD of the reference's lsd/lsd_opencv.cpp (LSD_REFINE_ADV) with
// the grey conversion and max-width downscale of Line3D::detectLineSegments (line3D.cc:243-310), for a batch of images.
//
// Per-pixel stages (grid.y = image; every image of the batch in the same launch):
//   k_lsd_gray     CV_RGB2GRAY on 8U (first channel = R) or a copy of a grey image
//   k_lsd_down     INTER_LINEAR on 8U, fixed point (only images wider than max_image_width)
//   k_lsd_blur_h   row pass of the 7-tap fp64 Gaussian, BORDER_REFLECT_101, taps summed left to right
//   k_lsd_blur_v   column pass, symmetric form: centre tap, then k[j] * (S[+j] + S[-j])
//   k_lsd_grad     the 0.8 INTER_LINEAR resample of the four pixels a gradient needs, fused with ll_angle: norm,
//                  fastAtan2 angle, NOTDEF, max_grad; clears the `used` map
// The walk (k_lsd_walk, one wave per image): flsd's seed loop in raster order.  A wave ballots 64 pixels at a time for
// the first eligible seed (not used, angle defined), lane 0 grows the region and runs region2rect / refine /
// reduce_region_radius (sequential by definition: region_grow updates the running angle after every pixel), and
// rect_improve runs on the whole wave with rect_nfa's aligned-point count split across the lanes (integers: exact).
// Every double sum keeps the reference's order.  DESIGN §11.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "l3d_lsd.h"

namespace l3d {
namespace {

constexpr double kPi = 3.1415926535897932384626433832795;   // CV_PI
constexpr double kDegToRads = kPi / 180;
constexpr double kNotDef = -1024.0;

// OpenCV's fastAtan2: float polynomial in degrees (DESIGN §11 states the definition chosen)
__device__ __forceinline__ float fast_atan2(float y, float x) {
    const float r2d = (float)(180.0 / kPi);
    const float p1 = 0.9997878412794807f * r2d, p3 = -0.3258083974640975f * r2d;
    const float p5 = 0.1555786518463281f * r2d, p7 = -0.04432655554792128f * r2d;
    const float ax = fabsf(x), ay = fabsf(y);
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + (float)DBL_EPSILON), c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        const float c = ax / (ay + (float)DBL_EPSILON), c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// INTER_LINEAR source index and float weight of destination index d (scale = 1 / inv_scale, double)
__device__ __forceinline__ void resize_map(int d, int n_src, double scale, int& s, float& f) {
    f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
}

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

__global__ void k_lsd_gray(const LsdImage* imgs) {
    const LsdImage& I = imgs[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.cols * I.rows) return;
    if (I.channels == 3) {
        const uint8_t* p = I.src + 3 * (size_t)i;
        I.gray[i] = (uint8_t)(((int)p[0] * 4899 + (int)p[1] * 9617 + (int)p[2] * 1868 + 8192) >> 14);
    } else {
        I.gray[i] = I.src[i];
    }
}

__global__ void k_lsd_down(const LsdImage* imgs) {
    const LsdImage& I = imgs[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!I.down || i >= I.gw * I.gh) return;
    const int x = i % I.gw, y = i / I.gw, W = I.cols, H = I.rows;
    int sx, sy;
    float fx, fy;
    resize_map(x, W, I.down_scale, sx, fx);
    resize_map(y, H, I.down_scale, sy, fy);
    const int a0 = (int)rintf((1.f - fx) * 2048.f), a1 = (int)rintf(fx * 2048.f);
    const int b0 = (int)rintf((1.f - fy) * 2048.f), b1 = (int)rintf(fy * 2048.f);
    const int sx1 = min(sx + 1, W - 1), sy1 = min(sy + 1, H - 1);
    const uint8_t* r0 = I.gray + (size_t)sy * W;
    const uint8_t* r1 = I.gray + (size_t)sy1 * W;
    const int h0 = r0[sx] * a0 + r0[sx1] * a1, h1 = r1[sx] * a0 + r1[sx1] * a1;
    const int v = (h0 * b0 + h1 * b1 + (1 << 21)) >> 22;
    I.small[i] = (uint8_t)min(max(v, 0), 255);
}

__global__ void k_lsd_blur_h(const LsdImage* imgs, LsdConst k) {
    const LsdImage& I = imgs[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.gw * I.gh) return;
    const int x = i % I.gw, W = I.gw;
    const uint8_t* row = I.small + (i - x);
    double acc = k.gauss[0] * (double)row[reflect101(x - 3, W)];
#pragma unroll
    for (int t = 1; t < kLsdTaps; ++t) acc = acc + k.gauss[t] * (double)row[reflect101(x + t - 3, W)];
    I.tmp[i] = acc;
}

__global__ void k_lsd_blur_v(const LsdImage* imgs, LsdConst k) {
    const LsdImage& I = imgs[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.gw * I.gh) return;
    const int x = i % I.gw, y = i / I.gw, W = I.gw, H = I.gh;
    // the symmetric column form of OpenCV's separable filter: centre tap, then k[j] * (S[+j] + S[-j]) outwards
    double acc = k.gauss[3] * I.tmp[(size_t)y * W + x];
#pragma unroll
    for (int j = 1; j <= 3; ++j)
        acc = acc + k.gauss[3 + j] * (I.tmp[(size_t)reflect101(y + j, H) * W + x] + I.tmp[(size_t)reflect101(y - j, H) * W + x]);
    I.blur[i] = acc;
}

// one pixel of the 0.8 resample of the blurred image: rows first (float weights in double), then columns
__device__ __forceinline__ double resampled(const LsdImage& I, int x, int y) {
    const double scale = 1.0 / kLsdScale;
    const int W = I.gw, H = I.gh;
    int sx, sy;
    float fx, fy;
    resize_map(x, W, scale, sx, fx);
    resize_map(y, H, scale, sy, fy);
    const int sx1 = min(sx + 1, W - 1), sy1 = min(sy + 1, H - 1);
    const double a0 = (double)(1.f - fx), a1 = (double)fx, b0 = (double)(1.f - fy), b1 = (double)fy;
    const double* r0 = I.blur + (size_t)sy * W;
    const double* r1 = I.blur + (size_t)sy1 * W;
    const double h0 = r0[sx] * a0 + r0[sx1] * a1;
    const double h1 = r1[sx] * a0 + r1[sx1] * a1;
    return h0 * b0 + h1 * b1;
}

__global__ void k_lsd_grad(const LsdImage* imgs, LsdConst k, LsdResult* res) {
    const LsdImage& I = imgs[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.sw * I.sh) return;
    const int x = i % I.sw, y = i / I.sw;
    I.used[i] = 0;
    if (x == (int)I.sw - 1 || y == (int)I.sh - 1) {
        I.deg[i] = kLsdNotDef;
        I.mod[i] = 0.0;
        return;
    }
    const double s00 = resampled(I, x, y), s01 = resampled(I, x + 1, y);
    const double s10 = resampled(I, x, y + 1), s11 = resampled(I, x + 1, y + 1);
    const double DA = s11 - s00, BC = s01 - s10;
    const double gx = DA + BC, gy = DA - BC;
    const double norm = sqrt((gx * gx + gy * gy) / 4);
    I.mod[i] = norm;
    if (norm <= k.rho) {
        I.deg[i] = kLsdNotDef;
    } else {
        I.deg[i] = fast_atan2((float)gx, (float)(-gy));
        atomicMax(&res[blockIdx.y].max_grad_bits, (unsigned long long)__double_as_longlong(norm));
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------
struct Rect {
    double x1, y1, x2, y2, width, x, y, theta, dx, dy, prec, p;
};

__device__ __forceinline__ double angle_at(const float* deg, int a) {
    const float d = deg[a];
    return d == kLsdNotDef ? kNotDef : (double)d * kDegToRads;
}

__device__ __forceinline__ bool is_aligned(const float* deg, int a, double theta, double prec) {
    const double ang = angle_at(deg, a);
    if (ang == kNotDef) return false;
    double t = theta - ang;
    if (t < 0) t = -t;
    if (t > (3 * kPi) / 2) {
        t -= 2 * kPi;
        if (t < 0) t = -t;
    }
    return t <= prec;
}

__device__ __forceinline__ double angle_diff_signed(double a, double b) {
    double d = a - b;
    while (d <= -kPi) d += 2 * kPi;
    while (d > kPi) d -= 2 * kPi;
    return d;
}

__device__ __forceinline__ bool double_equal(double a, double b) {
    if (a == b) return true;
    const double d = fabs(a - b), aa = fabs(a), bb = fabs(b);
    double m = aa > bb ? aa : bb;
    if (m < DBL_MIN) m = DBL_MIN;
    return d / m <= 100.0 * DBL_EPSILON;
}

__device__ __forceinline__ double dist(double x1, double y1, double x2, double y2) {
    return sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1));
}

// lane 0 only: region_grow (the running angle is updated after every added pixel)
__device__ int region_grow(const LsdImage& I, int sx, int sy, double prec, double& reg_angle) {
    const int W = I.sw, H = I.sh;
    const int adr = sx + sy * W;
    I.reg[0] = make_int2(sx, sy);
    int n = 1;
    reg_angle = angle_at(I.deg, adr);
    float sumdx = (float)cos(reg_angle), sumdy = (float)sin(reg_angle);
    I.used[adr] = 1;
    for (int i = 0; i < n; ++i) {
        const int2 q = I.reg[i];
        const int x0 = max(q.x - 1, 0), x1 = min(q.x + 1, W - 1);
        const int y0 = max(q.y - 1, 0), y1 = min(q.y + 1, H - 1);
        for (int yy = y0; yy <= y1; ++yy) {
            for (int xx = x0; xx <= x1; ++xx) {
                const int c = xx + yy * W;
                if (I.used[c] != 1 && is_aligned(I.deg, c, reg_angle, prec)) {
                    I.used[c] = 1;
                    I.reg[n++] = make_int2(xx, yy);
                    const double a = (double)(float)angle_at(I.deg, c);
                    sumdx = (float)((double)sumdx + cos(a));
                    sumdy = (float)((double)sumdy + sin(a));
                    reg_angle = (double)fast_atan2(sumdy, sumdx) * kDegToRads;
                }
            }
        }
    }
    return n;
}

__device__ double get_theta(const LsdImage& I, int n, double x, double y, double reg_angle, double prec) {
    double Ixx = 0.0, Iyy = 0.0, Ixy = 0.0;
    for (int i = 0; i < n; ++i) {
        const int2 q = I.reg[i];
        const double w = I.mod[q.x + q.y * (int)I.sw];
        const double dx = (double)q.x - x, dy = (double)q.y - y;
        Ixx += dy * dy * w;
        Iyy += dx * dx * w;
        Ixy -= dx * dy * w;
    }
    // the reference asserts here (a region of one point cannot reach it: min_reg_size > 1, refine needs 2)
    const double lambda = 0.5 * (Ixx + Iyy - sqrt((Ixx - Iyy) * (Ixx - Iyy) + 4.0 * Ixy * Ixy));
    double theta = fabs(Ixx) > fabs(Iyy) ? (double)fast_atan2((float)(lambda - Ixx), (float)Ixy)
                                         : (double)fast_atan2((float)Ixy, (float)(lambda - Iyy));
    theta *= kDegToRads;
    if (fabs(angle_diff_signed(theta, reg_angle)) > prec) theta += kPi;
    return theta;
}

__device__ void region2rect(const LsdImage& I, int n, double reg_angle, double prec, double p, Rect& r) {
    double x = 0, y = 0, sum = 0;
    for (int i = 0; i < n; ++i) {
        const int2 q = I.reg[i];
        const double w = I.mod[q.x + q.y * (int)I.sw];
        x += (double)q.x * w;
        y += (double)q.y * w;
        sum += w;
    }
    x /= sum;
    y /= sum;
    const double theta = get_theta(I, n, x, y, reg_angle, prec);
    const double dx = cos(theta), dy = sin(theta);
    double l_min = 0, l_max = 0, w_min = 0, w_max = 0;
    for (int i = 0; i < n; ++i) {
        const int2 q = I.reg[i];
        const double rx = (double)q.x - x, ry = (double)q.y - y;
        const double l = rx * dx + ry * dy;
        const double w = -rx * dy + ry * dx;
        if (l > l_max) l_max = l;
        else if (l < l_min) l_min = l;
        if (w > w_max) w_max = w;
        else if (w < w_min) w_min = w;
    }
    r.x1 = x + l_min * dx; r.y1 = y + l_min * dy;
    r.x2 = x + l_max * dx; r.y2 = y + l_max * dy;
    r.width = w_max - w_min;
    r.x = x; r.y = y; r.theta = theta; r.dx = dx; r.dy = dy; r.prec = prec; r.p = p;
    if (r.width < 1.0) r.width = 1.0;
}

__device__ bool reduce_region_radius(const LsdImage& I, int& n, double reg_angle, double prec, double p, Rect& r,
                                     double density) {
    const double xc = (double)I.reg[0].x, yc = (double)I.reg[0].y;
    const double r1 = (r.x1 - xc) * (r.x1 - xc) + (r.y1 - yc) * (r.y1 - yc);
    const double r2 = (r.x2 - xc) * (r.x2 - xc) + (r.y2 - yc) * (r.y2 - yc);
    double rad = r1 > r2 ? r1 : r2;
    while (density < kLsdDensityTh) {
        rad *= 0.75 * 0.75;
        for (int i = 0; i < n; ++i) {
            const int2 q = I.reg[i];
            if (((double)q.x - xc) * ((double)q.x - xc) + ((double)q.y - yc) * ((double)q.y - yc) > rad) {
                I.used[q.x + q.y * (int)I.sw] = 0;
                I.reg[i] = I.reg[n - 1];
                I.reg[n - 1] = q;
                --n;
                --i;
            }
        }
        if (n < 2) return false;
        region2rect(I, n, reg_angle, prec, p, r);
        density = (double)n / (dist(r.x1, r.y1, r.x2, r.y2) * r.width);
    }
    return true;
}

__device__ bool refine(const LsdImage& I, int& n, double reg_angle, double prec, double p, Rect& r) {
    double density = (double)n / (dist(r.x1, r.y1, r.x2, r.y2) * r.width);
    if (density >= kLsdDensityTh) return true;
    const int2 c = I.reg[0];
    const double xc = (double)c.x, yc = (double)c.y;
    const double ang_c = angle_at(I.deg, c.x + c.y * (int)I.sw);
    double sum = 0, s_sum = 0;
    int k = 0;
    for (int i = 0; i < n; ++i) {
        const int2 q = I.reg[i];
        I.used[q.x + q.y * (int)I.sw] = 0;
        if (dist(xc, yc, (double)q.x, (double)q.y) < r.width) {
            const double d = angle_diff_signed(angle_at(I.deg, q.x + q.y * (int)I.sw), ang_c);
            sum += d;
            s_sum += d * d;
            ++k;
        }
    }
    const double mean = sum / (double)k;
    const double tau = 2.0 * sqrt((s_sum - 2.0 * mean * sum) / (double)k + mean * mean);
    n = region_grow(I, c.x, c.y, tau, reg_angle);
    if (n < 2) return false;
    region2rect(I, n, reg_angle, prec, p, r);
    density = (double)n / (dist(r.x1, r.y1, r.x2, r.y2) * r.width);
    if (density < kLsdDensityTh) return reduce_region_radius(I, n, reg_angle, prec, p, r, density);
    return true;
}

__device__ __forceinline__ double log_gamma(double x) {
    if (x > 15.0)
        return 0.918938533204673 + (x - 0.5) * log(x) - x + 0.5 * x * log(x * sinh(1 / x) + 1 / (810.0 * pow(x, 6.0)));
    const double q[7] = {75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424,
                         2.50662827511};
    double a = (x + 0.5) * log(x + 5.5) - (x + 5.5), b = 0;
    for (int n = 0; n < 7; ++n) {
        a -= log(x + (double)n);
        b += q[n] * pow(x, (double)n);
    }
    return a + log(b);
}

__device__ double nfa(int n, int k, double p, double log_nt) {
    if (n == 0 || k == 0) return -log_nt;
    if (n == k) return -log_nt - (double)n * log10(p);
    const double p_term = p / (1 - p);
    const double log1 = ((double)n + 1) - log_gamma((double)k + 1) - log_gamma((double)(n - k) + 1) +
                        (double)k * log(p) + (double)(n - k) * log(1.0 - p);
    double term = exp(log1);
    if (double_equal(term, 0)) return k > n * p ? -log1 / 2.30258509299404568402 - log_nt : -log_nt;
    double tail = term;
    for (int i = k + 1; i <= n; ++i) {
        const double bt = (double)(n - i + 1) / (double)i, mt = bt * p_term;
        term *= mt;
        tail += term;
        if (bt < 1) {
            const double err = term * ((1 - pow(mt, (double)(n - i + 1))) / (1 - mt) - 1);
            if (err < 0.1 * fabs(-log10(tail) - log_nt) * tail) break;
        }
    }
    return -log10(tail) - log_nt;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Corner { int x, y; };

// the whole wave, uniform control flow; the aligned-point count is split across the lanes
__device__ double rect_nfa(const LsdImage& I, const Rect& r, int lane) {
    const double hw = r.width / 2.0, dyhw = r.dy * hw, dxhw = r.dx * hw;
    Corner c[4] = {{(int)(r.x1 - dyhw), (int)(r.y1 + dxhw)}, {(int)(r.x2 - dyhw), (int)(r.y2 + dxhw)},
                   {(int)(r.x2 + dyhw), (int)(r.y2 - dxhw)}, {(int)(r.x1 + dyhw), (int)(r.y1 - dxhw)}};
    // sort by (x, y): points that compare equal are equal, so any sort gives the reference's order
    for (int i = 1; i < 4; ++i)
        for (int j = i; j > 0 && (c[j].x < c[j - 1].x || (c[j].x == c[j - 1].x && c[j].y < c[j - 1].y)); --j) {
            const Corner t = c[j]; c[j] = c[j - 1]; c[j - 1] = t;
        }
    int mn = 0, mx = 0;
    for (int i = 1; i < 4; ++i) {
        if (c[mn].y > c[i].y) mn = i;
        if (c[mx].y < c[i].y) mx = i;
    }
    bool taken[4] = {false, false, false, false};
    taken[mn] = true;
    int lm = -1, rm = -1, tl = -1;
    for (int i = 0; i < 4; ++i) if (!taken[i] && (lm < 0 || c[lm].x > c[i].x)) lm = i;
    taken[lm] = true;
    for (int i = 0; i < 4; ++i) if (!taken[i] && (rm < 0 || c[rm].x < c[i].x)) rm = i;
    taken[rm] = true;
    for (int i = 0; i < 4; ++i) if (!taken[i] && (tl < 0 || c[tl].x > c[i].x)) tl = i;
    const Corner MN = c[mn], LM = c[lm], RM = c[rm], TL = c[tl];
    // integer divisions, and the tail's x where its y belongs, as lsd_opencv.cpp has them
    const double flstep = MN.y != LM.y ? (double)((MN.x - LM.x) / (MN.y - LM.y)) : 0;
    const double slstep = LM.y != TL.x ? (double)((LM.x - TL.x) / (LM.y - TL.x)) : 0;
    const double frstep = MN.y != RM.y ? (double)((MN.x - RM.x) / (MN.y - RM.y)) : 0;
    const double srstep = RM.y != TL.x ? (double)((RM.x - TL.x) / (RM.y - TL.x)) : 0;
    double lstep = flstep, rstep = frstep, lx = MN.x, rx = MN.x;
    const int W = I.sw, H = I.sh;
    int total = 0, alg = 0;
    for (int y = MN.y; y <= c[mx].y; ++y) {
        if (y >= 0 && y < H) {
            const int x0 = max((int)lx, 0), x1 = min((int)rx, W - 1);
            if (x1 >= x0) {
                total += x1 - x0 + 1;
                const int base = y * W;
                for (int x = x0 + lane; x <= x1; x += 64) alg += is_aligned(I.deg, base + x, r.theta, r.prec);
            }
        }
        if (y >= LM.y) lstep = slstep;
        if (y >= RM.y) rstep = srstep;
        lx += lstep;
        rx += rstep;
    }
    return nfa(total, wave_sum(alg), r.p, I.log_nt);
}

__device__ double rect_improve(const LsdImage& I, Rect& rec, int lane, uint32_t& evals) {
    const double delta = 0.5, delta_2 = delta / 2.0;
    double log_nfa = rect_nfa(I, rec, lane);
    ++evals;
    if (log_nfa > kLsdLogEps) return log_nfa;
    Rect r = rec;
    for (int n = 0; n < 5; ++n) {
        r.p /= 2;
        r.prec = r.p * kPi;
        const double v = rect_nfa(I, r, lane); ++evals;
        if (v > log_nfa) { log_nfa = v; rec = r; }
    }
    if (log_nfa > kLsdLogEps) return log_nfa;
    r = rec;
    for (int n = 0; n < 5; ++n) {
        if ((r.width - delta) >= 0.5) {
            r.width -= delta;
            const double v = rect_nfa(I, r, lane); ++evals;
            if (v > log_nfa) { rec = r; log_nfa = v; }
        }
    }
    if (log_nfa > kLsdLogEps) return log_nfa;
    r = rec;
    for (int n = 0; n < 5; ++n) {
        if ((r.width - delta) >= 0.5) {
            r.x1 += -r.dy * delta_2; r.y1 += r.dx * delta_2;
            r.x2 += -r.dy * delta_2; r.y2 += r.dx * delta_2;
            r.width -= delta;
            const double v = rect_nfa(I, r, lane); ++evals;
            if (v > log_nfa) { rec = r; log_nfa = v; }
        }
    }
    if (log_nfa > kLsdLogEps) return log_nfa;
    r = rec;
    for (int n = 0; n < 5; ++n) {
        if ((r.width - delta) >= 0.5) {
            r.x1 -= -r.dy * delta_2; r.y1 -= r.dx * delta_2;
            r.x2 -= -r.dy * delta_2; r.y2 -= r.dx * delta_2;
            r.width -= delta;
            const double v = rect_nfa(I, r, lane); ++evals;
            if (v > log_nfa) { rec = r; log_nfa = v; }
        }
    }
    if (log_nfa > kLsdLogEps) return log_nfa;
    r = rec;
    for (int n = 0; n < 5; ++n) {
        if ((r.width - delta) >= 0.5) {
            r.p /= 2;
            r.prec = r.p * kPi;
            const double v = rect_nfa(I, r, lane); ++evals;
            if (v > log_nfa) { rec = r; log_nfa = v; }
        }
    }
    return log_nfa;
}

struct WalkShared {
    Rect rec;
    int ok;
};

__global__ __launch_bounds__(64) void k_lsd_walk(const LsdImage* imgs, LsdConst k, LsdResult* res) {
    const LsdImage& I = imgs[blockIdx.x];
    LsdResult& R = res[blockIdx.x];
    const int lane = threadIdx.x;
    const int N = (int)(I.sw * I.sh);
    __shared__ WalkShared sh;
    uint32_t n_out = 0, seeds = 0, evals = 0;
    for (int base = 0; base < N;) {
        const int pix = base + lane;
        const bool elig = pix < N && I.used[pix] == 0 && I.deg[pix] != kLsdNotDef;
        const unsigned long long m = __ballot(elig);
        if (!m) { base += 64; continue; }
        const int s = base + __ffsll((long long)m) - 1;
        base = s + 1;
        if (lane == 0) {
            ++seeds;
            double reg_angle;
            int n = region_grow(I, s % (int)I.sw, s / (int)I.sw, k.prec, reg_angle);
            int ok = n >= I.min_reg_size;
            if (ok) {
                region2rect(I, n, reg_angle, k.prec, k.p, sh.rec);
                ok = refine(I, n, reg_angle, k.prec, k.p, sh.rec);
            }
            sh.ok = ok;
        }
        __syncthreads();
        if (sh.ok) {
            Rect rec = sh.rec;
            const double log_nfa = rect_improve(I, rec, lane, evals);
            if (log_nfa > kLsdLogEps) {
                if (lane == 0 && n_out < I.out_cap)
                    I.out[n_out] = make_float4((float)((rec.x1 + 0.5) / kLsdScale), (float)((rec.y1 + 0.5) / kLsdScale),
                                               (float)((rec.x2 + 0.5) / kLsdScale), (float)((rec.y2 + 0.5) / kLsdScale));
                ++n_out;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        R.n = n_out;
        R.overflow = n_out > I.out_cap;
        R.seeds = seeds;
        R.nfa_evals = evals;
    }
}

}  // namespace

hipError_t launch_lsd(const LsdImage* d_imgs, uint32_t n, uint32_t max_src_pix, uint32_t max_small_pix,
                      uint32_t max_scaled_pix, const LsdConst& k, LsdResult* d_res, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t T = 256;
    hipLaunchKernelGGL(k_lsd_gray, dim3((max_src_pix + T - 1) / T, n), dim3(T), 0, st, d_imgs);
    hipLaunchKernelGGL(k_lsd_down, dim3((max_small_pix + T - 1) / T, n), dim3(T), 0, st, d_imgs);
    hipLaunchKernelGGL(k_lsd_blur_h, dim3((max_small_pix + T - 1) / T, n), dim3(T), 0, st, d_imgs, k);
    hipLaunchKernelGGL(k_lsd_blur_v, dim3((max_small_pix + T - 1) / T, n), dim3(T), 0, st, d_imgs, k);
    hipLaunchKernelGGL(k_lsd_grad, dim3((max_scaled_pix + T - 1) / T, n), dim3(T), 0, st, d_imgs, k, d_res);
    hipLaunchKernelGGL(k_lsd_walk, dim3(n), dim3(64), 0, st, d_imgs, k, d_res);
    return hipGetLastError();
}

}  // namespace l3d
