// l3d_lsd.hip -- host side of line-segment detection: Line3D::detectLineSegments (line3D.cc:243-370) for a batch of
// images.  The image checks, the max-width downscale geometry, the arena of device buffers, the launch of k_lsd.hip's
// stages, then per image the upscale, the length filter, the length order (the reference's std::priority_queue) and
// the cap; the segment cache of addImage (line3D.cc:295-309, 362-366).  DESIGN §11.
#include <sys/stat.h>

#include <array>
#include <atomic>
#include <cmath>
#include <queue>

#include "l3d_ctx.h"
#include "l3d_lsd.h"

namespace l3d {

std::atomic<uint64_t> g_lsd_images_detected{0};   // test hooks (l3d_debug_counter)
std::atomic<uint64_t> g_lsd_cache_loads{0};

namespace {

constexpr uint32_t kDefMaxNumSegments = 3000;     // L3D_DEF_MAX_NUM_SEGMENTS: the cache name carries this, not the cap
constexpr float kMinLineLengthFactor = 0.005f;    // L3D_DEF_MIN_LINE_LENGTH_FACTOR

// SegmentData2D and its comparator (commons.h:132-156): the heap looks at the length only
struct Seg2D { float p1x, p1y, p2x, p2y, length; };
struct SegLess { bool operator()(const Seg2D& a, const Seg2D& b) const { return a.length < b.length; } };

// cv::resize(src, dst, Size(), f, f): dsize = round(n * f)
uint32_t resize_size(uint32_t n, double f) { return (uint32_t)std::nearbyint((double)n * f); }

struct Geometry {
    uint32_t gw, gh, sw, sh;
    bool down;
    double down_scale;    // 1 / s
    float upx, upy;
};

Geometry geometry(const l3d_image& im, int max_image_width) {
    Geometry g{im.cols, im.rows, 0, 0, false, 1.0, 1.0f, 1.0f};
    const int max_dim = (int)std::max(im.cols, im.rows);
    if (max_image_width > 0 && max_dim > max_image_width) {
        const float s = float(max_image_width) / float(max_dim);
        g.gw = resize_size(im.cols, (double)s);
        g.gh = resize_size(im.rows, (double)s);
        g.down = true;
        g.down_scale = 1.0 / (double)s;
        g.upx = float(im.cols) / float(g.gw);
        g.upy = float(im.rows) / float(g.gh);
    }
    g.sw = resize_size(g.gw, kLsdScale);
    g.sh = resize_size(g.gh, kLsdScale);
    return g;
}

int check_image(const l3d_image& im) {
    if (im.channels != 1 && im.channels != 3)
        return fail(L3D_ERR_ARG, "image type not supported! must be CV_8U (gray) or CV_8UC3 (RGB)!");
    if (!im.data || im.cols < 2 || im.rows < 2 || im.row_stride < im.cols * im.channels)
        return fail(L3D_ERR_ARG, "empty image or row stride smaller than a row");
    if ((uint64_t)im.cols * im.rows * 3 >= (1ull << 31)) return fail(L3D_ERR_LIMIT, "image larger than 2^31 bytes");
    return L3D_OK;
}

// every stage needs at least 2 x 2 pixels (the resample maps index n - 1)
int check_geometry(const Geometry& g) {
    if (std::min({g.gw, g.gh, g.sw, g.sh}) < 2) return fail(L3D_ERR_ARG, "image too small for line-segment detection");
    return L3D_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// LSD on the device for every image; raw[i] = its segments in detection order (LSD-input pixels), stats filled.
// tap (test hook, l3d_debug_lsd_stages): one record per image whose non-null host buffers receive the stage maps, copied
// out of the arena after the stream is synchronised and before the arena is released; nullptr: nothing extra is copied.
int run_lsd(l3d_ctx* c, const std::vector<const l3d_image*>& ims, const std::vector<Geometry>& geo,
            std::vector<std::vector<float4>>& raw, std::vector<l3d_detect_stats>& stats, l3d_lsd_stages* tap = nullptr) {
    const uint32_t n = (uint32_t)ims.size();
    raw.assign(n, {});
    if (!n) return L3D_OK;
    std::vector<LsdImage> d(n);
    size_t bytes = align256(n * sizeof(LsdImage)) + align256(n * sizeof(LsdResult));
    uint32_t max_src = 0, max_small = 0, max_scaled = 0;
    // first pass: offsets inside the arena (pointers are offsets until the arena exists)
    std::vector<std::array<size_t, 10>> off(n);
    for (uint32_t i = 0; i < n; ++i) {
        const l3d_image& im = *ims[i];
        const Geometry& g = geo[i];
        const size_t src = (size_t)im.cols * im.rows, sm = (size_t)g.gw * g.gh, sc = (size_t)g.sw * g.sh;
        LsdImage& I = d[i];
        I.cols = im.cols; I.rows = im.rows; I.channels = im.channels;
        I.gw = g.gw; I.gh = g.gh; I.sw = g.sw; I.sh = g.sh;
        I.down = g.down; I.down_scale = g.down_scale;
        // every accepted segment keeps at least two pixels of its region marked used for good: at most sc / 2 of them
        I.out_cap = (uint32_t)(sc / 2 + 1);
        I.log_nt = 5 * (std::log10(double(g.sw)) + std::log10(double(g.sh))) / 2 + std::log10(11.0);
        I.min_reg_size = int(-I.log_nt / std::log10(22.5 / 180));
        const size_t sizes[10] = {src * im.channels, src, g.down ? sm : 0, sm * 8, sm * 8, sc * 4, sc * 8, sc,
                                  sc * sizeof(int2), (size_t)I.out_cap * sizeof(float4)};
        for (int k = 0; k < 10; ++k) { off[i][k] = bytes; bytes += align256(sizes[k]); }
        max_src = std::max(max_src, (uint32_t)src);
        max_small = std::max(max_small, (uint32_t)sm);
        max_scaled = std::max(max_scaled, (uint32_t)sc);
    }
    // (arena's destructor waits for the device -- block_cache_give outside a ReleaseSynced scope, or hipFree: that wait
    // is what protects the caller's raw on the L3D_HIP_CHECK returns below; never call this inside a ReleaseSynced scope)
    DevBuf<char> arena;
    L3D_HIP_CHECK(arena.reserve(bytes));
    char* base = arena.p;
    LsdImage* d_imgs = (LsdImage*)base;
    LsdResult* d_res = (LsdResult*)(base + align256(n * sizeof(LsdImage)));
    for (uint32_t i = 0; i < n; ++i) {
        LsdImage& I = d[i];
        const auto& o = off[i];
        I.src = (const uint8_t*)(base + o[0]);
        I.gray = (uint8_t*)(base + o[1]);
        I.small = I.down ? (uint8_t*)(base + o[2]) : I.gray;
        I.tmp = (double*)(base + o[3]);
        I.blur = (double*)(base + o[4]);
        I.deg = (float*)(base + o[5]);
        I.mod = (double*)(base + o[6]);
        I.used = (uint8_t*)(base + o[7]);
        I.reg = (int2*)(base + o[8]);
        I.out = (float4*)(base + o[9]);
        const l3d_image& im = *ims[i];
        const size_t row = (size_t)im.cols * im.channels;
        L3D_HIP_CHECK(hipMemcpy2DAsync((void*)I.src, row, im.data, im.row_stride, row, im.rows, hipMemcpyHostToDevice, c->stream));
    }
    L3D_HIP_CHECK(hipMemcpyAsync(d_imgs, d.data(), n * sizeof(LsdImage), hipMemcpyHostToDevice, c->stream));
    L3D_HIP_CHECK(hipMemsetAsync(d_res, 0, n * sizeof(LsdResult), c->stream));
    LsdConst k{};
    {
        // getGaussianKernel(7, sigma_scale / scale): exp(scale2X x x), normalised by the reciprocal of the sum
        const double sigma = 0.6 / kLsdScale, scale2x = -0.5 / (sigma * sigma);
        double sum = 0;
        for (int t = 0; t < kLsdTaps; ++t) {
            const double x = t - (kLsdTaps - 1) * 0.5;
            k.gauss[t] = std::exp(scale2x * x * x);
            sum += k.gauss[t];
        }
        sum = 1. / sum;
        for (int t = 0; t < kLsdTaps; ++t) k.gauss[t] *= sum;
        k.prec = M_PI * 22.5 / 180;
        k.p = 22.5 / 180;
        k.rho = 2.0 / std::sin(k.prec);
    }
    L3D_HIP_CHECK(launch_lsd(d_imgs, n, max_src, max_small, max_scaled, k, d_res, c->stream));
    std::vector<LsdResult> res(n);
    L3D_HIP_CHECK(hipMemcpyAsync(res.data(), d_res, n * sizeof(LsdResult), hipMemcpyDeviceToHost, c->stream));
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i) {
        if (res[i].overflow) {
            (void)hipStreamSynchronize(c->stream);   // the copies into raw[0 .. i) are still queued: the caller drops raw
            return fail(L3D_ERR_LIMIT, "line-segment detection: output capacity exceeded");
        }
        raw[i].resize(res[i].n);
        if (res[i].n)
            L3D_HIP_CHECK(hipMemcpyAsync(raw[i].data(), d[i].out, res[i].n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        l3d_detect_stats& s = stats[i];
        s.width = geo[i].gw; s.height = geo[i].gh;
        s.raw_segments = res[i].n; s.seeds = res[i].seeds; s.nfa_evals = res[i].nfa_evals;
        s.max_grad = -1.0;
        if (res[i].max_grad_bits) std::memcpy(&s.max_grad, &res[i].max_grad_bits, sizeof(double));
        if (tap) {
            l3d_lsd_stages& t = tap[i];
            const size_t src = (size_t)ims[i]->cols * ims[i]->rows, sm = (size_t)geo[i].gw * geo[i].gh;
            const size_t sc = (size_t)geo[i].sw * geo[i].sh;
            const struct { void* dst; const void* from; size_t bytes; } maps[5] = {
                {t.gray, d[i].gray, src}, {t.small_gray, d[i].small, sm}, {t.blur, d[i].blur, sm * sizeof(double)},
                {t.deg, d[i].deg, sc * sizeof(float)}, {t.mod, d[i].mod, sc * sizeof(double)}};
            for (const auto& m : maps)
                if (m.dst) L3D_HIP_CHECK(hipMemcpyAsync(m.dst, m.from, m.bytes, hipMemcpyDeviceToHost, c->stream));
            t.raw_segments = res[i].n; t.overflow = res[i].overflow;
            t.seeds = res[i].seeds; t.nfa_evals = res[i].nfa_evals; t.max_grad_bits = res[i].max_grad_bits;
            t.stats = s;
        }
    }
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    g_lsd_images_detected += n;
    return L3D_OK;
}

// line3D.cc:318-360: upscale, keep length > 0.005 diag (diag of the ORIGINAL image, float), longest first, cap
void finish(const l3d_image& im, const Geometry& g, const std::vector<float4>& raw, uint32_t max_segments,
            std::vector<float>& out) {
    const float diag = sqrtf(float(im.rows * im.rows) + float(im.cols * im.cols));
    const float min_len = diag * kMinLineLengthFactor;
    std::priority_queue<Seg2D, std::vector<Seg2D>, SegLess> sorted;
    for (const float4& d : raw) {
        Seg2D s;
        s.p1x = d.x * g.upx; s.p1y = d.y * g.upy;
        s.p2x = d.z * g.upx; s.p2y = d.w * g.upy;
        const float dx = s.p1x - s.p2x, dy = s.p1y - s.p2y;
        s.length = sqrtf(dx * dx + dy * dy);
        if (s.length > min_len) sorted.push(s);
    }
    const size_t m = std::min<size_t>(sorted.size(), max_segments);
    for (size_t pos = 0; pos < m; ++pos) {
        const Seg2D s = sorted.top();
        sorted.pop();
        out.insert(out.end(), {s.p1x, s.p1y, s.p2x, s.p2y});
    }
}

std::string cache_path(const l3d_detect_options& o, uint32_t cam, const Geometry& g) {
    char name[128];
    std::snprintf(name, sizeof name, "segments_L3D++_%u_%ux%u_%u.bin", cam, g.gw, g.gh, kDefMaxNumSegments);
    return std::string(o.output_folder ? o.output_folder : "") + "/L3D++_data/" + name;
}

int detect(l3d_ctx* c, uint32_t n, const uint32_t* cams, const l3d_image* images, int max_image_width,
           uint32_t max_segments, const l3d_detect_options* cache, uint32_t* counts) {
    if (!c || (n && !images)) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    for (uint32_t i = 0; i < n; ++i) if (int rc = check_image(images[i])) return rc;
    (void)hipSetDevice(c->device);
    std::vector<Geometry> geo(n);
    std::vector<l3d_detect_stats> stats(n, l3d_detect_stats{});
    std::vector<std::vector<float>> segs(n);
    std::vector<const l3d_image*> todo;
    std::vector<uint32_t> todo_idx;
    for (uint32_t i = 0; i < n; ++i) {
        geo[i] = geometry(images[i], max_image_width);
        if (int rc = check_geometry(geo[i])) return rc;
        if (cache && cache->load_segments) {
            const std::string path = cache_path(*cache, cams[i], geo[i]);
            std::ifstream probe(path, std::ios::binary);
            if (probe) {
                probe.close();
                uint32_t m = 0;
                if (int rc = l3d_read_segment_cache(path.c_str(), nullptr, 0, &m)) return rc;
                segs[i].resize(4 * (size_t)m);
                if (int rc = l3d_read_segment_cache(path.c_str(), segs[i].data(), m, &m)) return rc;
                stats[i].width = geo[i].gw; stats[i].height = geo[i].gh;
                stats[i].from_cache = 1;
                stats[i].max_grad = -1.0;
                ++g_lsd_cache_loads;
                continue;
            }
        }
        todo.push_back(&images[i]);
        todo_idx.push_back(i);
    }
    std::vector<Geometry> tgeo;
    std::vector<l3d_detect_stats> tstats(todo.size(), l3d_detect_stats{});
    for (uint32_t i : todo_idx) tgeo.push_back(geo[i]);
    std::vector<std::vector<float4>> raw;
    if (int rc = run_lsd(c, todo, tgeo, raw, tstats)) return rc;
    for (size_t j = 0; j < todo.size(); ++j) {
        const uint32_t i = todo_idx[j];
        stats[i] = tstats[j];
        finish(images[i], geo[i], raw[j], max_segments, segs[i]);
        // line3D.cc:362-366: stored only when segments were found
        if (cache && cache->load_segments && !segs[i].empty()) {
            const std::string dir = std::string(cache->output_folder ? cache->output_folder : "") + "/L3D++_data";
            ::mkdir(dir.c_str(), 0755);
            if (int rc = l3d_write_segment_cache(cache_path(*cache, cams[i], geo[i]).c_str(), segs[i].data(),
                                                 (uint32_t)(segs[i].size() / 4)))
                return rc;
        }
    }
    c->det_segs.clear();
    c->det_counts.assign(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        stats[i].segments = (uint32_t)(segs[i].size() / 4);
        c->det_counts[i] = stats[i].segments;
        if (counts) counts[i] = stats[i].segments;
        c->det_segs.insert(c->det_segs.end(), segs[i].begin(), segs[i].end());
    }
    c->det_stats = stats;
    return L3D_OK;
}

void tap_geometry(const Geometry& g, l3d_lsd_stages& t) {
    t.gw = g.gw; t.gh = g.gh; t.sw = g.sw; t.sh = g.sh;
    t.down = g.down;
    t.raw_cap = (uint32_t)((size_t)g.sw * g.sh / 2 + 1);      // LsdImage::out_cap
}

// l3d_debug_lsd_stages: detect()'s checks and its run_lsd call, with a tap and without the host's filter, order and cap
int lsd_stages(l3d_ctx* c, uint32_t n, const l3d_image* images, int max_image_width, bool query_only, l3d_lsd_stages* out) {
    if (!c || (n && (!images || !out))) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    for (uint32_t i = 0; i < n; ++i) if (int rc = check_image(images[i])) return rc;
    std::vector<Geometry> geo(n);
    std::vector<const l3d_image*> ims(n);
    for (uint32_t i = 0; i < n; ++i) {
        geo[i] = geometry(images[i], max_image_width);
        if (int rc = check_geometry(geo[i])) return rc;
        ims[i] = &images[i];
    }
    for (uint32_t i = 0; i < n; ++i) tap_geometry(geo[i], out[i]);
    if (query_only) return L3D_OK;
    (void)hipSetDevice(c->device);
    std::vector<l3d_detect_stats> stats(n, l3d_detect_stats{});
    std::vector<std::vector<float4>> raw;
    if (int rc = run_lsd(c, ims, geo, raw, stats, out)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (out[i].raw4 && !raw[i].empty()) std::memcpy(out[i].raw4, raw[i].data(), raw[i].size() * sizeof(float4));
    return L3D_OK;
}

int add_view_image(l3d_ctx* c, uint32_t camID, const l3d_image* image, const l3d_detect_options* opts, const double K[9],
                   const double R[9], const double t[3], float median_depth, const uint32_t* list, uint32_t n_list,
                   bool by_worldpoints, uint32_t* n_segments) {
    if (n_segments) *n_segments = 0;
    if (!c || !image || !opts || !K || !R || !t) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    // the checks addImage makes before it detects (line3D.cc:119-158): no detection for a view that cannot be added
    auto add = [&](const float* s, uint32_t m) {
        return by_worldpoints ? l3d_add_view_worldpoints(c, camID, s, m, K, R, t, image->cols, image->rows, median_depth, list, n_list)
                              : l3d_add_view(c, camID, s, m, K, R, t, image->cols, image->rows, median_depth, list, n_list);
    };
    if (std::max(image->cols, image->rows) < 800 || c->views.count(camID) || !n_list || !list) return add(nullptr, 0);
    uint32_t m = 0;
    if (int rc = detect(c, 1, &camID, image, opts->max_image_width, opts->max_line_segments, opts, &m)) return rc;
    if (!m) return fail(L3D_ERR_NO_SEGMENTS, "no line segments found in image");
    const int rc = add(c->det_segs.data(), m);
    if (rc == L3D_OK && n_segments) *n_segments = m;     // still under the context mutex: this view's own count
    return rc;
}

// Line3D::undistortImage's input checks, made before any pixel is read or any memory is allocated.  Only
// fx, fy, cx, cy of K are read (cvK drops the skew and sets K(2,2) to 1).
int check_undistort(const l3d_image& im, const l3d_distortion& d) {
    if (int rc = check_image(im)) return rc;
    const double used[9] = {d.K[0], d.K[4], d.K[2], d.K[5], d.radial[0], d.radial[1], d.radial[2], d.tangential[0],
                            d.tangential[1]};
    for (double v : used)
        if (!std::isfinite(v)) return fail(L3D_ERR_ARG, "undistortImage: non-finite distortion coefficient or camera matrix entry");
    if (d.K[0] * d.K[4] == 0) return fail(L3D_ERR_ARG, "undistortImage: fx * fy == 0, the camera matrix is singular");
    if (im.cols >= 32767 || im.rows >= 32767)
        return fail(L3D_ERR_LIMIT, "undistortImage: image side of SHRT_MAX or more (cv::remap refuses it)");
    return L3D_OK;
}

// The batch behind both undistortion entries: inputs up, one launch (grid.y = image), outputs down.  Rec is
// the kernel's per-image record; fill(i, U) sets its coefficients and fx, fy, cx, cy and returns the camera matrix of
// the OUTPUT image, from which the inverse and the column table are built here.
template <class Rec, class Fill, class Launch>
int undistort_batch(l3d_ctx* c, uint32_t n, const l3d_image* in, uint8_t* const* out, Fill fill, Launch launch) {
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!n) return L3D_OK;
    (void)hipSetDevice(c->device);
    std::vector<Rec> d(n);
    std::vector<std::vector<double>> xtab(n);
    std::vector<std::array<size_t, 3>> off(n);
    size_t bytes = align256(n * sizeof(Rec));
    uint32_t max_pix = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const l3d_image& im = in[i];
        Rec& U = d[i];
        const double* Kn = fill(i, U);
        // cv::invert's closed form (DECOMP_LU, n = 3) of cvK, reduced: ir1, ir3, ir6, ir7 are +-0
        const double fx = Kn[0], fy = Kn[4], cx = Kn[2], cy = Kn[5];
        const double det = fx * fy, dd = 1.0 / det;
        const double ir0 = fy * dd, ir2 = (-(cx * fy)) * dd, ir8 = (fx * fy) * dd;
        U.cols = im.cols; U.rows = im.rows; U.channels = im.channels;
        U.w = 1.0 / ir8; U.ir4 = fx * dd; U.ir5 = (-(fx * cy)) * dd;
        // OpenCV accumulates _x += ir[0] along a row; ir1 = 0, so every row starts from ir2 and one table serves all
        std::vector<double>& X = xtab[i];
        X.resize(im.cols);
        X[0] = ir2;
        for (uint32_t j = 1; j < im.cols; ++j) X[j] = X[j - 1] + ir0;
        const size_t px = align256((size_t)im.cols * im.rows * im.channels);
        off[i] = {bytes, bytes + px, bytes + 2 * px};
        bytes += 2 * px + align256(im.cols * sizeof(double));
        max_pix = std::max(max_pix, im.cols * im.rows);
    }
    DevBuf<char> arena;
    L3D_HIP_CHECK(arena.reserve(bytes));
    char* base = arena.p;
    for (uint32_t i = 0; i < n; ++i) {
        Rec& U = d[i];
        U.src = (const uint8_t*)(base + off[i][0]);
        U.dst = (uint8_t*)(base + off[i][1]);
        U.xtab = (const double*)(base + off[i][2]);
        const size_t row = (size_t)in[i].cols * in[i].channels;
        L3D_HIP_CHECK(hipMemcpy2DAsync((void*)U.src, row, in[i].data, in[i].row_stride, row, in[i].rows, hipMemcpyHostToDevice, c->stream));
        L3D_HIP_CHECK(hipMemcpyAsync((void*)U.xtab, xtab[i].data(), in[i].cols * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    L3D_HIP_CHECK(hipMemcpyAsync(base, d.data(), n * sizeof(Rec), hipMemcpyHostToDevice, c->stream));
    L3D_HIP_CHECK(launch((const Rec*)base, n, max_pix, c->stream));
    // after every upload in stream order: out[i] may be the memory of an input
    for (uint32_t i = 0; i < n; ++i)
        L3D_HIP_CHECK(hipMemcpyAsync(out[i], d[i].dst, (size_t)in[i].cols * in[i].rows * in[i].channels, hipMemcpyDeviceToHost, c->stream));
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    return L3D_OK;
}

// Line3D::undistortImage for a batch: one k_undistort launch
int undistort(l3d_ctx* c, uint32_t n, const l3d_image* in, const l3d_distortion* dist, uint8_t* const* out) {
    if (!c || (n && (!in || !dist || !out))) return fail(L3D_ERR_ARG, "null argument");
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = check_undistort(in[i], dist[i])) return rc;
        if (!out[i]) return fail(L3D_ERR_ARG, "null argument");
    }
    return undistort_batch<UndImage>(c, n, in, out, [&](uint32_t i, UndImage& U) {
        const l3d_distortion& D = dist[i];
        U.fx = D.K[0]; U.fy = D.K[4]; U.cx = D.K[2]; U.cy = D.K[5];
        U.k1 = D.radial[0]; U.k2 = D.radial[1]; U.k3 = D.radial[2]; U.p1 = D.tangential[0]; U.p2 = D.tangential[1];
        return D.K;
    }, launch_undistort);
}

// the number of distortion parameters of an l3d_camera_model's model, 0 for an unknown one
uint32_t model_params(uint32_t model) {
    switch (model) {
        case L3D_CAM_FULL_OPENCV: return 8;
        case L3D_CAM_OPENCV_FISHEYE: return 4;
        case L3D_CAM_SIMPLE_RADIAL_FISHEYE: return 1;
        case L3D_CAM_RADIAL_FISHEYE: return 2;
        case L3D_CAM_FOV: return 1;
        default: return 0;
    }
}

bool has_new_K(const l3d_camera_model& m) {
    for (double v : m.K_new)
        if (!(v == 0)) return true;          // (a NaN counts as given, and is refused below)
    return false;
}

// the checks of §12 for the model entry, before any pixel is read or any memory is allocated
int check_undistort_model(const l3d_image& im, const l3d_camera_model& m) {
    if (int rc = check_image(im)) return rc;
    const uint32_t np = model_params(m.model);
    if (!np) return fail(L3D_ERR_ARG, "undistortImage: unknown camera model " + std::to_string(m.model));
    const bool kn = has_new_K(m);
    double used[16] = {m.K[0], m.K[4], m.K[2], m.K[5], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < np; ++k) used[4 + k] = m.params[k];
    if (kn) { used[12] = m.K_new[0]; used[13] = m.K_new[4]; used[14] = m.K_new[2]; used[15] = m.K_new[5]; }
    for (double v : used)
        if (!std::isfinite(v)) return fail(L3D_ERR_ARG, "undistortImage: non-finite distortion coefficient or camera matrix entry");
    if (m.K[0] * m.K[4] == 0 || (kn && m.K_new[0] * m.K_new[4] == 0))
        return fail(L3D_ERR_ARG, "undistortImage: fx * fy == 0, the camera matrix is singular");
    if (im.cols >= 32767 || im.rows >= 32767)
        return fail(L3D_ERR_LIMIT, "undistortImage: image side of SHRT_MAX or more (cv::remap refuses it)");
    return L3D_OK;
}

// undistortion by camera model for a batch: one k_undistort_model launch
int undistort_model(l3d_ctx* c, uint32_t n, const l3d_image* in, const l3d_camera_model* cams, uint8_t* const* out) {
    if (!c || (n && (!in || !cams || !out))) return fail(L3D_ERR_ARG, "null argument");
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = check_undistort_model(in[i], cams[i])) return rc;
        if (!out[i]) return fail(L3D_ERR_ARG, "null argument");
    }
    return undistort_batch<UndModelImage>(c, n, in, out, [&](uint32_t i, UndModelImage& U) {
        const l3d_camera_model& m = cams[i];
        const double* p = m.params;
        U.fx = m.K[0]; U.fy = m.K[4]; U.cx = m.K[2]; U.cy = m.K[5];
        U.model = m.model;
        U.k1 = U.k2 = U.k3 = U.p1 = U.p2 = 0;
        U.q[0] = U.q[1] = U.q[2] = U.q[3] = 0;
        switch (m.model) {
            case L3D_CAM_FULL_OPENCV:
                U.k1 = p[0]; U.k2 = p[1]; U.p1 = p[2]; U.p2 = p[3]; U.k3 = p[4];
                U.q[0] = p[5]; U.q[1] = p[6]; U.q[2] = p[7];
                break;
            case L3D_CAM_FOV:                // tan(omega / 2) once per image, on the host
                U.q[0] = p[0]; U.q[1] = p[0] * p[0]; U.q[2] = std::tan(p[0] / 2);
                break;
            default:                         // the fisheye family: the missing coefficients stay 0
                for (uint32_t k = 0; k < model_params(m.model); ++k) U.q[k] = p[k];
        }
        return has_new_K(m) ? m.K_new : m.K;
    }, launch_undistort_model);
}

}  // namespace
}  // namespace l3d

using namespace l3d;

extern "C" {

int l3d_detect_segments(l3d_ctx* c, uint32_t n_images, const l3d_image* images, int max_image_width,
                        uint32_t max_segments, uint32_t* counts) {
    return detect(c, n_images, nullptr, images, max_image_width, max_segments, nullptr, counts);
}

int l3d_detect_view_segments(l3d_ctx* c, uint32_t n_images, const uint32_t* camIDs, const l3d_image* images,
                             const l3d_detect_options* opts, uint32_t* counts) {
    if (!opts || (n_images && !camIDs)) return fail(L3D_ERR_ARG, "null argument");
    return detect(c, n_images, camIDs, images, opts->max_image_width, opts->max_line_segments, opts, counts);
}

int l3d_debug_lsd_stages(l3d_ctx* c, uint32_t n_images, const l3d_image* images, int max_image_width, int query_only,
                         l3d_lsd_stages* out) {
    return lsd_stages(c, n_images, images, max_image_width, query_only != 0, out);
}

int l3d_get_detected_segments(l3d_ctx* c, float* segs4, uint64_t cap, uint64_t* n) {
    if (!c || !n) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    *n = c->det_segs.size() / 4;
    if (segs4) std::memcpy(segs4, c->det_segs.data(), std::min<uint64_t>(cap, *n) * 16);
    return L3D_OK;
}

int l3d_get_detect_stats(l3d_ctx* c, l3d_detect_stats* out, uint32_t cap, uint32_t* n) {
    if (!c || !n) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    *n = (uint32_t)c->det_stats.size();
    if (out) std::memcpy(out, c->det_stats.data(), std::min<uint32_t>(cap, *n) * sizeof(l3d_detect_stats));
    return L3D_OK;
}

int l3d_add_view_image(l3d_ctx* c, uint32_t camID, const l3d_image* image, const l3d_detect_options* opts,
                       const double K[9], const double R[9], const double t[3], float median_depth,
                       const uint32_t* neighbors, uint32_t n_neighbors, uint32_t* n_segments) {
    return add_view_image(c, camID, image, opts, K, R, t, median_depth, neighbors, n_neighbors, false, n_segments);
}

int l3d_add_view_image_worldpoints(l3d_ctx* c, uint32_t camID, const l3d_image* image, const l3d_detect_options* opts,
                                   const double K[9], const double R[9], const double t[3], float median_depth,
                                   const uint32_t* worldpoints, uint32_t n_worldpoints, uint32_t* n_segments) {
    return add_view_image(c, camID, image, opts, K, R, t, median_depth, worldpoints, n_worldpoints, true, n_segments);
}

int l3d_undistort_images(l3d_ctx* c, uint32_t n_images, const l3d_image* in, const l3d_distortion* dist,
                         uint8_t* const* out) {
    return undistort(c, n_images, in, dist, out);
}

int l3d_undistort_images_model(l3d_ctx* c, uint32_t n_images, const l3d_image* in, const l3d_camera_model* cams,
                               uint8_t* const* out) {
    return undistort_model(c, n_images, in, cams, out);
}

}  // extern "C"
