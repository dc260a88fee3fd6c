// l3d_project.hip -- host side of the projection stages (kernels: k_project.hip): the 3D lines projected into
// cameras (l3d_project_segments / l3d_project_lines), rendered into line-id and inverse-depth planes
// (l3d_render_line_maps / l3d_render_lines) and drawn over images (l3d_draw_line_maps / l3d_draw_lines).  The context
// forms work on the lines the last reconstruct3Dlines left, on the context's stream and work space; the stateless forms
// bring a work space of their own and use the default stream, as l3d_triangulate_points does.
//
// Cameras are taken in GROUPS under a device-memory budget of kProjBudget = 256 MiB (l3d_set_projection_budget: a test
// hook that makes the groups small): stage 1 for the uncompacted and the
// compacted records of (camera, segment) (68 bytes each), stages 2 and 3 for the key planes (8 bytes per pixel: 16
// views of 2 Mpixel).  Every camera's result is computed from its own records in its own planes, so the grouping changes
// nothing but the number of launches.  Small tables go through pinned staging; planes and images are large and are
// copied straight between the caller's memory and the device.
#include "l3d_ctx.h"

using namespace l3d;

namespace {

constexpr size_t kProjBudget = (size_t)256 << 20;
constexpr uint32_t kProjMaxGroup = 4096;       // cameras per group at most (they are grid.y of the per-pixel kernels)
constexpr uint32_t kProjMaxSide = 65535;       // image sides: a camera's pixels are counted in 32 bits
static_assert(sizeof(ProjRecord) == sizeof(l3d_projected_segment) && sizeof(ProjRecord) == 32, "record layout");

int hip_fail(const char* where, hipError_t e) { return fail(L3D_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e)); }

int check_near(double near_plane) {
    if (!(near_plane > 0.0) || !std::isfinite(near_plane)) return fail(L3D_ERR_ARG, "the near plane must be positive and finite");
    return L3D_OK;
}
int check_camera_size(uint32_t c, const l3d_camera& cam) {
    if (!cam.width || !cam.height) return fail(L3D_ERR_ARG, "camera " + std::to_string(c) + " has a side of zero pixels");
    if (cam.width > kProjMaxSide || cam.height > kProjMaxSide)
        return fail(L3D_ERR_LIMIT, "camera " + std::to_string(c) + " has a side of more than 65535 pixels");
    return L3D_OK;
}
int check_cameras(uint32_t n_cams, const l3d_camera* cams) {
    if (n_cams && !cams) return fail(L3D_ERR_ARG, "null argument");
    for (uint32_t c = 0; c < n_cams; ++c) {
        if (int rc = check_camera_size(c, cams[c])) return rc;
        bool finite = true;
        for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(cams[c].K[k]) && std::isfinite(cams[c].R[k]);
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(cams[c].t[k]);
        if (!finite) return fail(L3D_ERR_ARG, "camera " + std::to_string(c) + " has a non-finite entry");
    }
    return L3D_OK;
}
int check_records(uint64_t n, const l3d_projected_segment* rec) {
    if (n && !rec) return fail(L3D_ERR_ARG, "null argument");
    for (uint64_t i = 0; i < n; ++i) {
        const l3d_projected_segment& r = rec[i];
        if (!(std::isfinite(r.x1) && std::isfinite(r.y1) && std::isfinite(r.x2) && std::isfinite(r.y2) &&
              std::isfinite(r.inv_depth1) && std::isfinite(r.inv_depth2)))
            return fail(L3D_ERR_ARG, "record " + std::to_string(i) + " has a non-finite entry");
        if (r.line > 0x7FFFFFFFu) return fail(L3D_ERR_LIMIT, "record " + std::to_string(i) + " names a line index of 2^31 or more");
    }
    return L3D_OK;
}
int check_images(uint32_t n, const l3d_image* images, const std::vector<std::pair<uint32_t, uint32_t>>* sizes) {
    if (n && !images) return fail(L3D_ERR_ARG, "null argument");
    for (uint32_t c = 0; c < n; ++c) {
        const l3d_image& im = images[c];
        if (!im.data) return fail(L3D_ERR_ARG, "null argument");
        if (im.channels != 1 && im.channels != 3) return fail(L3D_ERR_ARG, "image type not supported! must be 8-bit with 1 or 3 channels");
        if (!im.cols || !im.rows) return fail(L3D_ERR_ARG, "image " + std::to_string(c) + " has a side of zero pixels");
        if (im.cols > kProjMaxSide || im.rows > kProjMaxSide) return fail(L3D_ERR_LIMIT, "image " + std::to_string(c) + " has a side of more than 65535 pixels");
        if ((uint64_t)im.row_stride < (uint64_t)im.cols * im.channels) return fail(L3D_ERR_ARG, "image " + std::to_string(c) + ": row_stride is shorter than a row");
        if (sizes && (im.cols != (*sizes)[c].first || im.rows != (*sizes)[c].second))
            return fail(L3D_ERR_ARG, "image " + std::to_string(c) + " is " + std::to_string(im.cols) + " x " + std::to_string(im.rows) +
                                         ", its camera " + std::to_string((*sizes)[c].first) + " x " + std::to_string((*sizes)[c].second));
    }
    return L3D_OK;
}

// ---- stage 1 --------------------------------------------------------------------------------------------------------
// P6: n_seg x (P1, P2); counts[n_cams]; out: the visible records, camera after camera.  Arguments already checked.
int project_core(ProjWork& w, hipStream_t st, uint32_t n_cams, const l3d_camera* cams, uint32_t n_seg, const double* P6,
                 const uint32_t* line, double near_plane, uint32_t* counts, std::vector<l3d_projected_segment>& out) {
    out.clear();
    for (uint32_t c = 0; c < n_cams; ++c) counts[c] = 0;
    if (!n_cams || !n_seg) return L3D_OK;
    const size_t per_cam = 68 * (size_t)n_seg;
    const uint32_t g_max = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(kProjMaxGroup, projection_budget(w) / per_cam),
                                                                           ((size_t)1 << 31) / n_seg));
    for (uint32_t c0 = 0; c0 < n_cams; c0 += g_max) {
        const uint32_t g = std::min(g_max, n_cams - c0);
        const size_t n = (size_t)g * n_seg;
        Layout lay;
        const size_t o_cam = lay.take(sizeof(ProjCam) * g), o_P = lay.take(48 * (size_t)n_seg), o_line = lay.take(4 * (size_t)n_seg);
        const size_t in_bytes = lay.at, o_bounds = lay.take(4 * ((size_t)g + 1)), host_bytes = lay.at;
        const size_t o_vis = lay.take(4 * (n + 1)), o_rec = lay.take(32 * n), o_out = lay.take(32 * n), total = lay.at;
        if (w.h.reserve(host_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess ||
            w.scan_ws.reserve_zeroed(scan_ws_words(n, 4), st) != hipSuccess)
            return fail(L3D_ERR_HIP, "projection: allocation failed");
        char* h = w.h.p; char* d = w.d.p;
        for (uint32_t c = 0; c < g; ++c) {
            ProjCam pc;
            std::memcpy(pc.K, cams[c0 + c].K, 72); std::memcpy(pc.R, cams[c0 + c].R, 72); std::memcpy(pc.t, cams[c0 + c].t, 24);
            pc.xmax = (double)(cams[c0 + c].width - 1); pc.ymax = (double)(cams[c0 + c].height - 1);
            std::memcpy(h + o_cam + sizeof(ProjCam) * c, &pc, sizeof(ProjCam));
        }
        std::memcpy(h + o_P, P6, 48 * (size_t)n_seg);
        std::memcpy(h + o_line, line, 4 * (size_t)n_seg);
        uint32_t* h_bounds = (uint32_t*)(h + o_bounds);
        ProjArgs a{(const ProjCam*)(d + o_cam), g, n_seg, (const double*)(d + o_P), (const uint32_t*)(d + o_line), near_plane,
                   (ProjRecord*)(d + o_rec), (uint32_t*)(d + o_vis), (ProjRecord*)(d + o_out), (uint32_t*)(d + o_bounds)};
        hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launch_project_stage1(w, a, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_bounds, a.bounds, 4 * ((size_t)g + 1), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail("projection", e);
        const size_t n_vis = h_bounds[g], at = out.size();
        if (n_vis > n) return fail(L3D_ERR_HIP, "projection: the compaction reports more records than segments");
        for (uint32_t c = 0; c < g; ++c) counts[c0 + c] = h_bounds[c + 1] - h_bounds[c];
        if (n_vis) {
            out.resize(at + n_vis);
            e = hipMemcpyAsync(out.data() + at, a.out, 32 * n_vis, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_fail("projection", e);
        }
    }
    return L3D_OK;
}

// the segments of a caller: end points finite, at most 2^30 of them, line indices below 2^31
int gather_segments(uint32_t n_seg, const l3d_segment3d* segs, const uint32_t* line, std::vector<double>& P6) {
    if (n_seg && (!segs || !line)) return fail(L3D_ERR_ARG, "null argument");
    if (n_seg > L3D_PROJ_SEGMENT_MASK) return fail(L3D_ERR_LIMIT, "more than 2^30 segments");
    P6.resize(6 * (size_t)n_seg);
    for (uint32_t i = 0; i < n_seg; ++i) {
        for (int k = 0; k < 3; ++k) { P6[6 * (size_t)i + k] = segs[i].P1[k]; P6[6 * (size_t)i + 3 + k] = segs[i].P2[k]; }
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(P6[6 * (size_t)i + k])) return fail(L3D_ERR_ARG, "segment " + std::to_string(i) + " has a non-finite end point");
        if (line[i] > 0x7FFFFFFFu) return fail(L3D_ERR_LIMIT, "segment " + std::to_string(i) + " names a line index of 2^31 or more");
    }
    return L3D_OK;
}

// ---- stages 2 and 3 ---------------------------------------------------------------------------------------------------
struct MapJob {
    uint32_t n_cams = 0;
    std::vector<std::pair<uint32_t, uint32_t>> size;      // (width, height) per camera
    bool raster = false;                                  // line ids from records (stage 2) ...
    const uint32_t* n_rec = nullptr; const l3d_projected_segment* rec = nullptr; uint32_t thickness = 1;
    const int32_t* const* ids_in = nullptr;               // ... or from the caller's planes
    int32_t* const* ids_out = nullptr; float* const* iz_out = nullptr;   // planes out (the arrays or entries may be null)
    const l3d_image* images = nullptr;                    // stage 3 when set
    const uint8_t* colors = nullptr; uint32_t n_lines = 0, alpha = 255; uint8_t* const* rgb_out = nullptr;
};

int maps_core(ProjWork& w, hipStream_t st, const MapJob& j) {
    uint64_t rec_at = 0;
    for (uint32_t c0 = 0; c0 < j.n_cams;) {
        // the group: cameras while their key planes fit the budget (one at least)
        uint32_t c1 = c0; uint64_t n_pix = 0; uint32_t max_pix = 0; uint64_t n_rec = 0, img_bytes = 0;
        std::vector<MapCam> mc;
        while (c1 < j.n_cams && c1 - c0 < kProjMaxGroup) {
            const uint64_t pix = (uint64_t)j.size[c1].first * j.size[c1].second;
            if (c1 > c0 && (n_pix + pix) * 8 > projection_budget(w)) break;
            MapCam m{};
            m.width = j.size[c1].first; m.height = j.size[c1].second; m.rec0 = (uint32_t)n_rec; m.pix0 = n_pix; m.rgb_off = 3 * n_pix;
            if (j.images) {
                const l3d_image& im = j.images[c1];
                m.img_stride = im.row_stride; m.img_channels = im.channels; m.img_off = img_bytes;
                img_bytes += up256((uint64_t)(im.rows - 1) * im.row_stride + (uint64_t)im.cols * im.channels);
            }
            mc.push_back(m);
            n_pix += pix; max_pix = std::max<uint32_t>(max_pix, (uint32_t)pix);
            if (j.raster) n_rec += j.n_rec[c1];
            ++c1;
        }
        const uint32_t g = c1 - c0;
        if (n_rec >= ((uint64_t)1 << 31)) return fail(L3D_ERR_LIMIT, "more than 2^31 records in a group of cameras");
        const l3d_projected_segment* rec = j.raster ? j.rec + rec_at : nullptr;
        // an upper bound of the major-axis steps: sizes the launch, and keeps the 32-bit scan from overflowing
        uint64_t step_bound = 0;
        if (j.raster)
            for (uint32_t c = 0, r = 0; c < g; ++c) {
                const double side = (double)std::max(mc[c].width, mc[c].height);
                for (uint32_t k = 0; k < j.n_rec[c0 + c]; ++k, ++r) {
                    const double ext = std::max(std::fabs((double)rec[r].x2 - (double)rec[r].x1), std::fabs((double)rec[r].y2 - (double)rec[r].y1));
                    step_bound += std::isfinite(ext) ? (uint64_t)std::min(ext + 2.0, side) : (uint64_t)side;   // (records are finite)
                }
            }
        if (step_bound >= ((uint64_t)1 << 32)) return fail(L3D_ERR_LIMIT, "more than 2^32 raster steps in a group of cameras");
        const size_t b_cam = sizeof(MapCam) * g, b_rec = 32 * (size_t)n_rec, b_col = j.colors ? 3 * (size_t)j.n_lines : 0;
        Layout lay;
        const size_t o_cam = lay.take(b_cam), o_rec = lay.take(b_rec), o_col = lay.take(b_col), in_bytes = lay.at;
        const size_t o_steps = lay.take(4 * ((size_t)n_rec + 1)), o_ids = lay.take(4 * n_pix), o_iz = lay.take(4 * n_pix);
        const size_t o_img = lay.take(img_bytes), o_rgb = lay.take(j.images ? 3 * n_pix : 0), total = lay.at;
        if (w.h.reserve(in_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess ||
            (j.raster && (w.keys.reserve(n_pix) != hipSuccess || w.scan_ws.reserve_zeroed(scan_ws_words(n_rec, 4), st) != hipSuccess)))
            return fail(L3D_ERR_HIP, "line maps: allocation failed");
        char* h = w.h.p; char* d = w.d.p;
        std::memcpy(h + o_cam, mc.data(), b_cam);
        if (b_rec) std::memcpy(h + o_rec, rec, b_rec);
        if (b_col) std::memcpy(h + o_col, j.colors, b_col);
        MapArgs a{};
        a.cams = (const MapCam*)(d + o_cam); a.n_cams = g;
        a.rec = (const ProjRecord*)(d + o_rec); a.n_rec = (uint32_t)n_rec;
        a.steps = (uint32_t*)(d + o_steps); a.thickness = j.thickness;
        a.keys = w.keys.p; a.n_pix = n_pix; a.max_pix = max_pix;
        a.line_id = (int32_t*)(d + o_ids); a.inv_depth = (float*)(d + o_iz);
        a.img = (const uint8_t*)(d + o_img); a.rgb = (uint8_t*)(d + o_rgb);
        a.colors = b_col ? (const uint8_t*)(d + o_col) : nullptr; a.n_lines = j.n_lines; a.alpha = j.alpha;
        hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st);
        if (j.raster) {
            if (e == hipSuccess) e = hipMemsetAsync(a.keys, 0, 8 * n_pix, st);
            if (n_rec) {
                if (e == hipSuccess) e = launch_raster_count(a, st);
                if (e == hipSuccess) e = launch_scan(a.steps, a.n_rec, a.steps, w.scan_ws.p, nullptr, st);
                if (e == hipSuccess) e = launch_raster_lines(a, (uint32_t)std::min<uint64_t>(2048, (step_bound + 255) / 256), st);
            }
            if (e == hipSuccess) e = launch_map_decode(a, st);
        } else {
            for (uint32_t c = 0; c < g && e == hipSuccess; ++c)
                e = hipMemcpyAsync(a.line_id + mc[c].pix0, j.ids_in[c0 + c], 4 * (size_t)mc[c].width * mc[c].height, hipMemcpyHostToDevice, st);
        }
        if (j.images) {
            for (uint32_t c = 0; c < g && e == hipSuccess; ++c) {
                const l3d_image& im = j.images[c0 + c];
                e = hipMemcpyAsync(d + o_img + mc[c].img_off, im.data, (size_t)(im.rows - 1) * im.row_stride + (size_t)im.cols * im.channels,
                                   hipMemcpyHostToDevice, st);
            }
            if (e == hipSuccess) e = launch_overlay(a, st);
        }
        for (uint32_t c = 0; c < g && e == hipSuccess; ++c) {
            const size_t pix = (size_t)mc[c].width * mc[c].height;
            if (j.ids_out && j.ids_out[c0 + c]) e = hipMemcpyAsync(j.ids_out[c0 + c], a.line_id + mc[c].pix0, 4 * pix, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && j.iz_out && j.iz_out[c0 + c])
                e = hipMemcpyAsync(j.iz_out[c0 + c], a.inv_depth + mc[c].pix0, 4 * pix, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && j.images) e = hipMemcpyAsync(j.rgb_out[c0 + c], a.rgb + mc[c].rgb_off, 3 * pix, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail("line maps", e);
        rec_at += n_rec;
        c0 = c1;
    }
    return L3D_OK;
}

int check_thickness(uint32_t thickness) {
    if (!(thickness & 1u)) return fail(L3D_ERR_ARG, "thickness must be odd (1, 3, 5, ...)");
    if (thickness > 255) return fail(L3D_ERR_LIMIT, "thickness beyond 255 pixels");
    return L3D_OK;
}
int check_alpha(uint32_t alpha) { return alpha > 255 ? fail(L3D_ERR_ARG, "alpha must be 0 ... 255") : L3D_OK; }
template <class T>
int check_pointers(uint32_t n, T* const* p) {
    if (n && !p) return fail(L3D_ERR_ARG, "null argument");
    for (uint32_t c = 0; c < n; ++c)
        if (!p[c]) return fail(L3D_ERR_ARG, "null argument");
    return L3D_OK;
}
std::vector<std::pair<uint32_t, uint32_t>> camera_sizes(uint32_t n_cams, const l3d_camera* cams) {
    std::vector<std::pair<uint32_t, uint32_t>> s(n_cams);
    for (uint32_t c = 0; c < n_cams; ++c) s[c] = {cams[c].width, cams[c].height};
    return s;
}

}  // namespace

// shared with l3d_associate.hip: the budget of a group of cameras, and stage 1 on the context's lines (mutex held)
namespace l3d {
size_t projection_budget(const ProjWork& w) { return w.budget ? w.budget : kProjBudget; }
int check_projection_cameras(uint32_t n_cams, const l3d_camera* cams, double near_plane) {
    if (int rc = check_near(near_plane)) return rc;
    return check_cameras(n_cams, cams);
}
hipError_t launch_project_stage1(ProjWork& w, const ProjArgs& a, hipStream_t st) {
    const size_t n = (size_t)a.n_cams * a.n_seg;
    hipError_t e = launch_project_lines(a, st);
    if (e == hipSuccess) e = launch_scan(a.vis, (uint32_t)n, a.vis, w.scan_ws.p, nullptr, st);
    if (e == hipSuccess) e = launch_project_compact(a, st);
    return e;
}
int project_context_lines(l3d_ctx* c, uint32_t n_cams, const l3d_camera* cams, double near_plane, std::vector<uint32_t>& counts) {
    if (int rc = lines_ready(c, nullptr, "project")) return rc;
    if (int rc = set_device(c->device)) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (line.size() > L3D_PROJ_SEGMENT_MASK) return fail(L3D_ERR_LIMIT, "more than 2^30 segments");
    counts.assign(n_cams, 0);
    return project_core(c->proj, c->stream, n_cams, cams, (uint32_t)line.size(), P6.data(), line.data(), near_plane, counts.data(),
                        c->proj_records);
}
}  // namespace l3d

extern "C" {

int l3d_project_segments(int device, uint32_t n_cams, const l3d_camera* cams, uint32_t n_segments, const l3d_segment3d* segments,
                         const uint32_t* line_of_segment, double near_plane, uint32_t* counts, l3d_projected_segment* out,
                         uint64_t cap, uint64_t* n) {
    if (!n || (n_cams && !counts)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_near(near_plane)) return rc;
    if (int rc = check_cameras(n_cams, cams)) return rc;
    std::vector<double> P6;
    if (int rc = gather_segments(n_segments, segments, line_of_segment, P6)) return rc;
    std::vector<l3d_projected_segment> rec;
    std::vector<uint32_t> cnt(n_cams, 0);
    if (n_cams && n_segments) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        if (int rc = project_core(w, 0, n_cams, cams, n_segments, P6.data(), line_of_segment, near_plane, cnt.data(), rec)) return rc;
    }
    for (uint32_t c = 0; c < n_cams; ++c) counts[c] = cnt[c];
    *n = rec.size();
    if (out && !rec.empty()) std::memcpy(out, rec.data(), 32 * (size_t)std::min<uint64_t>(cap, rec.size()));
    return L3D_OK;
}

int l3d_render_line_maps(int device, uint32_t n_cams, const l3d_camera* cams, const uint32_t* n_records_per_cam,
                         const l3d_projected_segment* records, uint32_t thickness, int32_t* const* line_id_planes,
                         float* const* inv_depth_planes) {
    if (!n_cams) return L3D_OK;
    if (!cams || !n_records_per_cam) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thickness(thickness)) return rc;
    if (int rc = check_pointers(n_cams, line_id_planes)) return rc;
    for (uint32_t c = 0; c < n_cams; ++c)            // (the sizes only: K, R and t are not read here)
        if (int rc = check_camera_size(c, cams[c])) return rc;
    uint64_t n_rec = 0;
    for (uint32_t c = 0; c < n_cams; ++c) n_rec += n_records_per_cam[c];
    if (int rc = check_records(n_rec, records)) return rc;
    if (int rc = set_device(device)) return rc;
    MapJob j;
    j.n_cams = n_cams; j.size = camera_sizes(n_cams, cams); j.raster = true; j.n_rec = n_records_per_cam; j.rec = records;
    j.thickness = thickness; j.ids_out = line_id_planes; j.iz_out = inv_depth_planes;
    ProjWork w;
    return maps_core(w, 0, j);
}

int l3d_draw_line_maps(int device, uint32_t n_cams, const l3d_image* images, const int32_t* const* line_id_planes, uint32_t n_lines,
                       const uint8_t* colors, uint32_t alpha, uint8_t* const* out_rgb) {
    if (!n_cams) return L3D_OK;
    if (int rc = check_alpha(alpha)) return rc;
    if (int rc = check_images(n_cams, images, nullptr)) return rc;
    if (int rc = check_pointers(n_cams, line_id_planes)) return rc;
    if (int rc = check_pointers(n_cams, out_rgb)) return rc;
    if (int rc = set_device(device)) return rc;
    MapJob j;
    j.n_cams = n_cams; j.size.resize(n_cams);
    for (uint32_t c = 0; c < n_cams; ++c) j.size[c] = {images[c].cols, images[c].rows};
    j.ids_in = line_id_planes; j.images = images; j.colors = n_lines ? colors : nullptr; j.n_lines = n_lines; j.alpha = alpha; j.rgb_out = out_rgb;
    ProjWork w;
    return maps_core(w, 0, j);
}

int l3d_view_camera(l3d_ctx* c, uint32_t camID, l3d_camera* cam) {
    if (!c || !cam) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    auto f = c->views.find(camID);
    if (f == c->views.end()) return fail(L3D_ERR_ARG, "unknown camera ID");
    if (c->state == l3d_ctx::BEGUN || c->aff_shard_open) return fail(L3D_ERR_STATE, "the views are translated while a split call is open");
    *cam = camera_of(*f->second);
    return L3D_OK;
}

int l3d_set_projection_budget(l3d_ctx* c, uint64_t bytes) {  // test hook
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->proj.budget = (size_t)bytes;
    return L3D_OK;
}

int l3d_project_lines(l3d_ctx* c, uint32_t n_cams, const l3d_camera* cams, double near_plane, uint32_t* counts) {
    if (!c || (n_cams && !counts)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_near(near_plane)) return rc;
    if (int rc = check_cameras(n_cams, cams)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    std::vector<uint32_t> cnt;
    if (int rc = project_context_lines(c, n_cams, cams, near_plane, cnt)) return rc;
    for (uint32_t k = 0; k < n_cams; ++k) counts[k] = cnt[k];
    return L3D_OK;
}

int l3d_get_projected_lines(l3d_ctx* c, l3d_projected_segment* out, uint64_t cap, uint64_t* n) {
    if (!c || !n) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    *n = c->proj_records.size();
    if (out && *n) std::memcpy(out, c->proj_records.data(), 32 * (size_t)std::min<uint64_t>(cap, *n));
    return L3D_OK;
}

int l3d_render_lines(l3d_ctx* c, uint32_t n_cams, const l3d_camera* cams, double near_plane, uint32_t thickness,
                     int32_t* const* line_id_planes, float* const* inv_depth_planes) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_near(near_plane)) return rc;
    if (int rc = check_thickness(thickness)) return rc;
    if (int rc = check_cameras(n_cams, cams)) return rc;
    if (int rc = check_pointers(n_cams, line_id_planes)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    std::vector<uint32_t> cnt;
    if (int rc = project_context_lines(c, n_cams, cams, near_plane, cnt)) return rc;
    if (!n_cams) return L3D_OK;
    MapJob j;
    j.n_cams = n_cams; j.size = camera_sizes(n_cams, cams); j.raster = true; j.n_rec = cnt.data(); j.rec = c->proj_records.data();
    j.thickness = thickness; j.ids_out = line_id_planes; j.iz_out = inv_depth_planes;
    return maps_core(c->proj, c->stream, j);
}

int l3d_draw_lines(l3d_ctx* c, uint32_t n_cams, const l3d_camera* cams, const l3d_image* images, double near_plane,
                   uint32_t thickness, uint32_t alpha, const uint8_t* colors, uint8_t* const* out_rgb) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_near(near_plane)) return rc;
    if (int rc = check_thickness(thickness)) return rc;
    if (int rc = check_alpha(alpha)) return rc;
    if (int rc = check_cameras(n_cams, cams)) return rc;
    const std::vector<std::pair<uint32_t, uint32_t>> sizes = camera_sizes(n_cams, cams);
    if (int rc = check_images(n_cams, images, &sizes)) return rc;
    if (int rc = check_pointers(n_cams, out_rgb)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    std::vector<uint32_t> cnt;
    if (int rc = project_context_lines(c, n_cams, cams, near_plane, cnt)) return rc;
    if (!n_cams) return L3D_OK;
    MapJob j;
    j.n_cams = n_cams; j.size = sizes; j.raster = true; j.n_rec = cnt.data(); j.rec = c->proj_records.data(); j.thickness = thickness;
    j.images = images; j.colors = c->lines3D.empty() ? nullptr : colors; j.n_lines = (uint32_t)c->lines3D.size(); j.alpha = alpha;
    j.rgb_out = out_rgb;
    return maps_core(c->proj, c->stream, j);
}

}  // extern "C"
