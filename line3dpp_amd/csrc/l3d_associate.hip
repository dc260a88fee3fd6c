// l3d_associate.hip -- host side of the association of 2D segments with the projected 3D lines (kernel:
// k_associate.hip): the stateless l3d_associate_segments on a caller's records and segments, and
// l3d_associate_view_segments on the context's lines and the added views' own segments, on the context's stream and the
// work space of the projection stages.
//
// Cameras are taken in GROUPS under the budget of the projection stages (l3d_set_projection_budget makes the groups
// small): 32 bytes per record, 16 + 24 per segment.  Every segment's result is computed from its own camera's records,
// so the grouping changes nothing but the number of launches.  One packed upload and one download per group, both
// through pinned staging; the kernel hands out the squared distance and the root is taken here, after the download, by
// the host's correctly rounded sqrtf.
#include <atomic>

#include "l3d_ctx.h"

namespace l3d {
std::atomic<uint64_t> g_assoc_launches{0};      // test hooks (l3d_debug_counter): launches of k_associate so far ...
std::atomic<uint64_t> g_assoc_kernel_ns{0};     // ... and the kernel time of the last timed call (context at timing level 2)
}  // namespace l3d

using namespace l3d;

namespace {

constexpr uint32_t kAssocMaxGroup = 4096;       // cameras per group at most
static_assert(sizeof(AssocOut) == sizeof(l3d_association) && sizeof(AssocOut) == 24, "association layout");
static_assert(sizeof(ProjRecord) == sizeof(l3d_projected_segment), "record layout");
static_assert(kAssocSegmentMask == L3D_PROJ_SEGMENT_MASK, "segment mask");

int check_params(const l3d_associate_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    return check_thresholds(p->max_distance, p->min_cos2, p->min_overlap);
}

// Arguments already checked.  n_rec[c] records of camera c in rec, camera after camera; seg[c] = its n_seg[c] segments;
// out: one association per segment, camera after camera.  kernel_ms (may be null): the time of every launch, summed.
int associate_core(ProjWork& w, hipStream_t st, uint32_t n_cams, const uint32_t* n_rec, const l3d_projected_segment* rec,
                   const uint32_t* n_seg, const float* const* seg, const l3d_associate_params& p, l3d_association* out,
                   float* kernel_ms) {
    KernelTimer timer(kernel_ms);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "association: no event");
    int rc = L3D_OK;
    uint64_t rec_at = 0, seg_at = 0;
    std::vector<AssocCam> cams;
    for (uint32_t c0 = 0; c0 < n_cams && rc == L3D_OK;) {
        // the group: cameras while their records, segments and results fit the budget (one at least)
        uint32_t c1 = c0;
        uint64_t g_rec = 0, g_seg = 0, g_tiles = 0;
        cams.clear();
        while (c1 < n_cams && c1 - c0 < kAssocMaxGroup) {
            const uint64_t tiles = ((uint64_t)n_seg[c1] + kAssocTile - 1) / kAssocTile;
            if (c1 > c0 && (32 * (g_rec + n_rec[c1]) + 40 * (g_seg + n_seg[c1]) > projection_budget(w) ||
                            g_rec + n_rec[c1] >= ((uint64_t)1 << 32) || g_tiles + tiles >= ((uint64_t)1 << 31)))
                break;
            cams.push_back(AssocCam{(uint32_t)g_tiles, (uint32_t)g_seg, n_seg[c1], (uint32_t)g_rec, n_rec[c1]});
            g_rec += n_rec[c1]; g_seg += n_seg[c1]; g_tiles += tiles;
            ++c1;
        }
        const uint32_t g = c1 - c0;
        if (g_seg) {
            const size_t b_cam = sizeof(AssocCam) * g, b_rec = 32 * (size_t)g_rec, b_seg = 16 * (size_t)g_seg, b_out = 24 * (size_t)g_seg;
            Layout lay;
            const size_t o_cam = lay.take(b_cam), o_rec = lay.take(b_rec), o_seg = lay.take(b_seg), in_bytes = lay.at;
            const size_t o_out = lay.take(b_out), total = lay.at;
            if (w.h.reserve(total) != hipSuccess || w.d.reserve(total) != hipSuccess) { rc = fail(L3D_ERR_HIP, "association: allocation failed"); break; }
            char* h = w.h.p; char* d = w.d.p;
            std::memcpy(h + o_cam, cams.data(), b_cam);
            if (b_rec) std::memcpy(h + o_rec, rec + rec_at, b_rec);
            for (uint32_t c = 0; c < g; ++c)
                if (n_seg[c0 + c]) std::memcpy(h + o_seg + 16 * (size_t)cams[c].seg0, seg[c0 + c], 16 * (size_t)n_seg[c0 + c]);
            AssocArgs a{(const AssocCam*)(d + o_cam), g, (const float4*)(d + o_seg), (const ProjRecord*)(d + o_rec), (AssocOut*)(d + o_out),
                        p.max_distance * p.max_distance, p.min_cos2, p.min_overlap};
            hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = timer.start(st);
            if (e == hipSuccess) e = launch_associate(a, (uint32_t)g_tiles, st);
            if (e == hipSuccess) e = timer.stop(st);
            if (e == hipSuccess) e = hipMemcpyAsync(h + o_out, d + o_out, b_out, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { rc = fail(L3D_ERR_HIP, std::string("association: ") + hipGetErrorString(e)); break; }
            g_assoc_launches.fetch_add(1, std::memory_order_relaxed);
            timer.add();
            const AssocOut* res = (const AssocOut*)(h + o_out);
            for (size_t i = 0; i < (size_t)g_seg; ++i) {
                const AssocOut& r = res[i];
                out[seg_at + i] = l3d_association{r.record, r.line, r.segment, std::sqrt(r.d2), r.overlap, r.n_accepted};
            }
        }
        rec_at += g_rec; seg_at += g_seg;
        c0 = c1;
    }
    return rc;
}

}  // namespace

extern "C" {

int l3d_associate_segments(int device, uint32_t n_cams, const uint32_t* n_records_per_cam, const l3d_projected_segment* records,
                           const uint32_t* n_segments_per_cam, const float* segs4, const l3d_associate_params* params,
                           l3d_association* out) {
    if (int rc = check_params(params)) return rc;
    if (!n_cams) return L3D_OK;
    if (!n_records_per_cam || !n_segments_per_cam) return fail(L3D_ERR_ARG, "null argument");
    uint64_t n_rec = 0, n_seg = 0;
    for (uint32_t c = 0; c < n_cams; ++c) {
        if (n_records_per_cam[c] >= 0x80000000u) return fail(L3D_ERR_LIMIT, "camera " + std::to_string(c) + " has 2^31 or more records");
        n_rec += n_records_per_cam[c]; n_seg += n_segments_per_cam[c];
    }
    if (n_seg >= ((uint64_t)1 << 32)) return fail(L3D_ERR_LIMIT, "2^32 or more segments in total");
    if ((n_rec && !records) || (n_seg && (!segs4 || !out))) return fail(L3D_ERR_ARG, "null argument");
    std::vector<const float*> seg(n_cams);
    uint64_t r_at = 0, s_at = 0;
    for (uint32_t c = 0; c < n_cams; ++c) {
        for (uint32_t i = 0; i < n_records_per_cam[c]; ++i) {
            const l3d_projected_segment& r = records[r_at + i];
            if (!(std::isfinite(r.x1) && std::isfinite(r.y1) && std::isfinite(r.x2) && std::isfinite(r.y2)))
                return fail(L3D_ERR_ARG, "camera " + std::to_string(c) + ": record " + std::to_string(i) + " has a non-finite entry");
        }
        seg[c] = segs4 + 4 * s_at;
        for (uint32_t i = 0; i < n_segments_per_cam[c]; ++i)
            for (int k = 0; k < 4; ++k)
                if (!std::isfinite(seg[c][4 * (size_t)i + k]))
                    return fail(L3D_ERR_ARG, "camera " + std::to_string(c) + ": segment " + std::to_string(i) + " has a non-finite entry");
        r_at += n_records_per_cam[c]; s_at += n_segments_per_cam[c];
    }
    if (!n_seg) return L3D_OK;
    if (int rc = set_device(device)) return rc;
    ProjWork w;
    return associate_core(w, 0, n_cams, n_records_per_cam, records, n_segments_per_cam, seg.data(), *params, out, nullptr);
}

int l3d_associate_view_segments(l3d_ctx* c, uint32_t n_views, const uint32_t* camIDs, const l3d_associate_params* params,
                                double near_plane, uint64_t* offsets, l3d_association* out, uint32_t* support_segments,
                                uint32_t* support_views) {
    if (!c || !offsets || (n_views && !camIDs)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    if (!(near_plane > 0.0) || !std::isfinite(near_plane)) return fail(L3D_ERR_ARG, "the near plane must be positive and finite");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "segments are associated", "associate with")) return rc;
    ContextViews V;
    if (int rc = context_views(c, n_views, camIDs, nullptr, V)) return rc;
    uint64_t n_seg = 0;
    if (int rc = check_camera_segments(n_views, V.m.data(), V.seg.data(), n_seg)) return rc;
    const std::vector<uint32_t>& m = V.m;
    if (!out) {                                     // the sizes only
        offsets[0] = 0;
        for (uint32_t k = 0; k < n_views; ++k) offsets[k + 1] = offsets[k] + m[k];
        return L3D_OK;
    }
    std::vector<uint32_t> n_rec;
    if (int rc = project_context_lines(c, n_views, V.cams.data(), near_plane, n_rec)) return rc;
    for (uint32_t k = 0; k < n_views; ++k)
        if (n_rec[k] >= 0x80000000u) return fail(L3D_ERR_LIMIT, "camera " + std::to_string(k) + " has 2^31 or more records");
    std::vector<l3d_association> res(n_seg);
    float ms = 0.0f;
    if (n_seg)
        if (int rc = associate_core(c->proj, c->stream, n_views, n_rec.data(), c->proj_records.data(), m.data(), V.seg.data(), *params,
                                    res.data(), c->timing_level >= 2 ? &ms : nullptr))
            return rc;
    if (c->timing_level >= 2) g_assoc_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
    offsets[0] = 0;
    for (uint32_t k = 0; k < n_views; ++k) offsets[k + 1] = offsets[k] + m[k];
    if (n_seg) std::memcpy(out, res.data(), sizeof(l3d_association) * (size_t)n_seg);
    // per 3D line: the assigned (view, segment) pairs, and the distinct views among them (the views come one after another)
    const size_t n_lines = c->lines3D.size();
    if (support_segments) std::fill(support_segments, support_segments + n_lines, 0u);
    if (support_views) std::fill(support_views, support_views + n_lines, 0u);
    if (support_segments || support_views) {
        std::vector<uint32_t> last_view(n_lines, 0xFFFFFFFFu);
        for (uint32_t k = 0; k < n_views; ++k)
            for (uint64_t i = offsets[k]; i < offsets[k + 1]; ++i) {
                const l3d_association& r = res[i];
                if (r.record < 0 || r.line >= n_lines) continue;
                if (support_segments) ++support_segments[r.line];
                if (support_views && last_view[r.line] != k) { last_view[r.line] = k; ++support_views[r.line]; }
            }
    }
    return L3D_OK;
}

}  // extern "C"
