// l3d_model.hip -- the host plumbing that the stages on a flat model of 3D segments share (project,
// associate, compare, merge), declared in l3d_ctx.h beside ProjWork.  The sizes and the slicing rule are in l3d_model.h,
// the device side that compare and merge share (cmp_slice_range, cmp_stage_chunk, cmp_pair) in l3d_kernels.h.  Behind it
// what the entries on a model, cameras and the cameras' 2D segments share (§27-§29: refine, refit, bundle; §17's context
// entry): the checks of cameras and segments, the path into a stage from a stateless and from a context entry, and the
// way a new model gets back into the context.
#include "l3d_ctx.h"
#include "l3d_refit.h"

namespace l3d {

static_assert(kSliceChunk == kCmpChunk, "slice_plan counts the chunks of cmp_slice_range");

int check_thresholds(double max_distance, double min_cos2, double min_overlap) {
    if (!(max_distance >= 0.0) || !std::isfinite(max_distance)) return fail(L3D_ERR_ARG, "max_distance must be finite and not negative");
    if (!(min_cos2 >= 0.0 && min_cos2 <= 1.0)) return fail(L3D_ERR_ARG, "min_cos2 must lie in [0, 1]");
    if (!(min_overlap >= 0.0 && min_overlap <= 1.0)) return fail(L3D_ERR_ARG, "min_overlap must lie in [0, 1]");
    return L3D_OK;
}

int check_model(const char* side, size_t n, const double* segs, const uint32_t* line) {
    const std::string who = side ? std::string("the ") + side + " side" : std::string("the model");
    if (n >= ((size_t)1 << 30)) return fail(L3D_ERR_LIMIT, who + " has 2^30 or more segments");
    if (n && (!segs || !line)) return fail(L3D_ERR_ARG, "null argument");
    for (size_t i = 0; i < 6 * n; ++i)
        if (!(std::fabs(segs[i]) <= 0x1p100))          // (NaN and the infinities fail it too)
            return fail(L3D_ERR_ARG, (side ? who + ": " : std::string()) + "segment " + std::to_string(i / 6) +
                                         " has a coordinate that is not finite or beyond 2^100");
    return L3D_OK;
}

void context_segments(const l3d_ctx* c, std::vector<double>& P6, std::vector<uint32_t>& line) {
    P6.clear(); line.clear();
    for (size_t i = 0; i < c->lines3D.size(); ++i)
        for (const ReconSeg3D& s : c->lines3D[i].collinear) {
            const double p[6] = {s.P1.x, s.P1.y, s.P1.z, s.P2.x, s.P2.y, s.P2.z};
            P6.insert(P6.end(), p, p + 6);
            line.push_back((uint32_t)i);
        }
}

int lines_ready(const l3d_ctx* c, const char* busy, const char* verb) {
    if (busy && (c->state == l3d_ctx::BEGUN || c->aff_shard_open)) return fail(L3D_ERR_STATE, std::string(busy) + " while a split call is open");
    if (!c->lines_done) return fail(L3D_ERR_STATE, std::string("no 3D lines to ") + verb + ": l3d_reconstruct_3d_lines has not run");
    return L3D_OK;
}

l3d_camera camera_of(const HostView& v) {
    l3d_camera cam;
    std::memcpy(cam.K, v.K.m, 72); std::memcpy(cam.R, v.R.m, 72);
    cam.t[0] = v.t.x; cam.t[1] = v.t.y; cam.t[2] = v.t.z;
    cam.width = v.width; cam.height = v.height;
    return cam;
}

l3d_association no_association() { return l3d_association{-1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, 0.0f, 0u}; }

int check_pose_cameras(uint32_t n_cams, const l3d_camera* cams, double near_plane, bool no_skew) {
    if (int rc = check_projection_cameras(n_cams, cams, near_plane)) return rc;
    for (uint32_t c = 0; c < n_cams; ++c) {
        const double* K = cams[c].K;
        if (!(K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0))
            return fail(L3D_ERR_ARG, "camera " + std::to_string(c) + ": K must be upper triangular with K22 = 1 and K00, K11 not 0");
        if (no_skew && K[1] != 0.0) return fail(L3D_ERR_ARG, "camera " + std::to_string(c) + ": K01 must be 0 (no skew)");
    }
    return L3D_OK;
}

int check_camera_segments(uint32_t n_cams, const uint32_t* n_seg, const float* const* seg, uint64_t& n_total) {
    n_total = 0;
    for (uint32_t k = 0; k < n_cams; ++k) n_total += n_seg[k];
    if (n_total >= ((uint64_t)1 << 32)) return fail(L3D_ERR_LIMIT, "2^32 or more segments in total");
    for (uint32_t k = 0; k < n_cams; ++k) {
        if (n_seg[k] && !seg[k]) return fail(L3D_ERR_ARG, "null argument");
        for (size_t i = 0; i < 4 * (size_t)n_seg[k]; ++i)
            if (!std::isfinite(seg[k][i]))
                return fail(L3D_ERR_ARG, "camera " + std::to_string(k) + ": segment " + std::to_string(i / 4) + " has a non-finite entry");
    }
    return L3D_OK;
}

int camera_segments(uint32_t n_cams, const l3d_camera* cams, const uint32_t* n_segments_per_cam, const float* segs4,
                    std::vector<const float*>& seg) {
    if (n_cams && (!cams || !n_segments_per_cam)) return fail(L3D_ERR_ARG, "null argument");
    uint64_t n_seg = 0;
    for (uint32_t k = 0; k < n_cams; ++k) n_seg += n_segments_per_cam[k];
    if (n_seg && !segs4) return fail(L3D_ERR_ARG, "null argument");
    seg.resize(n_cams);
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_cams; ++k) { seg[k] = segs4 ? segs4 + 4 * at : nullptr; at += n_segments_per_cam[k]; }
    return L3D_OK;
}

int context_views(const l3d_ctx* c, uint32_t n_views, const uint32_t* camIDs, const l3d_camera* cams_in, ContextViews& V) {
    std::vector<uint32_t> sorted(camIDs, camIDs + n_views);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(L3D_ERR_ARG, "a camera ID is named twice");
    V.cams.resize(n_views); V.m.resize(n_views); V.seg.resize(n_views);
    for (uint32_t k = 0; k < n_views; ++k) {
        auto f = c->views.find(camIDs[k]);
        if (f == c->views.end()) return fail(L3D_ERR_ARG, "unknown camera ID");
        V.cams[k] = cams_in ? cams_in[k] : camera_of(*f->second);
        V.m[k] = f->second->M; V.seg[k] = f->second->segs.data();
    }
    return L3D_OK;
}

int context_job(const l3d_ctx* c, uint32_t n_views, const uint32_t* camIDs, const l3d_camera* cams_in, ContextViews& V, RefitJob& J) {
    if (int rc = context_views(c, n_views, camIDs, cams_in, V)) return rc;
    context_segments(c, V.P6, V.line);
    if (int rc = check_model("context's", V.line.size(), V.P6.data(), V.line.data())) return rc;
    J = RefitJob{(uint32_t)V.line.size(), V.P6.data(), V.line.data(), n_views, V.cams.data(), V.m.data(), V.seg.data()};
    return L3D_OK;
}

bool context_take_lines(l3d_ctx* c, const uint32_t* camIDs, const RefitModel& R, const std::vector<NewLine>& anew) {
    auto seg3 = [](const double* a, const double* b) {
        const d3 P1{a[0], a[1], a[2]}, P2{b[0], b[1], b[2]};
        ReconSeg3D s = segment3d(P1, P2);
        s.P1 = P1; s.P2 = P2;
        return s;
    };
    for (const NewLine& nl : anew) {
        const uint32_t l = nl.line;
        ReconLine& L = c->lines3D[l];
        L.collinear.clear();
        for (uint32_t k = R.seg_off[l]; k < R.seg_off[l + 1]; ++k) L.collinear.push_back(seg3(&R.segs[6 * (size_t)k], &R.segs[6 * (size_t)k + 3]));
        L.cluster_seg = seg3(nl.P1, nl.P2);
        L.residuals.clear();
        for (uint32_t r = R.obs_off[l]; r < R.obs_off[l + 1]; ++r) L.residuals.emplace_back(camIDs[R.obs[r].camera], R.obs[r].segment);
    }
    if (!anew.empty()) c->proj_records.clear();
    return !anew.empty();
}

KernelTimer::KernelTimer(float* into) : into_(into) {
    if (!into_) return;
    *into_ = 0.0f;
    if (hipEventCreate(&ev_[0]) == hipSuccess) (void)hipEventCreate(&ev_[1]);   // (ok() tells)
}
KernelTimer::~KernelTimer() { for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e); }

}  // namespace l3d
