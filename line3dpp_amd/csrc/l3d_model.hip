// l3d_model.hip -- the host plumbing that the stages on a flat model of 3D segments share (project,
// associate, compare, merge), declared in l3d_ctx.h beside ProjWork.  The sizes and the slicing rule are in l3d_model.h,
// the device side that compare and merge share (cmp_slice_range, cmp_stage_chunk, cmp_pair) in l3d_kernels.h.
#include "l3d_ctx.h"

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

KernelTimer::KernelTimer(float* into) : into_(into) {
    if (!into_) return;
    *into_ = 0.0f;
    if (hipEventCreate(&ev_[0]) == hipSuccess) (void)hipEventCreate(&ev_[1]);   // (ok() tells)
}
KernelTimer::~KernelTimer() { for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e); }

}  // namespace l3d
