// l3d_planes.hip -- the planes the 3D lines lie in (kernels: k_planes.hip): the stateless l3d_plane_segments on
// a caller's model, l3d_plane_lines on the context's lines, which it leaves untouched, and the handle that holds the
// result.
//
// Stage 0, the integer weights, is host code (l3d_planes.h).  Stage 1: the junctions of §24 are found by wf_junctions
// (l3d_wireframe.hip) and stay on the device, where k_pl_hypotheses turns each into a plane.  Stage 2: k_pl_score and
// k_pl_merge score every plane against every segment.  The host downloads 64 bytes of plane and 16 bytes of score per
// hypothesis and runs stage 3, the selection (l3d_planes.h).
#include <atomic>
#include <cstdio>
#include <memory>

#include "l3d_ctx.h"
#include "l3d_planes.h"
#include "l3d_wireframe.h"

namespace l3d {
// test hooks (l3d_debug_counter): launches of k_pl_score so far; the slices and the hypotheses of the last call; the time
// of the three plane kernels and that of the junction passes in the last timed call (context at timing level 2)
std::atomic<uint64_t> g_pl_score_launches{0}, g_pl_slices{0}, g_pl_hypotheses{0}, g_pl_kernel_ns{0}, g_pl_junction_ns{0};
}  // namespace l3d

using namespace l3d;

struct l3d_planes { PlResult r; };

namespace {

constexpr size_t kPlCellBudget = (size_t)256 << 20;        // the cells stay within this
static_assert(sizeof(PlHyp) == sizeof(PlHypothesis) && sizeof(l3d_pl_score) == sizeof(PlCell), "the device's records are the selection's");

int check_params(const l3d_planes_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (!(p->max_distance >= 0.0) || !std::isfinite(p->max_distance)) return fail(L3D_ERR_ARG, "max_distance must be finite and not negative");
    if (!(p->junction_distance >= 0.0) || !std::isfinite(p->junction_distance)) return fail(L3D_ERR_ARG, "junction_distance must be finite and not negative");
    if (!(p->junction_extension >= 0.0) || !std::isfinite(p->junction_extension)) return fail(L3D_ERR_ARG, "junction_extension must be finite and not negative");
    if (!(p->min_sin2 >= 0.0 && p->min_sin2 <= 1.0)) return fail(L3D_ERR_ARG, "min_sin2 must lie in [0, 1]");
    if (!(p->min_length >= 0.0) || !std::isfinite(p->min_length)) return fail(L3D_ERR_ARG, "min_length must be finite and not negative");
    if (!p->min_segments) return fail(L3D_ERR_ARG, "min_segments must be at least 1");
    if (!p->max_planes) return fail(L3D_ERR_ARG, "max_planes must be at least 1");
    if (!p->max_tests) return fail(L3D_ERR_ARG, "max_tests must be at least 1");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

// n > 0, arguments checked.  kernel_ms (may be null): [0], [1] the junction passes, [2] the plane kernels.
int detect(ProjWork& w, hipStream_t st, uint32_t n, const double* segs, const uint32_t* line, const l3d_planes_params& p,
           PlResult& out, float* kernel_ms) {
    PlWeights wt;
    pl_weights(n, segs, wt);
    const l3d_wireframe_params jp{p.junction_distance, p.junction_extension, p.min_sin2, p.slice_chunks, 0u};
    WfOnDevice list{kPlMaxHypotheses, "more than 2^24 plane hypotheses: lower junction_distance", nullptr, nullptr, nullptr, 0};
    std::vector<WfRecord> none;
    if (int rc = wf_junctions(w, st, n, segs, line, jp, none, kernel_ms, &list)) return rc;
    const size_t n_h = list.n_junctions;
    g_pl_hypotheses.store(n_h, std::memory_order_relaxed);
    std::vector<PlHyp> hyp(n_h);
    std::vector<l3d_pl_score> score(n_h);
    if (n_h) {                                             // (no junction: no score launch)
        const SlicePlan plan = slice_plan((uint32_t)n_h, n, p.slice_chunks, sizeof(PlCell), kPlCellBudget);
        const size_t b_w = 8 * (size_t)n, b_hyp = sizeof(PlHypothesis) * n_h, b_score = sizeof(PlCell) * n_h, b_cells = b_score * plan.n_slices;
        Layout lay;
        const size_t o_hyp = lay.take(b_hyp), o_score = lay.take(b_score), down_bytes = lay.at, o_w = lay.take(b_w), o_cells = lay.take(b_cells);
        DevBuf<char> d;                                    // (w's buffers hold the model and the junctions)
        PinnedBuf<char> h;
        if (d.reserve(lay.at) != hipSuccess || h.reserve(std::max(down_bytes, b_w)) != hipSuccess) return fail(L3D_ERR_HIP, "planes: allocation failed");
        unsigned long long* up = (unsigned long long*)h.p;
        for (uint32_t i = 0; i < n; ++i) up[i] = wt.live[i] ? wt.q[i] | kPlLiveBit : 0ull;
        KernelTimer timer(kernel_ms ? kernel_ms + 2 : nullptr);
        if (!timer.ok()) return fail(L3D_ERR_HIP, "planes: no event");
        PlArgs a{list.segs, n, (const unsigned long long*)(d.p + o_w), list.junctions, (uint32_t)n_h, plan.slice_chunks, plan.n_slices,
                 p.max_distance, (PlHypothesis*)(d.p + o_hyp), (PlCell*)(d.p + o_cells), (PlCell*)(d.p + o_score)};
        hipError_t e = hipMemcpyAsync(d.p + o_w, h.p, b_w, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = timer.start(st);
        if (e == hipSuccess) e = launch_pl_hypotheses(a, st);
        if (e == hipSuccess) e = launch_pl_score(a, st);
        if (e == hipSuccess) e = launch_pl_merge(a.cells, a.scores, a.n_h, a.n_slices, st);
        if (e == hipSuccess) e = timer.stop(st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);     // (the weights have left h)
        if (e == hipSuccess) e = hipMemcpyAsync(h.p, d.p, down_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("planes: ") + hipGetErrorString(e));
        timer.add();
        g_pl_score_launches.fetch_add(1, std::memory_order_relaxed);
        g_pl_slices.store(plan.n_slices, std::memory_order_relaxed);
        std::memcpy(hyp.data(), h.p + o_hyp, b_hyp);
        std::memcpy(score.data(), h.p + o_score, b_score);
    }
    size_t bad = 0;
    if (pl_select(n, segs, line, p, wt, hyp.data(), score.data(), n_h, out, &bad))
        return fail(L3D_ERR_HIP, "planes: the members of hypothesis " + std::to_string(bad) + " recomputed on the host differ from the device's score");
    return L3D_OK;
}

}  // namespace

extern "C" {

int l3d_plane_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_planes_params* params,
                       l3d_planes** out) {
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_model(nullptr, n, segs6, line)) return rc;
    auto pl = std::make_unique<l3d_planes>();
    if (n) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        if (int rc = detect(w, 0, n, segs6, line, *params, pl->r, nullptr)) return rc;
    }
    *out = pl.release();
    return L3D_OK;
}

int l3d_plane_lines(l3d_ctx* c, const l3d_planes_params* params, l3d_planes** out) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "planes are detected", "group into planes")) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (int rc = check_model(nullptr, line.size(), P6.data(), line.data())) return rc;
    const uint32_t n = (uint32_t)line.size();
    auto pl = std::make_unique<l3d_planes>();
    if (n) {
        if (int rc = set_device(c->device)) return rc;
        float ms[3] = {0.0f, 0.0f, 0.0f};
        const bool timed = c->timing_level >= 2;
        if (int rc = detect(c->proj, c->stream, n, P6.data(), line.data(), *params, pl->r, timed ? ms : nullptr)) return rc;
        if (timed) {
            g_pl_junction_ns.store((uint64_t)(((double)ms[0] + (double)ms[1]) * 1e6), std::memory_order_relaxed);
            g_pl_kernel_ns.store((uint64_t)((double)ms[2] * 1e6), std::memory_order_relaxed);
        }
    }
    *out = pl.release();
    return L3D_OK;
}

int l3d_planes_counts(const l3d_planes* pl, uint64_t* n_planes, uint64_t* n_memberships, uint64_t* n_hypotheses) {
    if (!pl) return fail(L3D_ERR_ARG, "null argument");
    if (n_planes) *n_planes = pl->r.planes.size();
    if (n_memberships) *n_memberships = pl->r.members.size();
    if (n_hypotheses) *n_hypotheses = pl->r.scores.size();
    return L3D_OK;
}

int l3d_planes_get(const l3d_planes* pl, l3d_pl_plane* planes, l3d_pl_member* members, uint32_t* seg_planes, l3d_pl_score* scores,
                   l3d_planes_summary* summary) {
    if (!pl) return fail(L3D_ERR_ARG, "null argument");
    const PlResult& r = pl->r;
    if (planes && !r.planes.empty()) std::memcpy(planes, r.planes.data(), sizeof(l3d_pl_plane) * r.planes.size());
    if (members && !r.members.empty()) std::memcpy(members, r.members.data(), sizeof(l3d_pl_member) * r.members.size());
    if (seg_planes && !r.seg_planes.empty()) std::memcpy(seg_planes, r.seg_planes.data(), sizeof(uint32_t) * r.seg_planes.size());
    if (scores && !r.scores.empty()) std::memcpy(scores, r.scores.data(), sizeof(l3d_pl_score) * r.scores.size());
    if (summary) *summary = r.sum;
    return L3D_OK;
}

int l3d_planes_save_obj(const l3d_planes* pl, const char* path) {
    if (!pl || !path) return fail(L3D_ERR_ARG, "null argument");
    FILE* f = std::fopen(path, "w");
    if (!f) return fail(L3D_ERR_IO, std::string("cannot write ") + path);
    unsigned long long v = 1;
    for (const l3d_pl_plane& p : pl->r.planes) {
        for (int k = 0; k < 4; ++k) std::fprintf(f, "v %.17g %.17g %.17g\n", p.corners[k][0], p.corners[k][1], p.corners[k][2]);
        std::fprintf(f, "f %llu %llu %llu %llu\n", v, v + 1, v + 2, v + 3);
        v += 4;
    }
    const bool bad = std::ferror(f) != 0;
    if (std::fclose(f) != 0 || bad) return fail(L3D_ERR_IO, std::string("cannot write ") + path);
    return L3D_OK;
}

void l3d_planes_close(l3d_planes* pl) { delete pl; }

}  // extern "C"
