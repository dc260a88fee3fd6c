// l3d_directions.hip -- the directions the 3D lines run in (kernels: k_directions.hip): the stateless
// l3d_direction_segments on a caller's model, l3d_direction_lines on the context's lines, which it leaves untouched, and the
// handle that holds the result.
//
// Stage 0, the integer weights, is host code (pl_weights of l3d_planes.h).  Stage 1: k_dir_units turns every segment into a
// unit direction.  Stage 2: k_dir_score and k_pl_merge score every direction against every segment.  The host downloads 16
// bytes of score per hypothesis -- never the unit records -- and runs stage 3, the selection (l3d_directions.h).
#include <atomic>
#include <cstdio>
#include <memory>

#include "l3d_ctx.h"
#include "l3d_directions.h"

namespace l3d {
// test hooks (l3d_debug_counter): launches of k_dir_score so far; the slices and the hypotheses of the last call; the time
// of the three kernels in the last timed call (context at timing level 2)
std::atomic<uint64_t> g_dir_score_launches{0}, g_dir_slices{0}, g_dir_hypotheses{0}, g_dir_kernel_ns{0};
}  // namespace l3d

using namespace l3d;

struct l3d_directions { DirResult r; };

namespace {

constexpr size_t kDirCellBudget = (size_t)256 << 20;       // the cells stay within this
static_assert(sizeof(l3d_dir_score) == sizeof(PlCell), "the device's cells are the selection's scores");

int check_params(const l3d_directions_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (!(p->max_sin2 >= 0.0 && p->max_sin2 <= 1.0)) return fail(L3D_ERR_ARG, "max_sin2 must lie in [0, 1]");
    if (!(p->min_length >= 0.0) || !std::isfinite(p->min_length)) return fail(L3D_ERR_ARG, "min_length must be finite and not negative");
    if (!(p->max_frame_cos2 >= 0.0 && p->max_frame_cos2 <= 1.0)) return fail(L3D_ERR_ARG, "max_frame_cos2 must lie in [0, 1]");
    if (!p->min_segments) return fail(L3D_ERR_ARG, "min_segments must be at least 1");
    if (!p->max_directions) return fail(L3D_ERR_ARG, "max_directions must be at least 1");
    if (!p->max_tests) return fail(L3D_ERR_ARG, "max_tests must be at least 1");
    if (p->frame_search < 1 || p->frame_search > 64) return fail(L3D_ERR_ARG, "frame_search must lie in 1 .. 64");
    for (uint32_t r : p->reserved)
        if (r != 0) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

// n > 0, arguments checked.  kernel_ms (may be null): the three kernels.
int detect(ProjWork& w, hipStream_t st, uint32_t n, const double* segs, const uint32_t* line, const l3d_directions_params& p,
           DirResult& out, float* kernel_ms) {
    PlWeights wt;
    pl_weights(n, segs, wt);
    g_dir_hypotheses.store(n, std::memory_order_relaxed);
    const SlicePlan plan = slice_plan(n, n, p.slice_chunks, sizeof(PlCell), kDirCellBudget);
    const size_t b_seg = 48 * (size_t)n, b_w = 8 * (size_t)n, b_unit = sizeof(DirUnit) * (size_t)n, b_score = sizeof(PlCell) * (size_t)n,
                 b_cells = b_score * plan.n_slices;
    Layout lay;
    const size_t o_seg = lay.take(b_seg), o_w = lay.take(b_w), in_bytes = lay.at, o_score = lay.take(b_score), o_unit = lay.take(b_unit),
                 o_cells = lay.take(b_cells);
    if (w.d.reserve(lay.at) != hipSuccess || w.h.reserve(std::max(in_bytes, b_score)) != hipSuccess)
        return fail(L3D_ERR_HIP, "directions: allocation failed");
    char* d = w.d.p;
    std::memcpy(w.h.p + o_seg, segs, b_seg);
    unsigned long long* up = (unsigned long long*)(w.h.p + o_w);
    for (uint32_t i = 0; i < n; ++i) up[i] = wt.live[i] ? wt.q[i] | kPlLiveBit : 0ull;
    KernelTimer timer(kernel_ms);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "directions: no event");
    DirArgs a{(const double*)(d + o_seg), n, (const unsigned long long*)(d + o_w), plan.slice_chunks, plan.n_slices, p.max_sin2,
              (DirUnit*)(d + o_unit), (PlCell*)(d + o_cells), (PlCell*)(d + o_score)};
    hipError_t e = hipMemcpyAsync(d, w.h.p, in_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = timer.start(st);
    if (e == hipSuccess) e = launch_dir_units(a, st);
    if (e == hipSuccess) e = launch_dir_score(a, st);
    if (e == hipSuccess) e = launch_pl_merge(a.cells, a.scores, n, plan.n_slices, st);
    if (e == hipSuccess) e = timer.stop(st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);     // (the model has left w.h)
    if (e == hipSuccess) e = hipMemcpyAsync(w.h.p, d + o_score, b_score, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("directions: ") + hipGetErrorString(e));
    timer.add();
    g_dir_score_launches.fetch_add(1, std::memory_order_relaxed);
    g_dir_slices.store(plan.n_slices, std::memory_order_relaxed);
    size_t bad = 0;
    if (dir_select(n, segs, line, p, wt, (const l3d_dir_score*)w.h.p, out, &bad))
        return fail(L3D_ERR_HIP, "directions: the members of hypothesis " + std::to_string(bad) + " recomputed on the host differ from the device's score");
    return L3D_OK;
}

}  // namespace

extern "C" {

int l3d_direction_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_directions_params* params,
                           l3d_directions** out) {
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_model(nullptr, n, segs6, line)) return rc;
    auto dr = std::make_unique<l3d_directions>();
    if (n) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        if (int rc = detect(w, 0, n, segs6, line, *params, dr->r, nullptr)) return rc;
    }
    *out = dr.release();
    return L3D_OK;
}

int l3d_direction_lines(l3d_ctx* c, const l3d_directions_params* params, l3d_directions** out) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "directions are detected", "group into directions")) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (int rc = check_model(nullptr, line.size(), P6.data(), line.data())) return rc;
    const uint32_t n = (uint32_t)line.size();
    auto dr = std::make_unique<l3d_directions>();
    if (n) {
        if (int rc = set_device(c->device)) return rc;
        float ms = 0.0f;
        const bool timed = c->timing_level >= 2;
        if (int rc = detect(c->proj, c->stream, n, P6.data(), line.data(), *params, dr->r, timed ? &ms : nullptr)) return rc;
        if (timed) g_dir_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
    }
    *out = dr.release();
    return L3D_OK;
}

int l3d_directions_counts(const l3d_directions* dr, uint64_t* n_directions, uint64_t* n_memberships, uint64_t* n_hypotheses) {
    if (!dr) return fail(L3D_ERR_ARG, "null argument");
    if (n_directions) *n_directions = dr->r.directions.size();
    if (n_memberships) *n_memberships = dr->r.members.size();
    if (n_hypotheses) *n_hypotheses = dr->r.scores.size();
    return L3D_OK;
}

int l3d_directions_get(const l3d_directions* dr, l3d_dir_direction* directions, l3d_dir_member* members, uint32_t* seg_directions,
                       l3d_dir_score* scores, l3d_directions_summary* summary) {
    if (!dr) return fail(L3D_ERR_ARG, "null argument");
    const DirResult& r = dr->r;
    if (directions && !r.directions.empty()) std::memcpy(directions, r.directions.data(), sizeof(l3d_dir_direction) * r.directions.size());
    if (members && !r.members.empty()) std::memcpy(members, r.members.data(), sizeof(l3d_dir_member) * r.members.size());
    if (seg_directions && !r.seg_directions.empty()) std::memcpy(seg_directions, r.seg_directions.data(), sizeof(uint32_t) * r.seg_directions.size());
    if (scores && !r.scores.empty()) std::memcpy(scores, r.scores.data(), sizeof(l3d_dir_score) * r.scores.size());
    if (summary) *summary = r.sum;
    return L3D_OK;
}

int l3d_directions_save_obj(const l3d_directions* dr, const char* path) {
    if (!dr || !path) return fail(L3D_ERR_ARG, "null argument");
    FILE* f = std::fopen(path, "w");
    if (!f) return fail(L3D_ERR_IO, std::string("cannot write ") + path);
    unsigned long long v = 1;
    for (const l3d_dir_direction& p : dr->r.directions) {
        for (const double t : {p.t_min, p.t_max})
            std::fprintf(f, "v %.17g %.17g %.17g\n", p.centroid[0] + t * p.D_fit[0], p.centroid[1] + t * p.D_fit[1], p.centroid[2] + t * p.D_fit[2]);
        std::fprintf(f, "l %llu %llu\n", v, v + 1);
        v += 2;
    }
    const bool bad = std::ferror(f) != 0;
    if (std::fclose(f) != 0 || bad) return fail(L3D_ERR_IO, std::string("cannot write ") + path);
    return L3D_OK;
}

void l3d_directions_close(l3d_directions* dr) { delete dr; }

}  // extern "C"
