// l3d_align.hip -- host side of the alignment of two 3D line models (kernels: k_align.hip and, unchanged,
// k_compare.hip): the stateless l3d_align_segments, l3d_align_lines with the context's lines as the moved side, on the
// context's stream and the work space of the projection stages, and the host-only l3d_transform_segments.
//
// One packed upload carries both models.  Per iteration: k_align_transform writes the moved queries, launch_compare (and
// launch_compare_merge where the references are sliced) matches them, k_align_normal sums the normal equations per tile
// of 256 queries; 37 doubles per tile come down, the host adds them in ascending tile order, solves the 7 x 7 system by
// a plain Cholesky factorisation and updates the transform.  The delivery pass repeats the first three steps with the
// final transform at max_distance and brings the records down.  Everything the host computes is fp64 in the order
// DESIGN §23 writes it, so that tests/align_model.py reproduces a whole run bit for bit.
#include <atomic>

#include "l3d_ctx.h"

namespace l3d {
// test hooks (l3d_debug_counter): iterations run and launches of k_align_normal so far, and the kernel time of the last
// timed call (context at timing level 2)
std::atomic<uint64_t> g_aln_iterations{0}, g_aln_normal_launches{0}, g_aln_kernel_ns{0};
}  // namespace l3d

using namespace l3d;

namespace {

constexpr size_t kAlnPartialBudget = (size_t)256 << 20;   // the partials of a comparison stay within this, as in l3d_compare.hip
static_assert(sizeof(l3d_similarity) == 64 && sizeof(l3d_align_params) == 64 && sizeof(l3d_align_summary) == 64 &&
              sizeof(l3d_align_iteration) == 432, "alignment structs");

int check_params(const l3d_align_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thresholds(p->max_distance, p->min_cos2, p->min_overlap)) return rc;
    if (!(p->start_distance == 0.0 || (std::isfinite(p->start_distance) && p->start_distance >= p->max_distance)))
        return fail(L3D_ERR_ARG, "start_distance must be 0, or finite and not below max_distance");
    if (!(p->step_tolerance > 0.0) || !std::isfinite(p->step_tolerance)) return fail(L3D_ERR_ARG, "step_tolerance must be finite and greater than 0");
    if (p->max_iterations < 1 || p->max_iterations > 256) return fail(L3D_ERR_ARG, "max_iterations must lie in [1, 256]");
    if (p->min_matches < 1) return fail(L3D_ERR_ARG, "min_matches must be at least 1");
    if (p->estimate_scale > 1) return fail(L3D_ERR_ARG, "estimate_scale must be 0 or 1");
    if (p->reserved[0] || p->reserved[1]) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

int check_similarity(const l3d_similarity* s) {
    if (!(s->scale > 0.0) || !std::isfinite(s->scale)) return fail(L3D_ERR_ARG, "similarity: scale must be finite and greater than 0");
    const double qq = ((s->q[0] * s->q[0] + s->q[1] * s->q[1]) + s->q[2] * s->q[2]) + s->q[3] * s->q[3];
    if (!(qq > 0.0) || !std::isfinite(qq)) return fail(L3D_ERR_ARG, "similarity: the quaternion must be finite and not zero");
    for (double t : s->t)
        if (!std::isfinite(t)) return fail(L3D_ERR_ARG, "similarity: the translation must be finite");
    return L3D_OK;
}

// the similarity a call starts from: the caller's, checked and with its quaternion normalised, or identity
int entry_similarity(const l3d_similarity* s, l3d_similarity& T) {
    if (!s) { T = l3d_similarity{1.0, {1.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}; return L3D_OK; }
    if (int rc = check_similarity(s)) return rc;
    T = *s;
    quat_normalise(T.q);
    return L3D_OK;
}

// Whoever applies a similarity divides its quaternion by its norm first -- the passes below and l3d_transform_segments
// alike, so that the latter reproduces a pass from the similarity the call returned.
void unit_quaternion(const l3d_similarity& T, double qh[4]) {
    for (int i = 0; i < 4; ++i) qh[i] = T.q[i];
    quat_normalise(qh);
}

void transform_host(size_t n, const double* segs, const l3d_similarity& T, double* out) {
    double qh[4], R[9];
    unit_quaternion(T, qh);
    sim_rotation(qh, R);
    for (size_t i = 0; i < 2 * n; ++i) sim_point(T.scale, R, T.t, segs + 3 * i, out + 3 * i);
}

// H delta = -b by a plain Cholesky factorisation H = L L^T, column by column (DESIGN §23 writes the loops out; they are
// cholesky_solve of l3d_model.h); without the scale, row and column 3 are left out and delta[3] = 0.  false: a pivot that
// is not finite and > 0.
bool solve_normal(const double* s, bool with_scale, double delta[7]) {
    static const int kRow[7] = {0, 7, 13, 18, 22, 25, 27};   // where row i of the upper triangle begins
    int idx[7], n = 0;
    for (int i = 0; i < 7; ++i)
        if (with_scale || i != 3) idx[n++] = i;
    double H[7 * 7] = {}, rhs[7], x[7], work[kCholeskyWork];
    for (int i = 0; i < n; ++i) {
        for (int j = i; j < n; ++j) H[i * n + j] = s[kRow[idx[i]] + (idx[j] - idx[i])];
        rhs[i] = -s[28 + idx[i]];
    }
    if (!cholesky_solve(n, H, rhs, x, work)) return false;
    for (int i = 0; i < 7; ++i) delta[i] = 0.0;
    for (int i = 0; i < n; ++i) delta[idx[i]] = x[i];
    return true;
}

// step 6: the update about c
void update(l3d_similarity& T, const double delta[7], const double c[3]) {
    double dR[9];
    quat_step(delta, T.q, dR);
    const double m = 1.0 + delta[3];
    const d3 u = mul33(dR, d3{T.t[0] - c[0], T.t[1] - c[1], T.t[2] - c[2]});
    T.scale = T.scale * m;
    T.t[0] = (c[0] + m * u.x) + delta[4]; T.t[1] = (c[1] + m * u.y) + delta[5]; T.t[2] = (c[2] + m * u.z) + delta[6];
}

double step_of(const double delta[7], double diag) {
    double s = std::fabs(delta[3]);
    for (int i = 0; i < 3; ++i) {
        s = std::max(s, std::fabs(delta[i]));
        s = std::max(s, std::fabs(delta[4 + i]) / diag);
    }
    return s;
}

struct Model { uint32_t n; const double* segs; const uint32_t* line; };
struct Outputs {
    l3d_similarity* similarity; l3d_align_summary* summary; double* segs6; l3d_line_match* q; l3d_line_match* r;
    l3d_align_iteration* trace;
};

void nothing(l3d_line_match* out, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) out[i] = l3d_line_match{-1, 0xFFFFFFFFu, 0u, 0.0f, 0.0};
}

void records(const CmpOut* res, uint32_t n, l3d_line_match* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = l3d_line_match{res[i].segment, res[i].line, res[i].n_accepted, res[i].overlap, std::sqrt(res[i].d2)};
}

// Arguments already checked, both sides non-empty, T the entry similarity, (c, diag) the box of R.  Outputs are written
// only after everything has run.  kernel_ms (may be null): the time of every launch of the call, summed.
int align_core(ProjWork& w, hipStream_t st, const Model& Q, const Model& R, const l3d_align_params& p, l3d_similarity T,
               const double c[3], double diag, const Outputs& o, float* kernel_ms) {
    const uint32_t n_tiles = (Q.n + kCmpTile - 1) / kCmpTile;
    const SlicePlan plan_q = slice_plan(Q.n, R.n, p.slice_chunks, sizeof(CmpPartial), kAlnPartialBudget);
    const SlicePlan plan_r = o.r ? slice_plan(R.n, Q.n, p.slice_chunks, sizeof(CmpPartial), kAlnPartialBudget) : SlicePlan{0, 0};
    size_t b_part = plan_q.n_slices > 1 ? sizeof(CmpPartial) * (size_t)Q.n * plan_q.n_slices : 0;
    if (plan_r.n_slices > 1) b_part = std::max(b_part, sizeof(CmpPartial) * (size_t)R.n * plan_r.n_slices);
    const size_t b_tiles = sizeof(double) * kAlnTerms * (size_t)n_tiles;
    Layout lay;
    const size_t o_qs = lay.take(48 * (size_t)Q.n), o_ql = lay.take(4 * (size_t)Q.n), o_rs = lay.take(48 * (size_t)R.n), o_rl = lay.take(4 * (size_t)R.n);
    const size_t in_bytes = lay.at;
    const size_t o_tiles = lay.take(b_tiles), o_moved = lay.take(48 * (size_t)Q.n), o_mq = lay.take(24 * (size_t)Q.n);
    const size_t o_mr = lay.take(o.r ? 24 * (size_t)R.n : 0), host_bytes = lay.at;
    const size_t o_part = lay.take(b_part), total = lay.at;
    if (w.h.reserve(host_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess) return fail(L3D_ERR_HIP, "alignment: allocation failed");
    char* h = w.h.p; char* d = w.d.p;
    std::memcpy(h + o_qs, Q.segs, 48 * (size_t)Q.n); std::memcpy(h + o_ql, Q.line, 4 * (size_t)Q.n);
    std::memcpy(h + o_rs, R.segs, 48 * (size_t)R.n); std::memcpy(h + o_rl, R.line, 4 * (size_t)R.n);
    KernelTimer timer(kernel_ms);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "alignment: no event");
    hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("alignment: ") + hipGetErrorString(e));

    double sums[kAlnTerms];
    // steps 2-4 under T at `gate`, the tiles' sums added in ascending order into `sums`; final: the records and the moved
    // queries come down too
    auto pass = [&](const l3d_similarity& T_, double gate, bool final) -> hipError_t {
        double qh[4];
        unit_quaternion(T_, qh);
        AlnTransformArgs ta{(const double*)(d + o_qs), (double*)(d + o_moved), Q.n, T_.scale,
                            {qh[0], qh[1], qh[2], qh[3]}, {T_.t[0], T_.t[1], T_.t[2]}};
        CmpArgs ca{(const double*)(d + o_moved), (const uint32_t*)(d + o_ql), Q.n, (const double*)(d + o_rs), (const uint32_t*)(d + o_rl), R.n,
                   plan_q.slice_chunks, plan_q.n_slices, 0u, gate * gate, p.min_cos2, p.min_overlap, (CmpOut*)(d + o_mq), (CmpPartial*)(d + o_part)};
        AlnNormalArgs na{(const double*)(d + o_moved), Q.n, (const double*)(d + o_rs), R.n, (const CmpOut*)(d + o_mq), {c[0], c[1], c[2]},
                         (double*)(d + o_tiles)};
        hipError_t e_ = timer.start(st);
        if (e_ == hipSuccess) e_ = launch_align_transform(ta, st);
        if (e_ == hipSuccess) e_ = launch_compare(ca, st);
        if (e_ == hipSuccess) e_ = launch_compare_merge(ca, st);
        if (e_ == hipSuccess) e_ = launch_align_normal(na, st);
        if (e_ == hipSuccess) e_ = timer.stop(st);
        if (e_ == hipSuccess) e_ = hipMemcpyAsync(h + o_tiles, d + o_tiles, b_tiles, hipMemcpyDeviceToHost, st);
        if (e_ == hipSuccess && final) e_ = hipMemcpyAsync(h + o_moved, d + o_moved, 48 * (size_t)Q.n, hipMemcpyDeviceToHost, st);
        if (e_ == hipSuccess && final) e_ = hipMemcpyAsync(h + o_mq, d + o_mq, 24 * (size_t)Q.n, hipMemcpyDeviceToHost, st);
        if (e_ == hipSuccess) e_ = hipStreamSynchronize(st);
        if (e_ != hipSuccess) return e_;
        timer.add();
        g_aln_normal_launches.fetch_add(1, std::memory_order_relaxed);
        const double* tiles = (const double*)(h + o_tiles);
        for (uint32_t k = 0; k < kAlnTerms; ++k) sums[k] = 0.0;
        for (uint32_t t = 0; t < n_tiles; ++t)
            for (uint32_t k = 0; k < kAlnTerms; ++k) sums[k] = sums[k] + tiles[(size_t)t * kAlnTerms + k];
        return hipSuccess;
    };

    std::vector<l3d_align_iteration> trace;
    uint32_t status = L3D_ALIGN_MAX_ITERATIONS;
    double g = p.start_distance, last_step = 0.0;
    for (uint32_t k = 0; k < p.max_iterations; ++k) {
        const double gate = g > p.max_distance ? g : p.max_distance;
        g = g * 0.5;
        if ((e = pass(T, gate, false)) != hipSuccess) break;
        g_aln_iterations.fetch_add(1, std::memory_order_relaxed);
        l3d_align_iteration it{};
        it.gate = gate;
        std::memcpy(it.sums, sums, sizeof(sums));
        it.n_matched = (uint64_t)sums[36];
        it.similarity = T;
        trace.push_back(it);
        if (it.n_matched < p.min_matches) { status = L3D_ALIGN_TOO_FEW; break; }
        double delta[7];
        if (!solve_normal(sums, p.estimate_scale != 0, delta)) { status = L3D_ALIGN_DEGENERATE; break; }
        update(T, delta, c);
        last_step = step_of(delta, diag);
        std::memcpy(trace.back().delta, delta, sizeof(delta));
        trace.back().similarity = T;
        if (gate == p.max_distance && last_step <= p.step_tolerance) { status = L3D_ALIGN_CONVERGED; break; }
    }
    // the delivery pass
    if (e == hipSuccess) e = pass(T, p.max_distance, true);
    if (e == hipSuccess && o.r) {
        CmpArgs ca{(const double*)(d + o_rs), (const uint32_t*)(d + o_rl), R.n, (const double*)(d + o_moved), (const uint32_t*)(d + o_ql), Q.n,
                   plan_r.slice_chunks, plan_r.n_slices, 0u, p.max_distance * p.max_distance, p.min_cos2, p.min_overlap,
                   (CmpOut*)(d + o_mr), (CmpPartial*)(d + o_part)};
        e = timer.start(st);
        if (e == hipSuccess) e = launch_compare(ca, st);
        if (e == hipSuccess) e = launch_compare_merge(ca, st);
        if (e == hipSuccess) e = timer.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(h + o_mr, d + o_mr, 24 * (size_t)R.n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) timer.add();
    }
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("alignment: ") + hipGetErrorString(e));

    l3d_align_summary s{};
    s.status = status; s.iterations = (uint32_t)trace.size(); s.n_matched = (uint64_t)sums[36];
    s.rms = s.n_matched ? std::sqrt(sums[35] / (2.0 * sums[36])) : 0.0;
    s.last_step = last_step; s.diag = diag;
    for (int k = 0; k < 3; ++k) s.center[k] = c[k];
    *o.similarity = T; *o.summary = s;
    if (o.segs6) std::memcpy(o.segs6, h + o_moved, 48 * (size_t)Q.n);
    if (o.q) records((const CmpOut*)(h + o_mq), Q.n, o.q);
    if (o.r) records((const CmpOut*)(h + o_mr), R.n, o.r);
    if (o.trace) std::memcpy(o.trace, trace.data(), sizeof(l3d_align_iteration) * trace.size());
    return L3D_OK;
}

// what both entries check and decide before any device work.  done: the call is answered (an error, or an empty side)
int prepare(const Model& Q, const Model& R, const l3d_align_params* p, const l3d_similarity* initial, const Outputs& o,
            l3d_similarity& T, double c[3], double& diag, bool& done) {
    done = true;
    if (!o.similarity || !o.summary) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = entry_similarity(initial, T)) return rc;
    c[0] = c[1] = c[2] = 0.0; diag = 0.0;
    if (R.n) bounding_box(R.n, R.segs, c, diag);
    if (Q.n && R.n) {
        if (!(diag > 0.0)) return fail(L3D_ERR_ARG, "the reference side's bounding box is a point");
        done = false;
        return L3D_OK;
    }
    // an empty side: nothing to iterate on
    l3d_align_summary s{};
    s.status = L3D_ALIGN_TOO_FEW; s.diag = diag;
    for (int k = 0; k < 3; ++k) s.center[k] = c[k];
    *o.similarity = T; *o.summary = s;
    if (o.segs6) transform_host(Q.n, Q.segs, T, o.segs6);
    if (o.q) nothing(o.q, Q.n);
    if (o.r) nothing(o.r, R.n);
    (void)p;
    return L3D_OK;
}

}  // namespace

extern "C" {

int l3d_align_segments(int device, uint32_t n_q, const double* q_segs6, const uint32_t* q_line, uint32_t n_r,
                       const double* r_segs6, const uint32_t* r_line, const l3d_align_params* params,
                       const l3d_similarity* initial, l3d_similarity* out_similarity, l3d_align_summary* summary,
                       double* out_segs6, l3d_line_match* out_q, l3d_line_match* out_r, l3d_align_iteration* trace) {
    if (int rc = check_params(params)) return rc;
    if (int rc = check_model("query", n_q, q_segs6, q_line)) return rc;
    if (int rc = check_model("reference", n_r, r_segs6, r_line)) return rc;
    const Model Q{n_q, q_segs6, q_line}, R{n_r, r_segs6, r_line};
    const Outputs o{out_similarity, summary, out_segs6, out_q, out_r, trace};
    l3d_similarity T; double c[3], diag; bool done;
    if (int rc = prepare(Q, R, params, initial, o, T, c, diag, done)) return rc;
    if (done) return L3D_OK;
    if (int rc = set_device(device)) return rc;
    ProjWork w;
    return align_core(w, 0, Q, R, *params, T, c, diag, o, nullptr);
}

int l3d_align_lines(l3d_ctx* c, uint32_t n_other, const double* other_segs6, const uint32_t* other_line,
                    const l3d_align_params* params, const l3d_similarity* initial, l3d_similarity* out_similarity,
                    l3d_align_summary* summary, double* out_segs6, l3d_line_match* out_mine, l3d_line_match* out_other,
                    l3d_align_iteration* trace) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    if (int rc = check_model("other", n_other, other_segs6, other_line)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "lines are aligned", "align")) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (int rc = check_model("context's", line.size(), P6.data(), line.data())) return rc;
    const Model Q{(uint32_t)line.size(), P6.data(), line.data()}, R{n_other, other_segs6, other_line};
    const Outputs o{out_similarity, summary, out_segs6, out_mine, out_other, trace};
    l3d_similarity T; double ctr[3], diag; bool done;
    if (int rc = prepare(Q, R, params, initial, o, T, ctr, diag, done)) return rc;
    if (done) return L3D_OK;
    if (int rc = set_device(c->device)) return rc;
    float ms = 0.0f;
    const bool timed = c->timing_level >= 2;
    if (int rc = align_core(c->proj, c->stream, Q, R, *params, T, ctr, diag, o, timed ? &ms : nullptr)) return rc;
    if (timed) g_aln_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
    return L3D_OK;
}

int l3d_transform_segments(uint32_t n, const double* segs6, const l3d_similarity* similarity, double* out_segs6) {
    if (!similarity || (n && (!segs6 || !out_segs6))) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_similarity(similarity)) return rc;
    transform_host(n, segs6, *similarity, out_segs6);
    return L3D_OK;
}

}  // extern "C"
