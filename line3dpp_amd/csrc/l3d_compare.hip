// l3d_compare.hip -- host side of the comparison of two 3D line models (kernels: k_compare.hip): the
// stateless l3d_compare_segments on a caller's two models, and l3d_compare_lines with the context's lines as one side,
// on the context's stream and the work space of the projection stages.
//
// One packed upload carries both models; per direction one launch of k_compare (and of k_compare_merge where the
// references are sliced) and one download, all through pinned staging.  The kernels hand out the squared distance and
// the root is taken here, after the download, by the host's correctly rounded sqrt.  The summaries are host code over
// the downloaded records.
//
// SLICING.  A model has a few thousand segments: a dozen tiles of 256 queries on 256 compute units.  The references are
// therefore cut into n_slices slices of slice_chunks chunks of 256, a workgroup per (tile, slice); a query's partial
// results are merged in ascending slice order without atomics, so no output depends on the slicing.
#include <atomic>

#include "l3d_ctx.h"

namespace l3d {
// test hooks (l3d_debug_counter): launches of k_compare and of k_compare_merge so far, the slices of the last direction
// run, and the kernel time of the last timed call (context at timing level 2)
std::atomic<uint64_t> g_cmp_launches{0}, g_cmp_merge_launches{0}, g_cmp_slices{0}, g_cmp_kernel_ns{0};
}  // namespace l3d

using namespace l3d;

namespace {

constexpr size_t kCmpPartialBudget = (size_t)256 << 20;   // the partials of a direction stay within this
static_assert(sizeof(CmpOut) == sizeof(l3d_line_match) && sizeof(l3d_line_match) == 24, "match layout");
static_assert(sizeof(l3d_compare_params) == 32 && sizeof(l3d_compare_summary) == 56, "comparison structs");

int check_params(const l3d_compare_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thresholds(p->max_distance, p->min_cos2, p->min_overlap)) return rc;
    if (p->exclude_same_line > 1) return fail(L3D_ERR_ARG, "exclude_same_line must be 0 or 1");
    return L3D_OK;
}

struct Side { const char* name; uint32_t n; const double* segs; const uint32_t* line; };

void nothing(l3d_line_match* out, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) out[i] = l3d_line_match{-1, 0xFFFFFFFFu, 0u, 0.0f, 0.0};
}

// one direction summed up: the queries q and their final records m
void summarize(const Side& q, const l3d_line_match* m, l3d_compare_summary* s) {
    l3d_compare_summary r{};
    r.n_segments = q.n;
    std::vector<uint32_t> lines(q.line, q.line + q.n), matched;
    for (uint32_t i = 0; i < q.n; ++i) {
        const double* v = q.segs + 6 * (size_t)i;
        const double ex = v[3] - v[0], ey = v[4] - v[1], ez = v[5] - v[2];
        const double len = std::sqrt(ex * ex + ey * ey + ez * ez);
        r.length_total += len;
        if (m[i].segment < 0) continue;
        ++r.n_matched;
        r.length_matched += len;
        if (m[i].n_accepted > 1) ++r.n_ambiguous;
        matched.push_back(q.line[i]);
    }
    std::sort(lines.begin(), lines.end());
    r.n_lines = (uint64_t)(std::unique(lines.begin(), lines.end()) - lines.begin());
    std::sort(matched.begin(), matched.end());
    r.n_lines_matched = (uint64_t)(std::unique(matched.begin(), matched.end()) - matched.begin());
    *s = r;
}

// Arguments already checked, both sides non-empty, at least one of out[0] (side 0 against side 1) and out[1] set.
// Results and summaries are written only after everything has run.  kernel_ms (may be null): the time of the launches of
// every direction, summed.  The slices of a direction: slice_plan of l3d_model.h, the partials within kCmpPartialBudget.
int compare_core(ProjWork& w, hipStream_t st, const Side side[2], const l3d_compare_params& p, l3d_line_match* const out[2],
                 l3d_compare_summary* const sum[2], float* kernel_ms) {
    const size_t b_seg[2] = {48 * (size_t)side[0].n, 48 * (size_t)side[1].n}, b_line[2] = {4 * (size_t)side[0].n, 4 * (size_t)side[1].n};
    const size_t b_out[2] = {out[0] ? 24 * (size_t)side[0].n : 0, out[1] ? 24 * (size_t)side[1].n : 0};
    SlicePlan plan[2] = {{0, 0}, {0, 0}};
    size_t b_part = 0;
    for (int k = 0; k < 2; ++k)
        if (out[k]) {
            plan[k] = slice_plan(side[k].n, side[1 - k].n, p.slice_chunks, sizeof(CmpPartial), kCmpPartialBudget);
            if (plan[k].n_slices > 1) b_part = std::max(b_part, sizeof(CmpPartial) * (size_t)side[k].n * plan[k].n_slices);
        }
    Layout lay;
    const size_t o_seg[2] = {lay.take(b_seg[0]), lay.take(b_seg[1])}, o_line[2] = {lay.take(b_line[0]), lay.take(b_line[1])};
    const size_t in_bytes = lay.at, o_out[2] = {lay.take(b_out[0]), lay.take(b_out[1])}, host_bytes = lay.at;
    const size_t o_part = lay.take(b_part), total = lay.at;
    if (w.h.reserve(host_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess) return fail(L3D_ERR_HIP, "comparison: allocation failed");
    char* h = w.h.p; char* d = w.d.p;
    for (int k = 0; k < 2; ++k) {
        std::memcpy(h + o_seg[k], side[k].segs, b_seg[k]);
        std::memcpy(h + o_line[k], side[k].line, b_line[k]);
    }
    KernelTimer timer(kernel_ms);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "comparison: no event");
    hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        if (!out[k]) continue;
        const Side& q = side[k]; const Side& r = side[1 - k];
        CmpArgs a{(const double*)(d + o_seg[k]), (const uint32_t*)(d + o_line[k]), q.n,
                  (const double*)(d + o_seg[1 - k]), (const uint32_t*)(d + o_line[1 - k]), r.n,
                  plan[k].slice_chunks, plan[k].n_slices, p.exclude_same_line, p.max_distance * p.max_distance, p.min_cos2, p.min_overlap,
                  (CmpOut*)(d + o_out[k]), (CmpPartial*)(d + o_part)};
        e = timer.start(st);
        if (e == hipSuccess) e = launch_compare(a, st);
        if (e == hipSuccess) e = launch_compare_merge(a, st);
        if (e == hipSuccess) e = timer.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(h + o_out[k], d + o_out[k], b_out[k], hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && kernel_ms) {           // (the events of a direction are read before the next one reuses them)
            e = hipStreamSynchronize(st);
            if (e == hipSuccess) timer.add();
        }
        if (e != hipSuccess) break;
        g_cmp_launches.fetch_add(1, std::memory_order_relaxed);
        if (plan[k].n_slices > 1) g_cmp_merge_launches.fetch_add(1, std::memory_order_relaxed);
        g_cmp_slices.store(plan[k].n_slices, std::memory_order_relaxed);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("comparison: ") + hipGetErrorString(e));
    for (int k = 0; k < 2; ++k) {
        if (!out[k]) continue;
        const CmpOut* res = (const CmpOut*)(h + o_out[k]);
        for (uint32_t i = 0; i < side[k].n; ++i)
            out[k][i] = l3d_line_match{res[i].segment, res[i].line, res[i].n_accepted, res[i].overlap, std::sqrt(res[i].d2)};
        if (sum[k]) summarize(side[k], out[k], sum[k]);
    }
    return L3D_OK;
}

// the forms without work: no output asked for, or a side without segments (every record "nothing", zero summaries)
bool nothing_to_compare(const Side side[2], l3d_line_match* const out[2], l3d_compare_summary* const sum[2]) {
    if ((out[0] || out[1]) && side[0].n && side[1].n) return false;
    for (int k = 0; k < 2; ++k) {
        if (!out[k]) continue;
        nothing(out[k], side[k].n);
        if (sum[k]) *sum[k] = l3d_compare_summary{};
    }
    return true;
}

}  // namespace

extern "C" {

int l3d_compare_segments(int device, uint32_t n_q, const double* q_segs6, const uint32_t* q_line, uint32_t n_r,
                         const double* r_segs6, const uint32_t* r_line, const l3d_compare_params* params,
                         l3d_line_match* out_q, l3d_line_match* out_r, l3d_compare_summary* summary_q,
                         l3d_compare_summary* summary_r) {
    if (int rc = check_params(params)) return rc;
    const Side side[2] = {{"query", n_q, q_segs6, q_line}, {"reference", n_r, r_segs6, r_line}};
    for (const Side& s : side)
        if (int rc = check_model(s.name, s.n, s.segs, s.line)) return rc;
    l3d_line_match* const out[2] = {out_q, out_r};
    l3d_compare_summary* const sum[2] = {summary_q, summary_r};
    if (nothing_to_compare(side, out, sum)) return L3D_OK;
    if (int rc = set_device(device)) return rc;
    ProjWork w;
    return compare_core(w, 0, side, *params, out, sum, nullptr);
}

int l3d_compare_lines(l3d_ctx* c, uint32_t n_other, const double* other_segs6, const uint32_t* other_line,
                      const l3d_compare_params* params, l3d_line_match* out_mine, l3d_line_match* out_other,
                      l3d_compare_summary* summary_mine, l3d_compare_summary* summary_other) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    const Side other{"other", n_other, other_segs6, other_line};
    if (int rc = check_model(other.name, other.n, other.segs, other.line)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "lines are compared", "compare")) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (int rc = check_model("context's", line.size(), P6.data(), line.data())) return rc;
    const Side side[2] = {{"context's", (uint32_t)line.size(), P6.data(), line.data()}, other};
    l3d_line_match* const out[2] = {out_mine, out_other};
    l3d_compare_summary* const sum[2] = {summary_mine, summary_other};
    if (nothing_to_compare(side, out, sum)) return L3D_OK;
    if (int rc = set_device(c->device)) return rc;
    float ms = 0.0f;
    const bool timed = c->timing_level >= 2;
    if (int rc = compare_core(c->proj, c->stream, side, *params, out, sum, timed ? &ms : nullptr)) return rc;
    if (timed) g_cmp_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
    return L3D_OK;
}

}  // extern "C"
