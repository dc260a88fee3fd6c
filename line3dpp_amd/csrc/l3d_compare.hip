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

constexpr uint32_t kCmpMaxSegments = 1u << 30;
constexpr size_t kCmpPartialBudget = (size_t)256 << 20;   // the partials of a direction stay within this
constexpr double kCmpMaxCoord = 0x1p100;
static_assert(sizeof(CmpOut) == sizeof(l3d_line_match) && sizeof(l3d_line_match) == 24, "match layout");
static_assert(sizeof(l3d_compare_params) == 32 && sizeof(l3d_compare_summary) == 56, "comparison structs");

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int check_params(const l3d_compare_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (!(p->max_distance >= 0.0) || !std::isfinite(p->max_distance)) return fail(L3D_ERR_ARG, "max_distance must be finite and not negative");
    if (!(p->min_cos2 >= 0.0 && p->min_cos2 <= 1.0)) return fail(L3D_ERR_ARG, "min_cos2 must lie in [0, 1]");
    if (!(p->min_overlap >= 0.0 && p->min_overlap <= 1.0)) return fail(L3D_ERR_ARG, "min_overlap must lie in [0, 1]");
    if (p->exclude_same_line > 1) return fail(L3D_ERR_ARG, "exclude_same_line must be 0 or 1");
    return L3D_OK;
}

struct Side { const char* name; uint32_t n; const double* segs; const uint32_t* line; };

int check_side(const Side& s) {
    if (s.n >= kCmpMaxSegments) return fail(L3D_ERR_LIMIT, std::string("the ") + s.name + " side has 2^30 or more segments");
    if (s.n && (!s.segs || !s.line)) return fail(L3D_ERR_ARG, "null argument");
    for (size_t i = 0; i < 6 * (size_t)s.n; ++i)
        if (!(std::fabs(s.segs[i]) <= kCmpMaxCoord))   // (NaN and the infinities fail it too)
            return fail(L3D_ERR_ARG, std::string("the ") + s.name + " side: segment " + std::to_string(i / 6) +
                                         " has a coordinate that is not finite or beyond 2^100");
    return L3D_OK;
}

// Slices of a direction with n_q queries and n_r references (both > 0), and the chunks per slice that go with them.
// The library's own choice is ONE CHUNK PER SLICE: measured on C1 and C2 it is the fastest of the slicings
// tried or level with it, where a rule that aims at 1024 workgroups was 35 % slower at C2 (13 slices of 5 chunks on 65
// tiles: 3.3 workgroups per compute unit, where seven fit).
void slicing(uint32_t n_q, uint32_t n_r, uint32_t asked_chunks, uint32_t& n_slices, uint32_t& slice_chunks) {
    const uint32_t n_chunks = (n_r + kCmpChunk - 1) / kCmpChunk;
    const uint32_t cap = (uint32_t)std::max<size_t>(1, kCmpPartialBudget / (sizeof(CmpPartial) * (size_t)n_q));
    slice_chunks = asked_chunks ? std::min(asked_chunks, n_chunks) : 1;
    n_slices = (n_chunks + slice_chunks - 1) / slice_chunks;
    if (n_slices <= cap) return;
    n_slices = cap;
    slice_chunks = (n_chunks + n_slices - 1) / n_slices;
    n_slices = (n_chunks + slice_chunks - 1) / slice_chunks;       // no slice is empty
}

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
// Results and summaries are written only after everything has run.  kernel_ms (may be null): events around the launches
// of every direction, summed.
int compare_core(ProjWork& w, hipStream_t st, const Side side[2], const l3d_compare_params& p, l3d_line_match* const out[2],
                 l3d_compare_summary* const sum[2], float* kernel_ms) {
    const size_t b_seg[2] = {48 * (size_t)side[0].n, 48 * (size_t)side[1].n}, b_line[2] = {4 * (size_t)side[0].n, 4 * (size_t)side[1].n};
    const size_t b_out[2] = {out[0] ? 24 * (size_t)side[0].n : 0, out[1] ? 24 * (size_t)side[1].n : 0};
    uint32_t n_slices[2] = {0, 0}, slice_chunks[2] = {0, 0};
    size_t b_part = 0;
    for (int k = 0; k < 2; ++k)
        if (out[k]) {
            slicing(side[k].n, side[1 - k].n, p.slice_chunks, n_slices[k], slice_chunks[k]);
            if (n_slices[k] > 1) b_part = std::max(b_part, sizeof(CmpPartial) * (size_t)side[k].n * n_slices[k]);
        }
    const size_t o_seg[2] = {0, up256(b_seg[0])};
    const size_t o_line[2] = {up256(o_seg[1] + b_seg[1]), up256(up256(o_seg[1] + b_seg[1]) + b_line[0])};
    const size_t in_bytes = o_line[1] + b_line[1];
    const size_t o_out[2] = {up256(in_bytes), up256(up256(in_bytes) + b_out[0])};
    const size_t host_bytes = o_out[1] + b_out[1], o_part = up256(host_bytes), total = o_part + b_part;
    if (w.h.reserve(host_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess) return fail(L3D_ERR_HIP, "comparison: allocation failed");
    char* h = w.h.p; char* d = w.d.p;
    for (int k = 0; k < 2; ++k) {
        std::memcpy(h + o_seg[k], side[k].segs, b_seg[k]);
        std::memcpy(h + o_line[k], side[k].line, b_line[k]);
    }
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (kernel_ms) {
        *kernel_ms = 0.0f;
        if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            return fail(L3D_ERR_HIP, "comparison: no event");
        }
    }
    hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        if (!out[k]) continue;
        const Side& q = side[k]; const Side& r = side[1 - k];
        CmpArgs a{(const double*)(d + o_seg[k]), (const uint32_t*)(d + o_line[k]), q.n,
                  (const double*)(d + o_seg[1 - k]), (const uint32_t*)(d + o_line[1 - k]), r.n,
                  slice_chunks[k], n_slices[k], p.exclude_same_line, p.max_distance * p.max_distance, p.min_cos2, p.min_overlap,
                  (CmpOut*)(d + o_out[k]), (CmpPartial*)(d + o_part)};
        if (kernel_ms) e = hipEventRecord(ev[0], st);
        if (e == hipSuccess) e = launch_compare(a, st);
        if (e == hipSuccess) e = launch_compare_merge(a, st);
        if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev[1], st);
        if (e == hipSuccess) e = hipMemcpyAsync(h + o_out[k], d + o_out[k], b_out[k], hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && kernel_ms) {           // (the events of a direction are read before the next one reuses them)
            e = hipStreamSynchronize(st);
            if (e == hipSuccess) *kernel_ms += ev_ms(ev[0], ev[1]);
        }
        if (e != hipSuccess) break;
        g_cmp_launches.fetch_add(1, std::memory_order_relaxed);
        if (n_slices[k] > 1) g_cmp_merge_launches.fetch_add(1, std::memory_order_relaxed);
        g_cmp_slices.store(n_slices[k], std::memory_order_relaxed);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
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
        if (int rc = check_side(s)) return rc;
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
    if (int rc = check_side(other)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (c->state == l3d_ctx::BEGUN || c->aff_shard_open) return fail(L3D_ERR_STATE, "lines are compared while a split call is open");
    if (!c->lines_done) return fail(L3D_ERR_STATE, "no 3D lines to compare: l3d_reconstruct_3d_lines has not run");
    // lines3D_ of the context, flattened as l3d_get_3d_lines flattens it
    std::vector<double> P6; std::vector<uint32_t> line;
    for (size_t i = 0; i < c->lines3D.size(); ++i)
        for (const ReconSeg3D& s : c->lines3D[i].collinear) {
            const double p[6] = {s.P1.x, s.P1.y, s.P1.z, s.P2.x, s.P2.y, s.P2.z};
            P6.insert(P6.end(), p, p + 6);
            line.push_back((uint32_t)i);
        }
    if (line.size() >= kCmpMaxSegments) return fail(L3D_ERR_LIMIT, "the context's side has 2^30 or more segments");
    const Side side[2] = {{"context's", (uint32_t)line.size(), P6.data(), line.data()}, other};
    if (int rc = check_side(side[0])) return rc;
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
