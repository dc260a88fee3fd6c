// l3d_wireframe.hip -- where 3D lines meet (kernels: k_wireframe.hip): the stateless l3d_wireframe_segments
// on a caller's model, l3d_wireframe_lines on the context's lines, which it leaves untouched, and the handle that holds the
// result.
//
// Stage 1, the junctions of the model, runs on the device: count, scan (k_scan.hip), write, with the total read in
// between -- the one host wait inside the call -- so that the list is allocated at its size and the limit of 2^28
// junctions is checked before it is.  Stage 2, the graph, is host code in l3d_wireframe.h.
#include <atomic>
#include <cstdio>
#include <memory>

#include "l3d_ctx.h"
#include "l3d_wireframe.h"

namespace l3d {
// test hooks (l3d_debug_counter): launches of k_wf_count and k_wf_write so far; the slices, the junctions and the
// workgroups of the count pass that left by the triangular rule in the last call; the kernel time of the last timed call
// (context at timing level 2), and the part of it that the count pass and the scan took
std::atomic<uint64_t> g_wf_count_launches{0}, g_wf_write_launches{0}, g_wf_slices{0}, g_wf_junctions{0}, g_wf_skipped_blocks{0}, g_wf_kernel_ns{0}, g_wf_count_ns{0};
}  // namespace l3d

using namespace l3d;

struct l3d_wireframe { WfGraph g; };

namespace {

constexpr uint64_t kWfMaxJunctions = 1ull << 28;
constexpr uint32_t kWfNoWrap = 92682;                     // up to here n (n - 1) / 2 pairs fit the 32-bit scan
constexpr size_t kWfCountBudget = (size_t)256 << 20;      // the counts stay within this
static_assert(sizeof(WfRecord) == sizeof(WfJunction), "the device's record is the graph's");

int check_params(const l3d_wireframe_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (!(p->max_distance >= 0.0) || !std::isfinite(p->max_distance)) return fail(L3D_ERR_ARG, "max_distance must be finite and not negative");
    if (!(p->max_extension >= 0.0) || !std::isfinite(p->max_extension)) return fail(L3D_ERR_ARG, "max_extension must be finite and not negative");
    if (!(p->min_sin2 >= 0.0 && p->min_sin2 <= 1.0)) return fail(L3D_ERR_ARG, "min_sin2 must lie in [0, 1]");
    if (p->reserved != 0) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

// the workgroups of the count pass that leave by the triangular rule: those of tile t and slice s whose last reference,
// min((s + 1) * slice_chunks * 256, n) - 1, is at or below the tile's first query 256 t
uint64_t skipped_blocks(uint32_t n, const SlicePlan& plan) {
    const uint64_t per_slice = (uint64_t)plan.slice_chunks * kSliceChunk;
    uint64_t skipped = 0;
    for (uint64_t q0 = 0; q0 < n; q0 += kCmpTile)            // (the last slice ends at n, the others at multiples of per_slice)
        skipped += std::min<uint64_t>(plan.n_slices - 1, (q0 + 1) / per_slice) + (n <= q0 + 1 ? 1 : 0);
    return skipped;
}

}  // namespace

namespace l3d {

// ---- stage 1: the junctions, ascending (a, b).  n > 0, arguments checked.  kernel_ms (may be null): [0] the time of the
// count pass with its scan, [1] that of the write pass.  Slices by §18's rule, the counts within kWfCountBudget.
// keep (null for the wireframe itself): the list stays on the device and `out` stays empty (l3d_ctx.h).
int wf_junctions(ProjWork& w, hipStream_t st, uint32_t n, const double* segs, const uint32_t* line, const l3d_wireframe_params& p,
                 std::vector<WfRecord>& out, float* kernel_ms, WfOnDevice* keep) {
    out.clear();
    if (keep) { keep->segs = nullptr; keep->line = nullptr; keep->junctions = nullptr; keep->n_junctions = 0; }
    const SlicePlan plan = slice_plan(n, n, p.slice_chunks, sizeof(uint32_t), kWfCountBudget);
    const uint32_t n_slices = plan.n_slices;
    const size_t cells = (size_t)n * n_slices;
    const size_t b_seg = 48 * (size_t)n, b_line = 4 * (size_t)n, b_cnt = 4 * (cells + 2);   // counts, the total, the wrap flag
    Layout lay;
    const size_t o_seg = lay.take(b_seg), o_line = lay.take(b_line), in_bytes = lay.at, o_cnt = lay.take(b_cnt), total = lay.at;
    if (w.h.reserve(in_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess ||
        w.scan_ws.reserve_zeroed(scan_ws_words(cells, 4), st) != hipSuccess)
        return fail(L3D_ERR_HIP, "wireframe: allocation failed");
    char* d = w.d.p;
    std::memcpy(w.h.p + o_seg, segs, b_seg);
    std::memcpy(w.h.p + o_line, line, b_line);
    KernelTimer timer(kernel_ms), timer_w(kernel_ms ? kernel_ms + 1 : nullptr);
    if (!timer.ok() || !timer_w.ok()) return fail(L3D_ERR_HIP, "wireframe: no event");
    WfArgs a{(const double*)(d + o_seg), (const uint32_t*)(d + o_line), n, plan.slice_chunks, n_slices, p.max_distance * p.max_distance,
             p.max_extension, p.min_sin2, (uint32_t*)(d + o_cnt), nullptr, 0u, (uint32_t*)(d + o_cnt) + cells + 1};
    uint32_t tail[2] = {0, 0};                             // the total and the wrap flag
    hipError_t e = hipMemcpyAsync(d, w.h.p, in_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.wrapped, 0, 4, st);
    if (e == hipSuccess) e = timer.start(st);
    if (e == hipSuccess) e = launch_wf_count(a, st);
    if (e == hipSuccess) e = launch_scan(a.counts, (uint32_t)cells, a.counts, w.scan_ws.p, nullptr, st);
    if (e == hipSuccess && n > kWfNoWrap) e = launch_wf_check(a, st);
    if (e == hipSuccess) e = timer.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(tail, a.counts + cells, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) timer.add();
    int rc = L3D_OK;
    if (e == hipSuccess) {
        g_wf_count_launches.fetch_add(1, std::memory_order_relaxed);
        g_wf_slices.store(n_slices, std::memory_order_relaxed);
        g_wf_skipped_blocks.store(skipped_blocks(n, plan), std::memory_order_relaxed);
        if (tail[1] || tail[0] > (keep ? keep->max_junctions : kWfMaxJunctions))
            rc = fail(L3D_ERR_LIMIT, keep ? keep->limit_message : "more than 2^28 junctions");
    }
    const size_t n_out = tail[0];
    if (e == hipSuccess && rc == L3D_OK && n_out) {        // (no junction: no write pass)
        if (w.keys.reserve(4 * n_out) != hipSuccess || (!keep && w.h.reserve(32 * n_out) != hipSuccess)) return fail(L3D_ERR_HIP, "wireframe: allocation failed");
        a.out = (WfJunction*)w.keys.p; a.n_out = (uint32_t)n_out;
        e = timer_w.start(st);
        if (e == hipSuccess) e = launch_wf_write(a, st);
        if (e == hipSuccess) e = timer_w.stop(st);
        if (e == hipSuccess && !keep) e = hipMemcpyAsync(w.h.p, a.out, 32 * n_out, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) timer_w.add();
        if (e == hipSuccess) {
            g_wf_write_launches.fetch_add(1, std::memory_order_relaxed);
            if (!keep) {
                const WfRecord* got = (const WfRecord*)w.h.p;
                out.assign(got, got + n_out);
            }
        }
    }
    if (e == hipSuccess && rc == L3D_OK && keep) { keep->segs = a.segs; keep->line = a.line; keep->junctions = a.out; keep->n_junctions = n_out; }
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("wireframe: ") + hipGetErrorString(e));
    if (rc == L3D_OK) g_wf_junctions.store(n_out, std::memory_order_relaxed);
    return rc;
}

}  // namespace l3d

extern "C" {

int l3d_wireframe_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_wireframe_params* params,
                           l3d_wireframe** out) {
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_model(nullptr, n, segs6, line)) return rc;
    auto wf = std::make_unique<l3d_wireframe>();
    if (n) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        std::vector<WfRecord> rec;
        if (int rc = wf_junctions(w, 0, n, segs6, line, *params, rec, nullptr)) return rc;
        wf_graph(n, segs6, line, params->max_distance, params->max_extension, rec.data(), rec.size(), wf->g);
    }
    *out = wf.release();
    return L3D_OK;
}

int l3d_wireframe_lines(l3d_ctx* c, const l3d_wireframe_params* params, l3d_wireframe** out) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "a wireframe is built", "connect")) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (int rc = check_model(nullptr, line.size(), P6.data(), line.data())) return rc;
    const uint32_t n = (uint32_t)line.size();
    auto wf = std::make_unique<l3d_wireframe>();
    if (n) {
        if (int rc = set_device(c->device)) return rc;
        float ms[2] = {0.0f, 0.0f};
        const bool timed = c->timing_level >= 2;
        std::vector<WfRecord> rec;
        if (int rc = wf_junctions(c->proj, c->stream, n, P6.data(), line.data(), *params, rec, timed ? ms : nullptr)) return rc;
        if (timed) {
            g_wf_kernel_ns.store((uint64_t)(((double)ms[0] + (double)ms[1]) * 1e6), std::memory_order_relaxed);
            g_wf_count_ns.store((uint64_t)((double)ms[0] * 1e6), std::memory_order_relaxed);
        }
        wf_graph(n, P6.data(), line.data(), params->max_distance, params->max_extension, rec.data(), rec.size(), wf->g);
    }
    *out = wf.release();
    return L3D_OK;
}

int l3d_wireframe_counts(const l3d_wireframe* wf, uint64_t* n_junctions, uint64_t* n_vertices, uint64_t* n_edges) {
    if (!wf) return fail(L3D_ERR_ARG, "null argument");
    if (n_junctions) *n_junctions = wf->g.junctions.size();
    if (n_vertices) *n_vertices = wf->g.vertices.size();
    if (n_edges) *n_edges = wf->g.edges.size();
    return L3D_OK;
}

int l3d_wireframe_get(const l3d_wireframe* wf, l3d_wf_junction* junctions, l3d_wf_vertex* vertices, l3d_wf_edge* edges,
                      l3d_wireframe_summary* summary) {
    if (!wf) return fail(L3D_ERR_ARG, "null argument");
    const WfGraph& g = wf->g;
    if (junctions && !g.junctions.empty()) std::memcpy(junctions, g.junctions.data(), sizeof(l3d_wf_junction) * g.junctions.size());
    if (vertices && !g.vertices.empty()) std::memcpy(vertices, g.vertices.data(), sizeof(l3d_wf_vertex) * g.vertices.size());
    if (edges && !g.edges.empty()) std::memcpy(edges, g.edges.data(), sizeof(l3d_wf_edge) * g.edges.size());
    if (summary) *summary = g.sum;
    return L3D_OK;
}

int l3d_wireframe_save_obj(const l3d_wireframe* wf, const char* path) {
    if (!wf || !path) return fail(L3D_ERR_ARG, "null argument");
    FILE* f = std::fopen(path, "w");
    if (!f) return fail(L3D_ERR_IO, std::string("cannot write ") + path);
    for (const l3d_wf_vertex& v : wf->g.vertices) std::fprintf(f, "v %.17g %.17g %.17g\n", v.P[0], v.P[1], v.P[2]);
    for (const l3d_wf_edge& e : wf->g.edges) std::fprintf(f, "l %u %u\n", e.v0 + 1, e.v1 + 1);
    const bool bad = std::ferror(f) != 0;
    if (std::fclose(f) != 0 || bad) return fail(L3D_ERR_IO, std::string("cannot write ") + path);
    return L3D_OK;
}

void l3d_wireframe_close(l3d_wireframe* wf) { delete wf; }

}  // extern "C"
