// l3d_merge.hip -- near-duplicate 3D lines merged (kernels: k_merge.hip): the stateless l3d_merge_segments
// on a caller's model, and l3d_merge_lines, which replaces the context's lines by the merged ones.
//
// Stage 1, the accepted pairs of the model against itself, runs on the device: count, scan (k_scan.hip), write, with the
// total read in between -- the one host wait inside the call -- so that the list is allocated at its size and the limit
// of 2^28 pairs is checked before it is.  Stages 2 and 3, the components and the fusion, are host code: the pairs are
// few and the work is sequential (the rationale of l3d_recon.h).  All of it is fp64 in the order DESIGN §19 writes it,
// so that tests/merge_model.py follows it operation for operation.
#include <atomic>

#include "l3d_ctx.h"

namespace l3d {
// test hooks (l3d_debug_counter): launches of k_merge_count and k_merge_write so far, the slices and the pairs of the
// last call, and the kernel time of the last timed call (context at timing level 2)
std::atomic<uint64_t> g_mrg_count_launches{0}, g_mrg_write_launches{0}, g_mrg_slices{0}, g_mrg_pairs{0}, g_mrg_kernel_ns{0};
}  // namespace l3d

using namespace l3d;

namespace {

constexpr uint64_t kMrgMaxPairs = 1ull << 28;
constexpr uint32_t kMrgNoWrap = 1u << 16;                 // up to here n (n - 1) pairs fit the 32-bit scan
constexpr size_t kMrgCountBudget = (size_t)256 << 20;     // the counts stay within this
static_assert(sizeof(l3d_merge_params) == 32 && sizeof(l3d_merge_line_info) == 16 && sizeof(l3d_merge_summary) == 80, "merge structs");
static_assert(sizeof(MrgPair) == 8, "pair layout");

int check_params(const l3d_merge_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thresholds(p->max_distance, p->min_cos2, p->min_overlap)) return rc;
    if (p->reserved != 0) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

// ---- stage 1: the accepted pairs, ascending (q, r).  n > 0, arguments checked.  kernel_ms (may be null): the time of
// the count pass with its scan, and of the write pass, summed.  Slices by §18's rule, the counts within kMrgCountBudget.
int merge_pairs(ProjWork& w, hipStream_t st, uint32_t n, const double* segs, const uint32_t* line, const l3d_merge_params& p,
                std::vector<MrgPair>& pairs, float* kernel_ms) {
    pairs.clear();
    const SlicePlan plan = slice_plan(n, n, p.slice_chunks, sizeof(uint32_t), kMrgCountBudget);
    const uint32_t n_slices = plan.n_slices;
    const size_t cells = (size_t)n * n_slices;
    const size_t b_seg = 48 * (size_t)n, b_line = 4 * (size_t)n, b_cnt = 4 * (cells + 2);   // counts, the total, the wrap flag
    Layout lay;
    const size_t o_seg = lay.take(b_seg), o_line = lay.take(b_line), in_bytes = lay.at, o_cnt = lay.take(b_cnt), total = lay.at;
    if (w.h.reserve(in_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess ||
        w.scan_ws.reserve_zeroed(scan_ws_words(cells, 4), st) != hipSuccess)
        return fail(L3D_ERR_HIP, "merge: allocation failed");
    char* d = w.d.p;
    std::memcpy(w.h.p + o_seg, segs, b_seg);
    std::memcpy(w.h.p + o_line, line, b_line);
    KernelTimer timer(kernel_ms);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "merge: no event");
    MrgArgs a{(const double*)(d + o_seg), (const uint32_t*)(d + o_line), n, plan.slice_chunks, n_slices, p.max_distance * p.max_distance, p.min_cos2,
              p.min_overlap, (uint32_t*)(d + o_cnt), nullptr, 0u, (uint32_t*)(d + o_cnt) + cells + 1};
    uint32_t tail[2] = {0, 0};                             // the total and the wrap flag
    hipError_t e = hipMemcpyAsync(d, w.h.p, in_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.wrapped, 0, 4, st);
    if (e == hipSuccess) e = timer.start(st);
    if (e == hipSuccess) e = launch_merge_count(a, st);
    if (e == hipSuccess) e = launch_scan(a.counts, (uint32_t)cells, a.counts, w.scan_ws.p, nullptr, st);
    if (e == hipSuccess && n > kMrgNoWrap) e = launch_merge_check(a, st);
    if (e == hipSuccess) e = timer.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(tail, a.counts + cells, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) timer.add();
    int rc = L3D_OK;
    if (e == hipSuccess) {
        g_mrg_count_launches.fetch_add(1, std::memory_order_relaxed);
        g_mrg_slices.store(n_slices, std::memory_order_relaxed);
        if (tail[1] || tail[0] > kMrgMaxPairs) rc = fail(L3D_ERR_LIMIT, "more than 2^28 accepted pairs of segments");
    }
    const size_t n_pairs = tail[0];
    if (e == hipSuccess && rc == L3D_OK && n_pairs) {      // (no pair: no write pass)
        if (w.keys.reserve(n_pairs) != hipSuccess || w.h.reserve(8 * n_pairs) != hipSuccess) return fail(L3D_ERR_HIP, "merge: allocation failed");
        a.pairs = (MrgPair*)w.keys.p; a.n_pairs = (uint32_t)n_pairs;
        e = timer.start(st);
        if (e == hipSuccess) e = launch_merge_write(a, st);
        if (e == hipSuccess) e = timer.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(w.h.p, a.pairs, 8 * n_pairs, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) timer.add();
        if (e == hipSuccess) {
            g_mrg_write_launches.fetch_add(1, std::memory_order_relaxed);
            const MrgPair* got = (const MrgPair*)w.h.p;
            pairs.assign(got, got + n_pairs);
        }
    }
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("merge: ") + hipGetErrorString(e));
    if (rc == L3D_OK) g_mrg_pairs.store(n_pairs, std::memory_order_relaxed);
    return rc;
}

// ---- stages 2 and 3 ---------------------------------------------------------------------------------------------------
struct V3 { double x, y, z; };
double dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }   // left to right
V3 sub3(const double* p, const V3& c) { return {p[0] - c.x, p[1] - c.y, p[2] - c.z}; }

struct Merged {
    std::vector<uint32_t> line_map;                 // [n] output line of every input segment
    std::vector<double> segs;                       // [n_out x 6]
    std::vector<uint32_t> seg_line;                 // [n_out]
    std::vector<l3d_merge_line_info> info;          // [lines out]
    std::vector<uint32_t> seg_begin;                // [lines out + 1] the output segments of a line
    std::vector<uint32_t> leader_line;              // [lines out] input line index of the leader (of the label: untouched)
    std::vector<std::vector<uint32_t>> members;     // [lines out] the input line indices, ascending
    l3d_merge_summary sum{};
};

double length_of(const double* v) {
    const double ex = v[3] - v[0], ey = v[4] - v[1], ez = v[5] - v[2];
    return std::sqrt(ex * ex + ey * ey + ez * ez);
}

// one component of two or more lines: members = its live segments, ascending.  Appends the fused segments to m.segs.
void fuse(const double* segs, const std::vector<uint32_t>& members, Merged& m, double& max_offset, uint32_t& leader) {
    struct Mem { V3 e; double len; };
    std::vector<Mem> mem(members.size());
    size_t lead = 0;
    for (size_t k = 0; k < members.size(); ++k) {                                 // 1.
        const double* v = segs + 6 * (size_t)members[k];
        mem[k].e = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
        mem[k].len = std::sqrt(mem[k].e.x * mem[k].e.x + mem[k].e.y * mem[k].e.y + mem[k].e.z * mem[k].e.z);
        if (mem[k].len > mem[lead].len) lead = k;                                 // (the first of equal lengths stays)
    }
    leader = members[lead];
    V3 dsum{0.0, 0.0, 0.0};                                                       // 2.
    for (const Mem& x : mem) {
        const double s = dot3(x.e, mem[lead].e) < 0.0 ? -1.0 : 1.0;
        dsum.x += s * x.e.x; dsum.y += s * x.e.y; dsum.z += s * x.e.z;
    }
    const double dn = std::sqrt(dot3(dsum, dsum));
    const V3 u{dsum.x / dn, dsum.y / dn, dsum.z / dn};
    double W = 0.0;                                                               // 3.
    V3 cs{0.0, 0.0, 0.0};
    for (size_t k = 0; k < members.size(); ++k) {
        const double* v = segs + 6 * (size_t)members[k];
        const V3 mid{(v[0] + v[3]) * 0.5, (v[1] + v[4]) * 0.5, (v[2] + v[5]) * 0.5};
        W += mem[k].len;
        cs.x += mem[k].len * mid.x; cs.y += mem[k].len * mid.y; cs.z += mem[k].len * mid.z;
    }
    const V3 c{cs.x / W, cs.y / W, cs.z / W};
    struct Iv { double lo, hi; uint32_t index; };
    std::vector<Iv> iv(members.size());
    max_offset = 0.0;
    for (size_t k = 0; k < members.size(); ++k) {                                 // 4. and 7.
        const double* v = segs + 6 * (size_t)members[k];
        double t[2];
        for (int end = 0; end < 2; ++end) {
            const V3 wv = sub3(v + 3 * end, c);
            t[end] = dot3(wv, u);
            const double off2 = dot3(wv, wv) - t[end] * t[end];
            const double off = off2 > 0.0 ? std::sqrt(off2) : 0.0;
            if (off > max_offset) max_offset = off;
        }
        iv[k] = {t[0] < t[1] ? t[0] : t[1], t[0] < t[1] ? t[1] : t[0], members[k]};
    }
    std::sort(iv.begin(), iv.end(), [](const Iv& a, const Iv& b) { return a.lo < b.lo || (a.lo == b.lo && a.index < b.index); });   // 5.
    auto emit = [&](double lo, double hi) {                                       // 6.
        const double o[6] = {c.x + lo * u.x, c.y + lo * u.y, c.z + lo * u.z, c.x + hi * u.x, c.y + hi * u.y, c.z + hi * u.z};
        m.segs.insert(m.segs.end(), o, o + 6);
    };
    double cur_lo = iv[0].lo, cur_hi = iv[0].hi;
    for (size_t k = 1; k < iv.size(); ++k) {
        if (iv[k].lo <= cur_hi) { if (iv[k].hi > cur_hi) cur_hi = iv[k].hi; continue; }
        emit(cur_lo, cur_hi);
        cur_lo = iv[k].lo; cur_hi = iv[k].hi;
    }
    emit(cur_lo, cur_hi);
}

void merge_host(uint32_t n, const double* segs, const uint32_t* line, const std::vector<MrgPair>& pairs, Merged& m) {
    m = Merged();
    m.line_map.assign(n, 0);
    m.seg_begin.assign(1, 0);
    // ---- stage 2: union-find over the distinct line indices; the smaller index becomes the root, so a root is its label
    std::vector<uint32_t> ids(line, line + n);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    auto at = [&](uint32_t id) { return (uint32_t)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
    std::vector<uint32_t> slot(n), parent(ids.size());
    for (uint32_t i = 0; i < n; ++i) slot[i] = at(line[i]);
    for (uint32_t k = 0; k < parent.size(); ++k) parent[k] = k;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    for (const MrgPair& p : pairs) {
        const uint32_t a = find(slot[p.q]), b = find(slot[p.r]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    std::vector<uint32_t> out_of(ids.size(), 0);            // root slot -> output line
    for (uint32_t k = 0; k < ids.size(); ++k)
        if (find(k) == k) {
            out_of[k] = (uint32_t)m.info.size();
            m.info.push_back(l3d_merge_line_info{0u, ids[k], 0.0});
            m.members.emplace_back();
        }
    for (uint32_t k = 0; k < ids.size(); ++k) {             // (ascending: the members come out ascending)
        const uint32_t o = out_of[find(k)];
        ++m.info[o].n_members;
        m.members[o].push_back(ids[k]);
    }
    std::vector<std::vector<uint32_t>> segs_of(m.info.size());
    for (uint32_t i = 0; i < n; ++i) {
        m.line_map[i] = out_of[find(slot[i])];
        segs_of[m.line_map[i]].push_back(i);
    }
    // ---- stage 3
    m.leader_line.resize(m.info.size());
    std::vector<uint32_t> live;
    for (size_t o = 0; o < m.info.size(); ++o) {
        if (m.info[o].n_members == 1) {
            for (uint32_t i : segs_of[o]) m.segs.insert(m.segs.end(), segs + 6 * (size_t)i, segs + 6 * (size_t)i + 6);
            m.leader_line[o] = m.info[o].label;
        } else {
            live.clear();
            for (uint32_t i : segs_of[o]) {
                const double* v = segs + 6 * (size_t)i;
                const double ex = v[3] - v[0], ey = v[4] - v[1], ez = v[5] - v[2];
                if (ex * ex + ey * ey + ez * ez > 0.0) live.push_back(i);
            }
            uint32_t leader = 0;
            fuse(segs, live, m, m.info[o].max_offset, leader);
            m.leader_line[o] = line[leader];
        }
        m.seg_begin.push_back((uint32_t)(m.segs.size() / 6));
        m.seg_line.resize(m.segs.size() / 6, (uint32_t)o);
    }
    l3d_merge_summary& s = m.sum;
    s.n_segments_in = n; s.n_segments_out = m.seg_line.size();
    s.n_lines_in = ids.size(); s.n_lines_out = m.info.size();
    s.n_pairs = pairs.size();
    for (const l3d_merge_line_info& L : m.info) {
        if (L.n_members >= 2) ++s.n_merged_components;
        if (L.n_members > s.largest_component) s.largest_component = L.n_members;
        if (L.max_offset > s.max_offset) s.max_offset = L.max_offset;
    }
    for (uint32_t i = 0; i < n; ++i) s.length_in += length_of(segs + 6 * (size_t)i);
    for (size_t i = 0; i < m.seg_line.size(); ++i) s.length_out += length_of(m.segs.data() + 6 * i);
}

uint32_t distinct_lines(uint32_t n, const uint32_t* line) {
    std::vector<uint32_t> ids(line, line + n);
    std::sort(ids.begin(), ids.end());
    return (uint32_t)(std::unique(ids.begin(), ids.end()) - ids.begin());
}

}  // namespace

extern "C" {

int l3d_merge_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_merge_params* params,
                       uint32_t* out_line_map, uint32_t out_seg_cap, double* out_segs6, uint32_t* out_seg_line,
                       uint32_t* out_n_segs, uint32_t out_line_cap, l3d_merge_line_info* out_line_info, uint32_t* out_n_lines,
                       l3d_merge_summary* summary) {
    if (int rc = check_params(params)) return rc;
    if (!out_n_segs || !out_n_lines) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_model(nullptr, n, segs6, line)) return rc;
    if (n && (!out_line_map || !out_segs6 || !out_seg_line || !out_line_info)) return fail(L3D_ERR_ARG, "null argument");
    if (out_seg_cap < n) return fail(L3D_ERR_ARG, "out_seg_cap is smaller than the number of segments");
    if (n && out_line_cap < distinct_lines(n, line)) return fail(L3D_ERR_ARG, "out_line_cap is smaller than the number of distinct lines");
    Merged m;
    if (n) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        std::vector<MrgPair> pairs;
        if (int rc = merge_pairs(w, 0, n, segs6, line, *params, pairs, nullptr)) return rc;
        merge_host(n, segs6, line, pairs, m);
        std::memcpy(out_line_map, m.line_map.data(), 4 * (size_t)n);
        std::memcpy(out_segs6, m.segs.data(), 8 * m.segs.size());
        std::memcpy(out_seg_line, m.seg_line.data(), 4 * m.seg_line.size());
        std::memcpy(out_line_info, m.info.data(), sizeof(l3d_merge_line_info) * m.info.size());
    }
    *out_n_segs = (uint32_t)m.seg_line.size();
    *out_n_lines = (uint32_t)m.info.size();
    if (summary) *summary = m.sum;
    return L3D_OK;
}

int l3d_merge_lines(l3d_ctx* c, const l3d_merge_params* params, l3d_merge_summary* summary) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "lines are merged", "merge")) return rc;
    std::vector<double> P6; std::vector<uint32_t> line;
    context_segments(c, P6, line);
    if (int rc = check_model(nullptr, line.size(), P6.data(), line.data())) return rc;
    const uint32_t n = (uint32_t)line.size();
    Merged m;
    if (n) {
        if (int rc = set_device(c->device)) return rc;
        float ms = 0.0f;
        const bool timed = c->timing_level >= 2;
        std::vector<MrgPair> pairs;
        if (int rc = merge_pairs(c->proj, c->stream, n, P6.data(), line.data(), *params, pairs, timed ? &ms : nullptr)) return rc;
        if (timed) g_mrg_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
        merge_host(n, P6.data(), line.data(), pairs, m);
    }
    // the merged model takes the place of lines3D_ (a line without segments -- reconstruct3Dlines makes none -- is in no
    // flattening and leaves with this)
    std::vector<ReconLine> out(m.info.size());
    for (size_t o = 0; o < m.info.size(); ++o) {
        if (m.info[o].n_members == 1) { out[o] = std::move(c->lines3D[m.info[o].label]); continue; }
        ReconLine& L = out[o];
        const uint32_t s0 = m.seg_begin[o], s1 = m.seg_begin[o + 1];
        auto seg = [&](const double* a, const double* b) {
            const d3 P1{a[0], a[1], a[2]}, P2{b[0], b[1], b[2]};
            ReconSeg3D s = segment3d(P1, P2);
            s.P1 = P1; s.P2 = P2;
            return s;
        };
        for (uint32_t k = s0; k < s1; ++k) L.collinear.push_back(seg(&m.segs[6 * (size_t)k], &m.segs[6 * (size_t)k + 3]));
        L.cluster_seg = seg(&m.segs[6 * (size_t)s0], &m.segs[6 * (size_t)(s1 - 1) + 3]);
        for (uint32_t id : m.members[o]) L.residuals.insert(L.residuals.end(), c->lines3D[id].residuals.begin(), c->lines3D[id].residuals.end());
        L.reference_view = c->lines3D[m.leader_line[o]].reference_view;
    }
    c->lines3D.swap(out);
    c->proj_records.clear();                               // (they name the lines of the model that has just been replaced)
    c->lines_merged = true;
    c->merged_distance = params->max_distance;
    if (summary) *summary = m.sum;
    return L3D_OK;
}

}  // extern "C"
