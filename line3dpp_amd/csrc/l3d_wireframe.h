// l3d_wireframe.h -- stage 2 of the wireframe: the graph built from the junction records of k_wireframe.hip.
// Host code: the junctions are few and the work is sequential (the rationale of l3d_recon.h and of §19's stage 2).  Plain
// C++17 without a HIP include (g++ compiles it for tests/test_wireframe_host.py); fp64 in the order DESIGN §24 writes it
// -- build with -ffp-contract=off -- so that tests/wireframe_model.py follows it operation for operation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/l3dpp_hip.h"

namespace l3d {

// what the device yields per junction, in ascending (a, b) order
struct WfRecord { uint32_t a, b; double sa, sb, gap2; };
static_assert(sizeof(WfRecord) == 32, "junction record layout");
static_assert(sizeof(l3d_wireframe_params) == 32 && sizeof(l3d_wf_junction) == 72 && sizeof(l3d_wf_vertex) == 48 &&
              sizeof(l3d_wf_edge) == 16 && sizeof(l3d_wireframe_summary) == 120, "wireframe structs");

struct WfGraph {
    std::vector<l3d_wf_junction> junctions;
    std::vector<l3d_wf_vertex> vertices;
    std::vector<l3d_wf_edge> edges;
    l3d_wireframe_summary sum{};
};

// union-find in which the smaller index becomes the root, so that a root is the smallest member of its set
struct WfSets {
    std::vector<uint32_t> parent;
    explicit WfSets(size_t n) : parent(n) { for (size_t k = 0; k < n; ++k) parent[k] = (uint32_t)k; }
    uint32_t find(uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    }
    void join(uint32_t x, uint32_t y) {
        const uint32_t a = find(x), b = find(y);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;
    }
};

// end class of the point t along a segment of length L (step 2)
inline uint32_t wf_end_class(double t, double L, double max_extension) {
    const bool at1 = t <= max_extension, at2 = t >= L - max_extension;
    if (at1 && at2) return t * 2.0 <= L ? L3D_WF_AT_P1 : L3D_WF_AT_P2;
    return at1 ? L3D_WF_AT_P1 : at2 ? L3D_WF_AT_P2 : L3D_WF_INTERIOR;
}

// segs [n x 6], line [n]; rec [n_rec]: the junctions of stage 1, every index below n.  Steps 1-9 of stage 2.
inline void wf_graph(uint32_t n, const double* segs, const uint32_t* line, double max_distance, double max_extension,
                     const WfRecord* rec, size_t n_rec, WfGraph& g) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    g = WfGraph();
    l3d_wireframe_summary& s = g.sum;
    s.n_segments = n; s.n_junctions = n_rec;
    std::vector<double> len(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double* v = segs + 6 * (size_t)i;
        const double ex = v[3] - v[0], ey = v[4] - v[1], ez = v[5] - v[2];
        const double E2 = ex * ex + ey * ey + ez * ez;
        len[i] = std::sqrt(E2);
        if (!(E2 > 0.0)) ++s.n_point_segments;
        s.length_total += len[i];
    }
    // 1.-3. the junctions; an attachment = where a junction lies on one of its two segments
    struct Att { uint32_t seg; double t; uint32_t junction; };
    std::vector<Att> inner;                                  // the interior attachments
    std::vector<uint32_t> end_first(2 * (size_t)n, kNone);   // [2 * segment + end] the first junction at that end
    WfSets sets(n_rec);
    g.junctions.resize(n_rec);
    for (size_t k = 0; k < n_rec; ++k) {
        const WfRecord& r = rec[k];
        l3d_wf_junction& j = g.junctions[k];
        const double* va = segs + 6 * (size_t)r.a;
        const double* vb = segs + 6 * (size_t)r.b;
        j.a = r.a; j.b = r.b; j.sa = r.sa; j.sb = r.sb;
        for (int c = 0; c < 3; ++c) {
            const double pa = va[c] + r.sa * (va[c + 3] - va[c]), pb = vb[c] + r.sb * (vb[c + 3] - vb[c]);
            j.J[c] = (pa + pb) * 0.5;
        }
        j.gap = std::sqrt(r.gap2);
        if (j.gap > s.max_gap) s.max_gap = j.gap;
        const double t[2] = {r.sa * len[r.a], r.sb * len[r.b]};
        const uint32_t seg[2] = {r.a, r.b};
        uint32_t cls[2];
        for (int side = 0; side < 2; ++side) {
            cls[side] = wf_end_class(t[side], len[seg[side]], max_extension);
            if (cls[side] == L3D_WF_INTERIOR) { inner.push_back(Att{seg[side], t[side], (uint32_t)k}); continue; }
            uint32_t& first = end_first[2 * (size_t)seg[side] + cls[side]];                   // 4. the same end of a segment
            if (first == kNone) first = (uint32_t)k; else sets.join(first, (uint32_t)k);
        }
        j.class_a = cls[0]; j.class_b = cls[1];
        const int ends = (cls[0] != L3D_WF_INTERIOR) + (cls[1] != L3D_WF_INTERIOR);
        j.kind = ends == 2 ? L3D_WF_L : ends == 1 ? L3D_WF_T : L3D_WF_X;
        ++(ends == 2 ? s.n_L : ends == 1 ? s.n_T : s.n_X);
    }
    // 4. the sweep along every segment's interior
    std::sort(inner.begin(), inner.end(), [](const Att& x, const Att& y) {
        return x.seg != y.seg ? x.seg < y.seg : x.t != y.t ? x.t < y.t : x.junction < y.junction; });
    for (size_t k = 1; k < inner.size(); ++k)
        if (inner[k].seg == inner[k - 1].seg && inner[k].t - inner[k - 1].t <= max_distance) sets.join(inner[k - 1].junction, inner[k].junction);
    // 5. the junction vertices, numbered by their smallest member
    std::vector<uint32_t> vertex_of_root(n_rec, kNone);
    for (size_t k = 0; k < n_rec; ++k)
        if (sets.find((uint32_t)k) == k) { vertex_of_root[k] = (uint32_t)g.vertices.size(); g.vertices.push_back(l3d_wf_vertex{}); }
    for (size_t k = 0; k < n_rec; ++k) {                     // (ascending: the sums run in junction order)
        l3d_wf_junction& j = g.junctions[k];
        j.vertex = vertex_of_root[sets.find((uint32_t)k)];
        l3d_wf_vertex& v = g.vertices[j.vertex];
        v.P[0] += j.J[0]; v.P[1] += j.J[1]; v.P[2] += j.J[2];
        ++v.n_junctions; v.kinds |= j.kind;
    }
    for (l3d_wf_vertex& v : g.vertices) {
        const double count = (double)v.n_junctions;
        v.P[0] /= count; v.P[1] /= count; v.P[2] /= count;
    }
    for (const l3d_wf_junction& j : g.junctions) {
        l3d_wf_vertex& v = g.vertices[j.vertex];
        const double dx = j.J[0] - v.P[0], dy = j.J[1] - v.P[1], dz = j.J[2] - v.P[2];
        const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (d > v.spread) v.spread = d;
    }
    s.n_junction_vertices = g.vertices.size();
    for (const l3d_wf_vertex& v : g.vertices) if (v.spread > s.max_spread) s.max_spread = v.spread;
    // 6. the free ends, in (segment, end) order
    std::vector<uint32_t> end_vertex(2 * (size_t)n, kNone);
    for (uint32_t i = 0; i < n; ++i) {
        if (!(len[i] > 0.0)) continue;                       // (sqrt(E2) > 0 iff E2 > 0)
        for (int end = 0; end < 2; ++end) {
            const uint32_t first = end_first[2 * (size_t)i + end];
            if (first != kNone) { end_vertex[2 * (size_t)i + end] = g.junctions[first].vertex; continue; }
            const double* p = segs + 6 * (size_t)i + 3 * end;
            end_vertex[2 * (size_t)i + end] = (uint32_t)g.vertices.size();
            g.vertices.push_back(l3d_wf_vertex{{p[0], p[1], p[2]}, 0.0, 0u, 0u, 0u, 0u});
            ++s.n_free_ends;
        }
    }
    s.n_vertices = g.vertices.size();
    // 7. the edges: the stops of every live segment
    struct Stop { double t; uint32_t vertex; };
    std::vector<Stop> stops;
    size_t at = 0;                                           // inner is sorted by segment
    for (uint32_t i = 0; i < n; ++i) {
        stops.clear();
        for (; at < inner.size() && inner[at].seg == i; ++at) stops.push_back(Stop{inner[at].t, g.junctions[inner[at].junction].vertex});
        if (!(len[i] > 0.0)) continue;
        // a vertex once, at the smallest t of its attachments, then by (t, vertex)
        std::sort(stops.begin(), stops.end(), [](const Stop& x, const Stop& y) { return x.vertex != y.vertex ? x.vertex < y.vertex : x.t < y.t; });
        stops.erase(std::unique(stops.begin(), stops.end(), [](const Stop& x, const Stop& y) { return x.vertex == y.vertex; }), stops.end());
        std::sort(stops.begin(), stops.end(), [](const Stop& x, const Stop& y) { return x.t != y.t ? x.t < y.t : x.vertex < y.vertex; });
        uint32_t prev = end_vertex[2 * (size_t)i];
        auto step = [&](uint32_t v) {
            if (v != prev) {
                g.edges.push_back(l3d_wf_edge{prev, v, i, line[i]});
                ++g.vertices[prev].degree; ++g.vertices[v].degree;
            }
            prev = v;
        };
        for (const Stop& x : stops) step(x.vertex);
        step(end_vertex[2 * (size_t)i + 1]);
    }
    s.n_edges = g.edges.size();
    // 8. the connected components, numbered by their smallest vertex
    WfSets comp(g.vertices.size());
    for (const l3d_wf_edge& e : g.edges) comp.join(e.v0, e.v1);
    std::vector<uint32_t> number(g.vertices.size(), kNone);
    for (size_t v = 0; v < g.vertices.size(); ++v)
        if (comp.find((uint32_t)v) == v) number[v] = (uint32_t)s.n_components++;
    for (size_t v = 0; v < g.vertices.size(); ++v) g.vertices[v].component = number[comp.find((uint32_t)v)];
    std::vector<uint64_t> edges_of(s.n_components, 0);
    for (const l3d_wf_edge& e : g.edges) ++edges_of[g.vertices[e.v0].component];
    for (uint64_t c : edges_of) if (c > s.largest_component) s.largest_component = c;
}

}  // namespace l3d
