// l3d_planes.h -- stages 0 and 3 of the plane detection: the integer weights of the segments, and the
// selection of the planes from the hypotheses and the scores that k_planes.hip yields.  Host code: the selection is
// sequential and touches a few candidates (the rationale of l3d_wireframe.h).  Plain C++17 without a HIP include (g++
// compiles it for tests/test_planes_host.py); fp64 in the order DESIGN §25 writes it -- build with -ffp-contract=off --
// so that tests/planes_model.py follows it operation for operation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/l3dpp_hip.h"

namespace l3d {

// what the device yields per hypothesis, in the junctions' (a, b) order; a dead one is all zero but for a and b
struct PlHyp { double N[3], J[3]; uint32_t a, b, live, pad; };
static_assert(sizeof(PlHyp) == 64, "plane hypothesis layout");
static_assert(sizeof(l3d_planes_params) == 64 && sizeof(l3d_pl_plane) == 264 && sizeof(l3d_pl_member) == 8 &&
              sizeof(l3d_pl_score) == 16 && sizeof(l3d_planes_summary) == 136, "planes structs");

constexpr int kPlJacobiSweeps = 8;
constexpr uint64_t kPlMaxHypotheses = 1ull << 24;

struct PlResult {
    std::vector<l3d_pl_plane> planes;
    std::vector<l3d_pl_member> members;
    std::vector<uint32_t> seg_planes;       // [n]
    std::vector<l3d_pl_score> scores;       // [n_hypotheses]
    l3d_planes_summary sum{};
};

// ---- stage 0: the lengths, their sequential total, the scale exponent and the integer weights
struct PlWeights {
    std::vector<double> len;                // [n] sqrt(E2)
    std::vector<uint64_t> q;                // [n] floor(len * 2^e); 0 for a point
    std::vector<uint8_t> live;              // [n] E2 > 0
    double length_total = 0.0;
    int e = 0;
    uint64_t n_points = 0;
};
inline void pl_weights(uint32_t n, const double* segs, PlWeights& w) {
    w = PlWeights();
    w.len.resize(n); w.q.assign(n, 0); w.live.assign(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const double* v = segs + 6 * (size_t)i;
        const double ex = v[3] - v[0], ey = v[4] - v[1], ez = v[5] - v[2];
        const double E2 = (ex * ex + ey * ey) + ez * ez;
        w.len[i] = std::sqrt(E2);
        w.live[i] = E2 > 0.0;
        if (!w.live[i]) ++w.n_points;
        w.length_total += w.len[i];
    }
    if (!n) return;
    int x = 0;
    (void)std::frexp(w.length_total, &x);
    w.e = 52 - x;
    for (uint32_t i = 0; i < n; ++i)
        if (w.live[i]) w.q[i] = (uint64_t)std::floor(std::ldexp(w.len[i], w.e));
}

inline double pl_dot(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// The Jacobi of DESIGN §25 on the symmetric 3 x 3 S = {xx, xy, xz, yy, yz, zz}: kPlJacobiSweeps cyclic sweeps over (0,1),
// (0,2), (1,2), the rotation as §25 writes it.  -> A, whose diagonal holds the eigenvalues, and V, whose columns are the
// eigenvectors.  Shared by the planes' refit (the smallest) and the directions' (the largest, l3d_directions.h).
inline void pl_jacobi(const double S[6], double A[3][3], double V[3][3]) {
    const double A0[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[i][j] = A0[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2}, R[3] = {2, 1, 0};
    for (int sweep = 0; sweep < kPlJacobiSweeps; ++sweep)
        for (int k = 0; k < 3; ++k) {
            const int p = P[k], q = Q[k], r = R[k];
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double root = std::sqrt(theta * theta + 1.0);
            const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);
            const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
            A[p][p] = A[p][p] - t * apq;
            A[q][q] = A[q][q] + t * apq;
            A[p][q] = 0.0; A[q][p] = 0.0;
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
            A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
            for (int i = 0; i < 3; ++i) {
                const double vip = V[i][p], viq = V[i][q];
                V[i][p] = c * vip - s * viq;
                V[i][q] = s * vip + c * viq;
            }
        }
}
// column m of V, divided by its length
inline void pl_unit_column(const double V[3][3], int m, double out[3]) {
    const double v[3] = {V[0][m], V[1][m], V[2][m]};
    const double len = std::sqrt(pl_dot(v, v));
    out[0] = v[0] / len; out[1] = v[1] / len; out[2] = v[2] / len;
}
// The eigenvector of the smallest eigenvalue: the column of the smallest diagonal entry (the first of equals), divided by
// its length.
inline void pl_smallest_eigenvector(const double S[6], double out[3]) {
    double A[3][3], V[3][3];
    pl_jacobi(S, A, V);
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    pl_unit_column(V, m, out);
}

// the inliers of a plane (N, J) among the live segments, ascending: stage 2's test
inline void pl_members(uint32_t n, const double* segs, const PlWeights& w, const double N[3], const double J[3], double max_distance,
                       std::vector<uint32_t>& out) {
    out.clear();
    for (uint32_t s = 0; s < n; ++s) {
        if (!w.live[s]) continue;
        const double* v = segs + 6 * (size_t)s;
        const double u1[3] = {v[0] - J[0], v[1] - J[1], v[2] - J[2]}, u2[3] = {v[3] - J[0], v[4] - J[1], v[5] - J[2]};
        const double h1 = pl_dot(N, u1), h2 = pl_dot(N, u2);
        if (std::fabs(h1) <= max_distance && std::fabs(h2) <= max_distance) out.push_back(s);
    }
}

// root mean square of the 2 n end-point distances h = N.(p - O) of the members
inline double pl_rms(const double* segs, const std::vector<uint32_t>& mem, const double N[3], const double O[3]) {
    double acc = 0.0;
    for (uint32_t s : mem) {
        const double* v = segs + 6 * (size_t)s;
        const double u1[3] = {v[0] - O[0], v[1] - O[1], v[2] - O[2]}, u2[3] = {v[3] - O[0], v[4] - O[1], v[5] - O[2]};
        const double h1 = pl_dot(N, u1), h2 = pl_dot(N, u2);
        acc += h1 * h1 + h2 * h2;
    }
    return std::sqrt(acc / (2.0 * (double)mem.size()));
}

// step 3: the record of an accepted plane
inline l3d_pl_plane pl_describe(const double* segs, const uint32_t* line, const PlWeights& w, uint32_t index, const PlHyp& h,
                                uint64_t weight, const std::vector<uint32_t>& mem) {
    l3d_pl_plane P{};
    P.hypothesis = index; P.a = h.a; P.b = h.b; P.n_segments = (uint32_t)mem.size(); P.weight = weight;
    for (int c = 0; c < 3; ++c) { P.N[c] = h.N[c]; P.J[c] = h.J[c]; }
    P.d = pl_dot(h.N, h.J);
    std::vector<uint32_t> lines;
    for (uint32_t s : mem) { lines.push_back(line[s]); P.length += w.len[s]; }
    std::sort(lines.begin(), lines.end());
    P.n_lines = (uint32_t)(std::unique(lines.begin(), lines.end()) - lines.begin());
    P.rms = pl_rms(segs, mem, h.N, h.J);
    // the refit: centroid, scatter, smallest eigenvector
    const double count = 2.0 * (double)mem.size();
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t s : mem)
        for (int end = 0; end < 2; ++end)
            for (int c = 0; c < 3; ++c) sum[c] += segs[6 * (size_t)s + 3 * end + c];
    for (int c = 0; c < 3; ++c) P.centroid[c] = sum[c] / count;
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t s : mem)
        for (int end = 0; end < 2; ++end) {
            const double* p = segs + 6 * (size_t)s + 3 * end;
            const double dx = p[0] - P.centroid[0], dy = p[1] - P.centroid[1], dz = p[2] - P.centroid[2];
            S[0] += dx * dx; S[1] += dx * dy; S[2] += dx * dz; S[3] += dy * dy; S[4] += dy * dz; S[5] += dz * dz;
        }
    pl_smallest_eigenvector(S, P.N_fit);
    if (!(pl_dot(P.N_fit, h.N) >= 0.0)) for (int c = 0; c < 3; ++c) P.N_fit[c] = -P.N_fit[c];
    P.d_fit = pl_dot(P.N_fit, P.centroid);
    P.rms_fit = pl_rms(segs, mem, P.N_fit, P.centroid);
    // the patch
    const double* va = segs + 6 * (size_t)h.a;
    const double ea[3] = {va[3] - va[0], va[4] - va[1], va[5] - va[2]};
    const double La = std::sqrt(pl_dot(ea, ea));
    const double U[3] = {ea[0] / La, ea[1] / La, ea[2] / La};
    const double V[3] = {h.N[1] * U[2] - h.N[2] * U[1], h.N[2] * U[0] - h.N[0] * U[2], h.N[0] * U[1] - h.N[1] * U[0]};
    double lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
    bool first = true;
    for (uint32_t s : mem)
        for (int end = 0; end < 2; ++end) {
            const double* p = segs + 6 * (size_t)s + 3 * end;
            const double u[3] = {p[0] - h.J[0], p[1] - h.J[1], p[2] - h.J[2]};
            const double cu = pl_dot(u, U), cv = pl_dot(u, V);
            if (first) { lo[0] = hi[0] = cu; lo[1] = hi[1] = cv; first = false; continue; }
            if (cu < lo[0]) lo[0] = cu;
            if (cu > hi[0]) hi[0] = cu;
            if (cv < lo[1]) lo[1] = cv;
            if (cv > hi[1]) hi[1] = cv;
        }
    const double cu[4] = {lo[0], hi[0], hi[0], lo[0]}, cv[4] = {lo[1], lo[1], hi[1], hi[1]};
    for (int k = 0; k < 4; ++k)
        for (int c = 0; c < 3; ++c) P.corners[k][c] = (h.J[c] + cu[k] * U[c]) + cv[k] * V[c];
    return P;
}

// Stage 3.  segs [n x 6], line [n]; hyp, score [n_h]: the device's records, every index below n.  -> 0, or 1 where the
// members recomputed for a tested hypothesis differ from the device's score: *bad is that hypothesis.
inline int pl_select(uint32_t n, const double* segs, const uint32_t* line, const l3d_planes_params& par, const PlWeights& w,
                     const PlHyp* hyp, const l3d_pl_score* score, size_t n_h, PlResult& r, size_t* bad) {
    r = PlResult();
    l3d_planes_summary& s = r.sum;
    r.seg_planes.assign(n, 0);
    r.scores.assign(score, score + n_h);
    s.n_segments = n; s.n_point_segments = w.n_points; s.n_hypotheses = n_h;
    s.scale_exponent = w.e; s.length_total = w.length_total;
    // 1. the candidates
    std::vector<uint32_t> cand;
    for (size_t h = 0; h < n_h; ++h) {
        if (!hyp[h].live) { ++s.n_dead; continue; }
        if (score[h].count >= par.min_segments && std::ldexp((double)score[h].weight, -w.e) >= par.min_length) cand.push_back((uint32_t)h);
    }
    s.n_candidates = cand.size();
    std::sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) {
        return score[x].weight != score[y].weight ? score[x].weight > score[y].weight
               : score[x].count != score[y].count ? score[x].count > score[y].count : x < y; });
    // 2. the walk
    std::vector<std::vector<uint8_t>> in_plane;              // [plane][segment]
    std::vector<uint32_t> mem;
    for (uint32_t h : cand) {
        if (r.planes.size() >= par.max_planes) break;
        const PlHyp& H = hyp[h];
        bool dropped = false;
        for (const std::vector<uint8_t>& m : in_plane) if (m[H.a] && m[H.b]) { dropped = true; break; }
        if (dropped) { ++s.n_dropped; continue; }
        if (s.n_tested == par.max_tests) { s.truncated = 1; break; }
        ++s.n_tested;
        pl_members(n, segs, w, H.N, H.J, par.max_distance, mem);
        uint64_t weight = 0;
        for (uint32_t m : mem) weight += w.q[m];
        if (mem.size() != score[h].count || weight != score[h].weight) { if (bad) *bad = h; return 1; }
        bool rejected = false;
        for (const std::vector<uint8_t>& m : in_plane) {
            uint64_t common = 0;
            for (uint32_t i : mem) if (m[i]) common += w.q[i];
            if (2 * common > weight) { rejected = true; break; }
        }
        if (rejected) { ++s.n_rejected; continue; }
        const uint32_t number = (uint32_t)r.planes.size();
        r.planes.push_back(pl_describe(segs, line, w, h, H, weight, mem));
        in_plane.emplace_back(n, (uint8_t)0);
        for (uint32_t i : mem) { in_plane.back()[i] = 1; r.members.push_back(l3d_pl_member{number, i}); ++r.seg_planes[i]; }
        if (r.planes.back().rms > s.max_rms) s.max_rms = r.planes.back().rms;
    }
    // 5. the summary
    s.n_planes = r.planes.size(); s.n_memberships = r.members.size();
    for (uint32_t i = 0; i < n; ++i) {
        if (!r.seg_planes[i]) continue;
        ++s.n_segments_in_planes;
        if (r.seg_planes[i] > 1) ++s.n_segments_in_several;
        s.length_in_planes += w.len[i];
    }
    return 0;
}

}  // namespace l3d
