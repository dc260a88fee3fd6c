// l3d_directions.h -- stage 3 of the direction detection: the selection of the directions from the scores that
// k_directions.hip yields, their refit and the frame.  Stage 0, the integer weights, is pl_weights of l3d_planes.h, and
// the refit shares its Jacobi.  Host code: the selection is sequential and touches a few candidates (the rationale of
// l3d_planes.h).  Plain C++17 without a HIP include (g++ compiles it for tests/test_directions_host.py); fp64 in the
// order DESIGN §26 writes it -- build with -ffp-contract=off -- so that tests/directions_model.py follows it operation for
// operation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "l3d_planes.h"

namespace l3d {

static_assert(sizeof(l3d_directions_params) == 64 && sizeof(l3d_dir_direction) == 136 && sizeof(l3d_dir_member) == 8 &&
              sizeof(l3d_dir_score) == 16 && sizeof(l3d_directions_summary) == 200, "directions structs");

constexpr uint32_t kDirNone = 0xFFFFFFFFu;  // an unused slot of the frame

// no direction: no axis, every slot unused, R the identity
inline void dir_no_frame(l3d_directions_summary& s) {
    s.frame_axes = 0; s.frame[0] = s.frame[1] = s.frame[2] = kDirNone;
    for (int k = 0; k < 9; ++k) s.R[k] = k % 4 == 0 ? 1.0 : 0.0;
}

struct DirResult {
    std::vector<l3d_dir_direction> directions;
    std::vector<l3d_dir_member> members;
    std::vector<uint32_t> seg_directions;   // [n]
    std::vector<l3d_dir_score> scores;      // [n]: hypothesis h is segment h
    l3d_directions_summary sum{};
    DirResult() { dir_no_frame(sum); }
};

// x × y, each component x·y' − y·x'
inline void dir_cross(const double* x, const double* y, double out[3]) {
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}
// the squared sine of the angle between two unit vectors: |x × y|^2
inline double dir_sin2(const double* x, const double* y) {
    double X[3];
    dir_cross(x, y, X);
    return pl_dot(X, X);
}

// stage 1 on the host: D [3 n], e / sqrt(E2) per component for a live segment, 0 for a point
inline void dir_units(uint32_t n, const double* segs, const PlWeights& w, std::vector<double>& D) {
    D.assign(3 * (size_t)n, 0.0);
    for (uint32_t i = 0; i < n; ++i) {
        if (!w.live[i]) continue;
        const double* v = segs + 6 * (size_t)i;
        for (int c = 0; c < 3; ++c) D[3 * (size_t)i + c] = (v[3 + c] - v[c]) / w.len[i];
    }
}

// The eigenvector of the largest eigenvalue of S = {xx, xy, xz, yy, yz, zz}, by §25's Jacobi: the column of the largest
// diagonal entry (the first of equals), divided by its length.
inline void dir_largest_eigenvector(const double S[6], double out[3]) {
    double A[3][3], V[3][3];
    pl_jacobi(S, A, V);
    int m = 0;
    if (A[1][1] > A[m][m]) m = 1;
    if (A[2][2] > A[m][m]) m = 2;
    pl_unit_column(V, m, out);
}

// the inliers of direction Dh among the live segments, ascending: stage 2's test on the host's D
inline void dir_members(uint32_t n, const PlWeights& w, const std::vector<double>& D, const double* Dh, double max_sin2,
                        std::vector<uint32_t>& out) {
    out.clear();
    for (uint32_t s = 0; s < n; ++s)
        if (w.live[s] && dir_sin2(Dh, &D[3 * (size_t)s]) <= max_sin2) out.push_back(s);
}

inline double dir_rms_sin(const std::vector<double>& D, const std::vector<uint32_t>& mem, const double* axis) {
    double acc = 0.0;
    for (uint32_t s : mem) acc += dir_sin2(axis, &D[3 * (size_t)s]);
    return std::sqrt(acc / (double)mem.size());
}

// step 3: the record of an accepted direction
inline l3d_dir_direction dir_describe(const double* segs, const uint32_t* line, const PlWeights& w, const std::vector<double>& D,
                                      uint32_t h, uint64_t weight, const std::vector<uint32_t>& mem) {
    l3d_dir_direction P{};
    const double* Dh = &D[3 * (size_t)h];
    P.hypothesis = h; P.n_segments = (uint32_t)mem.size(); P.weight = weight;
    for (int c = 0; c < 3; ++c) P.D[c] = Dh[c];
    std::vector<uint32_t> lines;
    for (uint32_t s : mem) { lines.push_back(line[s]); P.length += w.len[s]; }
    std::sort(lines.begin(), lines.end());
    P.n_lines = (uint32_t)(std::unique(lines.begin(), lines.end()) - lines.begin());
    P.rms_sin = dir_rms_sin(D, mem, Dh);
    // the refit: the length-weighted scatter of the members' directions, its largest eigenvector
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t s : mem) {
        const double* d = &D[3 * (size_t)s];
        const double L = w.len[s];
        S[0] += L * (d[0] * d[0]); S[1] += L * (d[0] * d[1]); S[2] += L * (d[0] * d[2]);
        S[3] += L * (d[1] * d[1]); S[4] += L * (d[1] * d[2]); S[5] += L * (d[2] * d[2]);
    }
    dir_largest_eigenvector(S, P.D_fit);
    if (pl_dot(P.D_fit, Dh) < 0.0) for (int c = 0; c < 3; ++c) P.D_fit[c] = -P.D_fit[c];
    P.rms_sin_fit = dir_rms_sin(D, mem, P.D_fit);
    // the extent along the refit, about the centroid of the members' end points
    const double count = 2.0 * (double)mem.size();
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t s : mem)
        for (int end = 0; end < 2; ++end)
            for (int c = 0; c < 3; ++c) sum[c] += segs[6 * (size_t)s + 3 * end + c];
    for (int c = 0; c < 3; ++c) P.centroid[c] = sum[c] / count;
    bool first = true;
    for (uint32_t s : mem)
        for (int end = 0; end < 2; ++end) {
            const double* p = segs + 6 * (size_t)s + 3 * end;
            const double u[3] = {p[0] - P.centroid[0], p[1] - P.centroid[1], p[2] - P.centroid[2]};
            const double t = pl_dot(u, P.D_fit);
            if (first) { P.t_min = P.t_max = t; first = false; continue; }
            if (t < P.t_min) P.t_min = t;
            if (t > P.t_max) P.t_max = t;
        }
    return P;
}

// step 5: the frame among the first min(n_directions, frame_search) directions
inline void dir_frame(const std::vector<l3d_dir_direction>& dir, const l3d_directions_params& par, l3d_directions_summary& s) {
    dir_no_frame(s);
    if (dir.empty()) return;
    const uint32_t F = (uint32_t)std::min<size_t>(dir.size(), par.frame_search);
    auto orthogonal = [&](uint32_t i, uint32_t j) {
        const double c = pl_dot(dir[i].D_fit, dir[j].D_fit);
        return c * c <= par.max_frame_cos2;
    };
    uint32_t pick[3] = {0u, kDirNone, kDirNone};
    uint32_t axes = 1;
    uint64_t best = 0;
    for (uint32_t i = 0; i < F; ++i)
        for (uint32_t j = i + 1; j < F; ++j) {
            if (!orthogonal(i, j)) continue;
            for (uint32_t k = j + 1; k < F; ++k) {
                if (!orthogonal(i, k) || !orthogonal(j, k)) continue;
                const uint64_t sum = dir[i].weight + dir[j].weight + dir[k].weight;
                if (axes < 3 || sum > best) { axes = 3; best = sum; pick[0] = i; pick[1] = j; pick[2] = k; }
            }
        }
    if (axes < 3)
        for (uint32_t i = 0; i < F; ++i)
            for (uint32_t j = i + 1; j < F; ++j) {
                if (!orthogonal(i, j)) continue;
                const uint64_t sum = dir[i].weight + dir[j].weight;
                if (axes < 2 || sum > best) { axes = 2; best = sum; pick[0] = i; pick[1] = j; }
            }
    s.frame_axes = axes;
    for (int k = 0; k < 3; ++k) s.frame[k] = pick[k];
    const double* x = dir[pick[0]].D_fit;
    double second[3] = {0.0, 0.0, 0.0};
    if (axes >= 2) {
        for (int c = 0; c < 3; ++c) second[c] = dir[pick[1]].D_fit[c];
    } else {
        int m = 0;
        if (std::fabs(x[1]) < std::fabs(x[m])) m = 1;
        if (std::fabs(x[2]) < std::fabs(x[m])) m = 2;
        second[m] = 1.0;
    }
    const double along = pl_dot(second, x);
    const double yp[3] = {second[0] - along * x[0], second[1] - along * x[1], second[2] - along * x[2]};
    const double len = std::sqrt(pl_dot(yp, yp));
    const double y[3] = {yp[0] / len, yp[1] / len, yp[2] / len};
    double z[3];
    dir_cross(x, y, z);
    for (int c = 0; c < 3; ++c) { s.R[c] = x[c]; s.R[3 + c] = y[c]; s.R[6 + c] = z[c]; }
}

// Stage 3.  segs [n x 6], line [n]; score [n]: the device's cells, hypothesis h = segment h.  -> 0, or 1 where the members
// recomputed for a tested hypothesis differ from the device's score: *bad is that hypothesis.
inline int dir_select(uint32_t n, const double* segs, const uint32_t* line, const l3d_directions_params& par, const PlWeights& w,
                      const l3d_dir_score* score, DirResult& r, size_t* bad) {
    r = DirResult();
    l3d_directions_summary& s = r.sum;
    r.seg_directions.assign(n, 0);
    r.scores.assign(score, score + n);
    s.n_segments = n; s.n_point_segments = w.n_points;
    s.scale_exponent = w.e; s.length_total = w.length_total;
    std::vector<double> D;
    dir_units(n, segs, w, D);
    // 1. the candidates
    std::vector<uint32_t> cand;
    for (uint32_t h = 0; h < n; ++h)
        if (w.live[h] && score[h].count >= par.min_segments && std::ldexp((double)score[h].weight, -w.e) >= par.min_length) cand.push_back(h);
    s.n_candidates = cand.size();
    std::sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) {
        return score[x].weight != score[y].weight ? score[x].weight > score[y].weight
               : score[x].count != score[y].count ? score[x].count > score[y].count : x < y; });
    // 2. the walk
    std::vector<std::vector<uint8_t>> in_dir;               // [direction][segment]
    std::vector<uint32_t> mem;
    for (uint32_t h : cand) {
        if (r.directions.size() >= par.max_directions) break;
        bool dropped = false;
        for (const std::vector<uint8_t>& m : in_dir) if (m[h]) { dropped = true; break; }
        if (dropped) { ++s.n_dropped; continue; }
        if (s.n_tested == par.max_tests) { s.truncated = 1; break; }
        ++s.n_tested;
        dir_members(n, w, D, &D[3 * (size_t)h], par.max_sin2, mem);
        uint64_t weight = 0;
        for (uint32_t m : mem) weight += w.q[m];
        if (mem.size() != score[h].count || weight != score[h].weight) { if (bad) *bad = h; return 1; }
        bool rejected = false;
        for (const std::vector<uint8_t>& m : in_dir) {
            uint64_t common = 0;
            for (uint32_t i : mem) if (m[i]) common += w.q[i];
            if (2 * common > weight) { rejected = true; break; }
        }
        if (rejected) { ++s.n_rejected; continue; }
        const uint32_t number = (uint32_t)r.directions.size();
        r.directions.push_back(dir_describe(segs, line, w, D, h, weight, mem));
        in_dir.emplace_back(n, (uint8_t)0);
        for (uint32_t i : mem) { in_dir.back()[i] = 1; r.members.push_back(l3d_dir_member{number, i}); ++r.seg_directions[i]; }
    }
    // 5. the frame, 6. the summary
    dir_frame(r.directions, par, s);
    s.n_directions = r.directions.size(); s.n_memberships = r.members.size();
    for (uint32_t i = 0; i < n; ++i) {
        if (!r.seg_directions[i]) continue;
        ++s.n_segments_in_directions;
        if (r.seg_directions[i] > 1) ++s.n_segments_in_several;
        s.length_in_directions += w.len[i];
    }
    return 0;
}

}  // namespace l3d
