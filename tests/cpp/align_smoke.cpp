// align_smoke.cpp -- alignLines of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the Python
// test (the format facade_smoke.cpp reads):
//   align_smoke <scene> <out>
// The other model is this one's own get3Dlines under a known similarity (scale 1.25, a rotation about (1, 2, 2) / 3,
// a shift); the start handed to the facade is that similarity a little off.  Checked here: the facade returns the same
// bytes as the C-ABI call l3d_align_lines with the same parameters, and the model is left as it was.  Written to <out>:
// the parameters, the start, both models as flat segments and line indices, and the facade's similarity, summary, moved
// segments and both arrays of l3d_line_match; the test compares them with the model.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Vec4f { float v[4]; float operator[](int i) const { return v[i]; } };

typedef std::vector<L3DPP_HIP::Line3D::FinalLine3D> Lines;

static void flatten(const Lines& lines, std::vector<double>& segs, std::vector<uint32_t>& line) {
    for (size_t i = 0; i < lines.size(); ++i)
        for (const l3d_segment3d& s : lines[i].collinear3Dsegments_) {
            segs.insert(segs.end(), s.P1, s.P1 + 3);
            segs.insert(segs.end(), s.P2, s.P2 + 3);
            line.push_back((uint32_t)i);
        }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nv = 0;
    if (fread(&nv, 4, 1, f) != 1 || nv < 2) return 4;
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    for (uint32_t i = 0; i < nv; ++i) {
        uint32_t hdr[5];  // cam, M, width, height, n_nb
        Mat3 K, R; Vec3 t; float md;
        if (fread(hdr, 4, 5, f) != 5 || fread(K.m, 8, 9, f) != 9 || fread(R.m, 8, 9, f) != 9 ||
            fread(t.v, 8, 3, f) != 3 || fread(&md, 4, 1, f) != 1) return 5;
        std::vector<uint32_t> nb(hdr[4]);
        if (fread(nb.data(), 4, hdr[4], f) != hdr[4]) return 6;
        std::vector<Vec4f> segs(hdr[1]);
        if (fread(segs.data(), 16, hdr[1], f) != hdr[1]) return 7;
        L3DPP_HIP::ImageSize img{(int)hdr[2], (int)hdr[3]};
        l3d.addImage(hdr[0], img, K, R, t, md, std::list<unsigned int>(nb.begin(), nb.end()), segs);
    }
    fclose(f);
    // before reconstruct3Dlines there are no lines: the error is printed, the outputs stay as they were
    l3d_similarity sim{7.0, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    l3d_align_summary sum{};
    sum.iterations = 99;
    l3d.alignLines(Lines(), sim, sum, 0.01);
    if (sim.scale != 7.0 || sum.iterations != 99) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines own, other;
    l3d.get3Dlines(own);
    if (own.size() < 3) return 9;
    // the other frame: y = 1.25 R x + t, R the rotation of 0.5 rad about (1, 2, 2) / 3
    const l3d_similarity truth{1.25, {std::cos(0.25), std::sin(0.25) / 3.0, 2.0 * std::sin(0.25) / 3.0, 2.0 * std::sin(0.25) / 3.0}, {0.5, -1.0, 2.0}};
    std::vector<double> q, r;
    std::vector<uint32_t> ql, rl;
    flatten(own, q, ql);
    r.resize(q.size());
    if (l3d_transform_segments((uint32_t)ql.size(), q.data(), &truth, r.data()) != L3D_OK) return 10;
    other = own;
    size_t k = 0;
    for (Lines::value_type& L : other)
        for (l3d_segment3d& s : L.collinear3Dsegments_) {
            std::memcpy(s.P1, &r[6 * k], 24);
            std::memcpy(s.P2, &r[6 * k + 3], 24);
            ++k;
        }
    rl = ql;
    l3d_similarity start = truth;
    start.scale *= 1.01; start.q[1] += 0.004; start.t[2] += 0.01;
    const double max_distance = 0.005, start_distance = 0.16, max_angle = 10.0, min_overlap = 0.5;
    l3d.alignLines(other, sim, sum, max_distance, start_distance, &start, true, 91.0);     // an angle beyond 90 degrees: printed
    if (sim.scale != 7.0 || sum.iterations != 99) return 11;
    std::vector<double> moved;
    std::vector<l3d_line_match> mine, theirs;
    l3d.alignLines(other, sim, sum, max_distance, start_distance, &start, true, max_angle, min_overlap, &moved, &mine, &theirs);
    if (moved.size() != q.size() || mine.size() != ql.size() || theirs.size() != rl.size() || mine.empty()) return 12;
    // the C-ABI call itself
    const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
    const l3d_align_params par{max_distance, cosine * cosine, min_overlap, start_distance, 1e-9, 50u, 8u, 1u, 0u, {0u, 0u}};
    std::vector<double> m2(q.size());
    std::vector<l3d_line_match> a(ql.size()), b(rl.size());
    l3d_similarity sim2; l3d_align_summary sum2;
    if (l3d_align_lines(l3d.handle(), (uint32_t)rl.size(), r.data(), rl.data(), &par, &start, &sim2, &sum2, m2.data(), a.data(), b.data(), nullptr) != L3D_OK) return 13;
    if (std::memcmp(&sim, &sim2, sizeof sim) != 0 || std::memcmp(&sum, &sum2, sizeof sum) != 0) return 14;
    if (std::memcmp(moved.data(), m2.data(), 8 * moved.size()) != 0) return 15;
    if (std::memcmp(a.data(), mine.data(), sizeof(l3d_line_match) * a.size()) != 0) return 16;
    if (std::memcmp(b.data(), theirs.data(), sizeof(l3d_line_match) * b.size()) != 0) return 17;
    // the model itself has not moved
    Lines after;
    l3d.get3Dlines(after);
    std::vector<double> q2; std::vector<uint32_t> ql2;
    flatten(after, q2, ql2);
    if (q2.size() != q.size() || std::memcmp(q2.data(), q.data(), 8 * q.size()) != 0) return 18;
    f = fopen(argv[2], "wb");
    if (!f) return 19;
    const uint32_t n[2] = {(uint32_t)ql.size(), (uint32_t)rl.size()};
    fwrite(&par, sizeof par, 1, f);
    fwrite(&start, sizeof start, 1, f);
    fwrite(n, 4, 2, f);
    fwrite(q.data(), 8, q.size(), f); fwrite(ql.data(), 4, ql.size(), f);
    fwrite(r.data(), 8, r.size(), f); fwrite(rl.data(), 4, rl.size(), f);
    fwrite(&sim, sizeof sim, 1, f);
    fwrite(&sum, sizeof sum, 1, f);
    fwrite(moved.data(), 8, moved.size(), f);
    fwrite(mine.data(), sizeof(l3d_line_match), mine.size(), f);
    fwrite(theirs.data(), sizeof(l3d_line_match), theirs.size(), f);
    fclose(f);
    printf("RESULT segments=%u status=%u iterations=%u matched=%llu\n", n[0], sum.status, sum.iterations, (unsigned long long)sum.n_matched);
    return 0;
}
