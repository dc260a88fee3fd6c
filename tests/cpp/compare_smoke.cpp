// compare_smoke.cpp -- compareLines of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the Python
// test (the format facade_smoke.cpp reads):
//   compare_smoke <scene> <out>
// The other model is this one's own get3Dlines with its first line dropped, every second segment reversed and every
// third line moved by 1e-3.  Checked here: the facade returns the same bytes as the C-ABI call l3d_compare_lines with
// the same thresholds.  Written to <out>: max_distance, the squared cosine handed to the C-ABI, min_overlap, the
// numbers of segments of both sides, both models as flat segments (6 doubles) and line indices, and both arrays of
// l3d_line_match; the test compares them with the model.
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
    // before reconstruct3Dlines there are no lines: the error is printed, the outputs stay empty
    std::vector<l3d_line_match> mine(1), theirs(1);
    l3d.compareLines(Lines(), mine, theirs, 0.01);
    if (!mine.empty() || !theirs.empty()) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines own, other;
    l3d.get3Dlines(own);
    if (own.size() < 3) return 9;
    other.assign(own.begin() + 1, own.end());
    size_t k = 0;
    for (size_t i = 0; i < other.size(); ++i)
        for (l3d_segment3d& s : other[i].collinear3Dsegments_) {
            if (k++ % 2) for (int c = 0; c < 3; ++c) std::swap(s.P1[c], s.P2[c]);
            if (i % 3 == 0) { s.P1[1] += 1e-3; s.P2[1] += 1e-3; }
        }
    const double max_distance = 2e-3, max_angle = 10.0, min_overlap = 0.5;
    mine.assign(1, l3d_line_match{});
    l3d.compareLines(other, mine, theirs, max_distance, 91.0);     // an angle beyond 90 degrees: printed, empty
    if (!mine.empty() || !theirs.empty()) return 10;
    l3d.compareLines(other, mine, theirs, max_distance, max_angle, min_overlap);
    // the C-ABI call itself
    std::vector<double> q, r;
    std::vector<uint32_t> ql, rl;
    flatten(own, q, ql);
    flatten(other, r, rl);
    if (mine.size() != ql.size() || theirs.size() != rl.size() || mine.empty() || theirs.empty()) return 11;
    const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
    const l3d_compare_params par{max_distance, cosine * cosine, min_overlap, 0u, 0u};
    std::vector<l3d_line_match> a(ql.size()), b(rl.size());
    l3d_compare_summary sa, sb;
    if (l3d_compare_lines(l3d.handle(), (uint32_t)rl.size(), r.data(), rl.data(), &par, a.data(), b.data(), &sa, &sb) != L3D_OK) return 12;
    if (std::memcmp(a.data(), mine.data(), sizeof(l3d_line_match) * a.size()) != 0) return 13;
    if (std::memcmp(b.data(), theirs.data(), sizeof(l3d_line_match) * b.size()) != 0) return 14;
    uint64_t matched = 0;
    for (const l3d_line_match& m : mine) matched += m.segment >= 0;
    if (matched != sa.n_matched || sa.n_segments != ql.size() || sb.n_segments != rl.size()) return 15;
    f = fopen(argv[2], "wb");
    if (!f) return 16;
    const double thr[3] = {max_distance, par.min_cos2, min_overlap};
    const uint32_t n[2] = {(uint32_t)ql.size(), (uint32_t)rl.size()};
    fwrite(thr, 8, 3, f);
    fwrite(n, 4, 2, f);
    fwrite(q.data(), 8, q.size(), f); fwrite(ql.data(), 4, ql.size(), f);
    fwrite(r.data(), 8, r.size(), f); fwrite(rl.data(), 4, rl.size(), f);
    fwrite(mine.data(), sizeof(l3d_line_match), mine.size(), f);
    fwrite(theirs.data(), sizeof(l3d_line_match), theirs.size(), f);
    fclose(f);
    printf("RESULT segments=%u/%u matched=%llu\n", n[0], n[1], (unsigned long long)matched);
    return 0;
}
