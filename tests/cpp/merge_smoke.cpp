// merge_smoke.cpp -- mergeLines of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the Python test
// (the format facade_smoke.cpp reads):
//   merge_smoke <scene> <out>
// Checked here: after mergeLines, get3Dlines hands out the very bytes the stateless C-ABI call l3d_merge_segments
// returns for the model as it was before, with the same thresholds, and the same summary.  Written to <out>:
// max_distance, the squared cosine handed to the C-ABI, min_overlap, the numbers of segments before and after, the model
// before and the model after as flat segments (6 doubles) and line indices, and the l3d_merge_summary; the test compares
// them with the numpy model.
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
    const double max_distance = 1.5, max_angle = 10.0, min_overlap = 0.5;
    l3d_merge_summary none;
    std::memset(&none, 0x5A, sizeof(none));
    l3d_merge_summary got = none;
    l3d.mergeLines(max_distance, max_angle, min_overlap, &got);    // before reconstruct3Dlines: printed, nothing written
    if (std::memcmp(&got, &none, sizeof(none)) != 0) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines before, after;
    l3d.get3Dlines(before);
    if (before.size() < 3) return 9;
    l3d.mergeLines(max_distance, 91.0, min_overlap, &got);         // an angle beyond 90 degrees: printed, nothing done
    l3d.get3Dlines(after);
    if (std::memcmp(&got, &none, sizeof(none)) != 0 || after.size() != before.size()) return 10;
    // the stateless C-ABI call on the model as it is now
    std::vector<double> q;
    std::vector<uint32_t> ql;
    flatten(before, q, ql);
    const uint32_t n = (uint32_t)ql.size();
    const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
    const l3d_merge_params par{max_distance, cosine * cosine, min_overlap, 0u, 0u};
    std::vector<uint32_t> line_map(n), seg_line(n);
    std::vector<double> segs(6 * (size_t)n);
    std::vector<l3d_merge_line_info> info(n);
    uint32_t n_segs = 0, n_lines = 0;
    l3d_merge_summary want;
    if (l3d_merge_segments(0, n, q.data(), ql.data(), &par, line_map.data(), n, segs.data(), seg_line.data(), &n_segs, n, info.data(),
                           &n_lines, &want) != L3D_OK) return 11;
    l3d.mergeLines(max_distance, max_angle, min_overlap, &got);
    if (std::memcmp(&got, &want, sizeof(want)) != 0) return 12;
    l3d.get3Dlines(after);
    std::vector<double> r;
    std::vector<uint32_t> rl;
    flatten(after, r, rl);
    if (after.size() != n_lines || rl.size() != n_segs) return 13;
    if (std::memcmp(r.data(), segs.data(), 48 * (size_t)n_segs) != 0) return 14;
    if (std::memcmp(rl.data(), seg_line.data(), 4 * (size_t)n_segs) != 0) return 15;
    f = fopen(argv[2], "wb");
    if (!f) return 16;
    const double thr[3] = {max_distance, par.min_cos2, min_overlap};
    const uint32_t cnt[2] = {n, n_segs};
    fwrite(thr, 8, 3, f);
    fwrite(cnt, 4, 2, f);
    fwrite(q.data(), 8, q.size(), f); fwrite(ql.data(), 4, ql.size(), f);
    fwrite(r.data(), 8, r.size(), f); fwrite(rl.data(), 4, rl.size(), f);
    fwrite(&got, sizeof(got), 1, f);
    fclose(f);
    printf("RESULT lines=%u->%u segments=%u->%u merged=%llu\n", (unsigned)before.size(), n_lines, n, n_segs,
           (unsigned long long)got.n_merged_components);
    return 0;
}
