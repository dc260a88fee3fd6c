// directions_smoke.cpp -- detectDirections of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the
// Python test (the format facade_smoke.cpp reads):
//   directions_smoke <scene> <out>
// Checked here: detectDirections hands out the very bytes the stateless C-ABI call l3d_direction_segments returns for the
// model of get3Dlines with the same parameters, and leaves that model as it was.  Written to <out>: the 64 bytes of
// l3d_directions_params handed to the C-ABI, the numbers of segments, directions, memberships and hypotheses, the model as
// flat segments (6 doubles) and line indices, the four arrays and the l3d_directions_summary; the test compares them with
// the numpy model.
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
typedef L3DPP_HIP::Line3D::Directions Directions;

static void flatten(const Lines& lines, std::vector<double>& segs, std::vector<uint32_t>& line) {
    for (size_t i = 0; i < lines.size(); ++i)
        for (const l3d_segment3d& s : lines[i].collinear3Dsegments_) {
            segs.insert(segs.end(), s.P1, s.P1 + 3);
            segs.insert(segs.end(), s.P2, s.P2 + 3);
            line.push_back((uint32_t)i);
        }
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
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
    const double max_angle = 15.0, frame_angle = 20.0;
    Directions d = l3d.detectDirections(max_angle);                 // before reconstruct3Dlines: printed, an empty result
    if (d.ok || !d.directions.empty() || !d.members.empty() || !d.scores.empty()) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines before, after;
    l3d.get3Dlines(before);
    if (before.size() < 3) return 9;
    d = l3d.detectDirections(91.0);                                 // an angle beyond 90 degrees: printed, an empty result
    if (d.ok || !d.directions.empty()) return 10;
    // the stateless C-ABI call on the model
    std::vector<double> q;
    std::vector<uint32_t> ql;
    flatten(before, q, ql);
    const uint32_t n = (uint32_t)ql.size();
    const double sine = std::sin(max_angle * (3.14159265358979323846 / 180.0));
    const double frame_sine = std::sin(frame_angle * (3.14159265358979323846 / 180.0));
    const l3d_directions_params par{sine * sine, 1.0, frame_sine * frame_sine, 3u, 8u, 100u, 0u, 16u, {0u, 0u, 0u, 0u, 0u}};
    l3d_directions* h = nullptr;
    if (l3d_direction_segments(0, n, q.data(), ql.data(), &par, &h) != L3D_OK) return 11;
    Directions want;
    uint64_t nd = 0, nm = 0, nh = 0;
    if (l3d_directions_counts(h, &nd, &nm, &nh) != L3D_OK) return 12;
    want.directions.resize(nd); want.members.resize(nm); want.seg_directions.resize(n); want.scores.resize(nh);
    if (l3d_directions_get(h, want.directions.data(), want.members.data(), want.seg_directions.data(), want.scores.data(), &want.summary) != L3D_OK)
        return 13;
    l3d_directions_close(h);
    d = l3d.detectDirections(max_angle, 1.0, 3, 8, 100, frame_angle);
    if (!d.ok) return 14;
    if (!same(d.directions, want.directions) || !same(d.members, want.members) || !same(d.seg_directions, want.seg_directions) ||
        !same(d.scores, want.scores))
        return 15;
    if (std::memcmp(&d.summary, &want.summary, sizeof(want.summary)) != 0) return 16;
    // the model is as it was
    l3d.get3Dlines(after);
    std::vector<double> r;
    std::vector<uint32_t> rl;
    flatten(after, r, rl);
    if (after.size() != before.size() || !same(r, q) || !same(rl, ql)) return 17;
    f = fopen(argv[2], "wb");
    if (!f) return 18;
    const uint64_t cnt[4] = {n, nd, nm, nh};
    fwrite(&par, sizeof(par), 1, f);
    fwrite(cnt, 8, 4, f);
    fwrite(q.data(), 8, q.size(), f); fwrite(ql.data(), 4, ql.size(), f);
    fwrite(d.directions.data(), sizeof(l3d_dir_direction), d.directions.size(), f);
    fwrite(d.members.data(), sizeof(l3d_dir_member), d.members.size(), f);
    fwrite(d.seg_directions.data(), 4, d.seg_directions.size(), f);
    fwrite(d.scores.data(), sizeof(l3d_dir_score), d.scores.size(), f);
    fwrite(&d.summary, sizeof(d.summary), 1, f);
    fclose(f);
    printf("RESULT segments=%u directions=%llu memberships=%llu\n", n, (unsigned long long)nd, (unsigned long long)nm);
    return 0;
}
