// wireframe_smoke.cpp -- wireframe of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the Python test
// (the format facade_smoke.cpp reads):
//   wireframe_smoke <scene> <out>
// Checked here: wireframe hands out the very bytes the stateless C-ABI call l3d_wireframe_segments returns for the model
// of get3Dlines with the same thresholds, and leaves that model as it was.  Written to <out>: max_distance,
// max_extension, the squared sine handed to the C-ABI, the numbers of segments, junctions, vertices and edges, the model
// as flat segments (6 doubles) and line indices, the three arrays and the l3d_wireframe_summary; the test compares them
// with the numpy model.
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
typedef L3DPP_HIP::Line3D::Wireframe Wireframe;

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
    const double max_distance = 1.5, min_angle = 10.0;
    Wireframe w = l3d.wireframe(max_distance);                      // before reconstruct3Dlines: printed, an empty result
    if (w.ok || !w.junctions.empty() || !w.vertices.empty() || !w.edges.empty()) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines before, after;
    l3d.get3Dlines(before);
    if (before.size() < 3) return 9;
    w = l3d.wireframe(max_distance, -1.0, 91.0);                    // an angle beyond 90 degrees: printed, an empty result
    if (w.ok || !w.vertices.empty()) return 10;
    // the stateless C-ABI call on the model
    std::vector<double> q;
    std::vector<uint32_t> ql;
    flatten(before, q, ql);
    const uint32_t n = (uint32_t)ql.size();
    const double sine = std::sin(min_angle * (3.14159265358979323846 / 180.0));
    const l3d_wireframe_params par{max_distance, max_distance, sine * sine, 0u, 0u};
    l3d_wireframe* h = nullptr;
    if (l3d_wireframe_segments(0, n, q.data(), ql.data(), &par, &h) != L3D_OK) return 11;
    Wireframe want;
    uint64_t nj = 0, nvx = 0, ne = 0;
    if (l3d_wireframe_counts(h, &nj, &nvx, &ne) != L3D_OK) return 12;
    want.junctions.resize(nj); want.vertices.resize(nvx); want.edges.resize(ne);
    if (l3d_wireframe_get(h, want.junctions.data(), want.vertices.data(), want.edges.data(), &want.summary) != L3D_OK) return 13;
    l3d_wireframe_close(h);
    w = l3d.wireframe(max_distance, -1.0, min_angle);
    if (!w.ok) return 14;
    if (!same(w.junctions, want.junctions) || !same(w.vertices, want.vertices) || !same(w.edges, want.edges)) return 15;
    if (std::memcmp(&w.summary, &want.summary, sizeof(want.summary)) != 0) return 16;
    // the model is as it was
    l3d.get3Dlines(after);
    std::vector<double> r;
    std::vector<uint32_t> rl;
    flatten(after, r, rl);
    if (after.size() != before.size() || !same(r, q) || !same(rl, ql)) return 17;
    f = fopen(argv[2], "wb");
    if (!f) return 18;
    const double thr[3] = {par.max_distance, par.max_extension, par.min_sin2};
    const uint64_t cnt[4] = {n, nj, nvx, ne};
    fwrite(thr, 8, 3, f);
    fwrite(cnt, 8, 4, f);
    fwrite(q.data(), 8, q.size(), f); fwrite(ql.data(), 4, ql.size(), f);
    fwrite(w.junctions.data(), sizeof(l3d_wf_junction), w.junctions.size(), f);
    fwrite(w.vertices.data(), sizeof(l3d_wf_vertex), w.vertices.size(), f);
    fwrite(w.edges.data(), sizeof(l3d_wf_edge), w.edges.size(), f);
    fwrite(&w.summary, sizeof(w.summary), 1, f);
    fclose(f);
    printf("RESULT segments=%u junctions=%llu vertices=%llu edges=%llu components=%llu\n", n, (unsigned long long)nj,
           (unsigned long long)nvx, (unsigned long long)ne, (unsigned long long)w.summary.n_components);
    return 0;
}
