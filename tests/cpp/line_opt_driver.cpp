// line_opt_driver.cpp -- the bundled reconstruction through the C++ facade (include/line3dpp/line3D.h), as a reference
// main_*.cpp asks for it: reconstruct3Dlines(3, false, -1, true, 50).  Scene file as tests/cpp/facade_smoke.cpp reads it
// (written by tests/test_gpu_line_opt.py); the same scene is reconstructed once without and once with bundling, and the
// cluster lines of equal residual sets are compared: bundled lines have moved.
#include <cmath>
#include <cstdio>
#include <list>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Vec4f { float v[4]; float operator[](int i) const { return v[i]; } };
using Key = std::set<std::pair<unsigned, unsigned>>;

static bool run(const char* path, bool use_ceres, std::map<Key, l3d_segment3d>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t nv = 0;
    if (fread(&nv, 4, 1, f) != 1) return false;
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    for (uint32_t i = 0; i < nv; ++i) {
        uint32_t hdr[5];  // cam, M, width, height, n_nb
        Mat3 K, R; Vec3 t; float md;
        if (fread(hdr, 4, 5, f) != 5 || fread(K.m, 8, 9, f) != 9 || fread(R.m, 8, 9, f) != 9 ||
            fread(t.v, 8, 3, f) != 3 || fread(&md, 4, 1, f) != 1) return false;
        std::vector<uint32_t> nb(hdr[4]);
        if (fread(nb.data(), 4, hdr[4], f) != hdr[4]) return false;
        std::vector<Vec4f> segs(hdr[1]);
        if (fread(segs.data(), 16, hdr[1], f) != hdr[1]) return false;
        L3DPP_HIP::ImageSize img{(int)hdr[2], (int)hdr[3]};
        l3d.addImage(hdr[0], img, K, R, t, md, std::list<unsigned int>(nb.begin(), nb.end()), segs);
    }
    fclose(f);
    l3d.matchImages();
    if (use_ceres) l3d.reconstruct3Dlines(3, false, -1, true, 50);
    else l3d.reconstruct3Dlines(3);
    std::vector<L3DPP_HIP::Line3D::FinalLine3D> lines;
    l3d.get3Dlines(lines);
    for (auto& L : lines) {
        Key k;
        for (auto& r : *L.underlyingCluster_.residuals()) k.insert({r.camID_, r.segID_});
        out[k] = L.underlyingCluster_.seg3D();
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::map<Key, l3d_segment3d> off, on;
    if (!run(argv[1], false, off) || !run(argv[1], true, on)) return 3;
    size_t common = 0, moved = 0;
    for (auto& kv : on) {
        auto it = off.find(kv.first);
        if (it == off.end()) continue;
        ++common;
        const double* a = reinterpret_cast<const double*>(&kv.second);   // P1[3], P2[3], dir[3]
        const double* b = reinterpret_cast<const double*>(&it->second);
        double dd = 0; for (int k = 0; k < 6; ++k) dd = std::fmax(dd, std::fabs(a[k] - b[k]));
        moved += dd > 1e-9;
    }
    printf("RESULT lines_off=%zu lines_on=%zu common=%zu moved=%zu\n", off.size(), on.size(), common, moved);
    return 0;
}
