// associate_smoke.cpp -- associateSegments of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the
// Python test (the format facade_smoke.cpp reads):
//   associate_smoke <scene> <out>
// Checked here: the all-views form returns the same records as the C-ABI call with the same thresholds, and the form
// for one view the same as its entry in the all-views form.  Written to <out>: the number of views, the squared cosine
// handed to the C-ABI, and per view (camID, number of segments, the l3d_association of every segment); the test compares
// them with the model.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Vec4f { float v[4]; float operator[](int i) const { return v[i]; } };

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nv = 0;
    if (fread(&nv, 4, 1, f) != 1 || nv < 2) return 4;
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    std::vector<uint32_t> cams;
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
        cams.push_back(hdr[0]);
    }
    fclose(f);
    // before reconstruct3Dlines there are no lines: the error is printed, the output stays empty
    std::map<unsigned int, std::vector<l3d_association>> all;
    all[0].resize(1);
    l3d.associateSegments(all);
    if (!all.empty()) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    std::vector<l3d_association> one(1);
    l3d.associateSegments(cams[1], one, 2.5, 91.0);            // an angle beyond 90 degrees: printed, empty
    if (!one.empty()) return 9;
    l3d.associateSegments(all);
    if (all.size() != nv) return 10;
    l3d.associateSegments(cams[1], one);
    if (one.size() != all[cams[1]].size() || one.empty() ||
        std::memcmp(one.data(), all[cams[1]].data(), sizeof(l3d_association) * one.size()) != 0) return 11;
    // the C-ABI call itself, views in ascending camID as the map holds them
    std::vector<uint32_t> ids;
    for (const auto& kv : all) ids.push_back(kv.first);
    const double cosine = std::cos(10.0 * (3.14159265358979323846 / 180.0));
    const l3d_associate_params par{2.5, cosine * cosine, 0.5};
    std::vector<uint64_t> off(nv + 1);
    if (l3d_associate_view_segments(l3d.handle(), nv, ids.data(), &par, 1e-6, off.data(), nullptr, nullptr, nullptr) != L3D_OK) return 12;
    std::vector<l3d_association> flat(off[nv] ? off[nv] : 1);
    uint32_t n_lines = 0;
    if (l3d_num_3d_lines(l3d.handle(), &n_lines, nullptr, nullptr) != L3D_OK) return 13;
    std::vector<uint32_t> sup_s(n_lines + 1), sup_v(n_lines + 1);
    if (l3d_associate_view_segments(l3d.handle(), nv, ids.data(), &par, 1e-6, off.data(), flat.data(), sup_s.data(), sup_v.data()) != L3D_OK) return 14;
    uint64_t assigned = 0, supported = 0;
    for (uint32_t k = 0; k < nv; ++k) {
        const std::vector<l3d_association>& a = all[ids[k]];
        if (a.size() != off[k + 1] - off[k]) return 15;
        if (!a.empty() && std::memcmp(a.data(), flat.data() + off[k], sizeof(l3d_association) * a.size()) != 0) return 16;
        for (const l3d_association& r : a) assigned += r.record >= 0;
    }
    for (uint32_t i = 0; i < n_lines; ++i) supported += sup_s[i];
    if (assigned != supported) return 17;
    f = fopen(argv[2], "wb");
    if (!f) return 18;
    fwrite(&nv, 4, 1, f);
    fwrite(&par.min_cos2, 8, 1, f);
    for (uint32_t k = 0; k < nv; ++k) {
        const uint32_t hdr[2] = {ids[k], (uint32_t)all[ids[k]].size()};
        fwrite(hdr, 4, 2, f);
        fwrite(all[ids[k]].data(), sizeof(l3d_association), hdr[1], f);
    }
    fclose(f);
    printf("RESULT views=%u assigned=%llu\n", nv, (unsigned long long)assigned);
    return 0;
}
