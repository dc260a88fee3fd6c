// bundle_smoke.cpp -- bundleModel of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the Python
// test (the format facade_smoke.cpp reads):
//   bundle_smoke <scene> <out>
// Checked here: a call before reconstruct3Dlines and one with an angle beyond 90 degrees print an error and leave the
// model, the summary and the camera map as they were; a call with one view's camera given by hand replaces the model,
// fills the summary and writes every view's new camera into the map.
// Written to <out>: the summary, the model before and the model after as flat segments and line indices, and per view
// its camID, the camera the context holds and the camera the call returned; the test compares them with the stateless call.
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

typedef std::vector<L3DPP_HIP::Line3D::FinalLine3D> Lines;

static void flatten(const Lines& lines, std::vector<double>& segs, std::vector<uint32_t>& line) {
    for (size_t i = 0; i < lines.size(); ++i)
        for (const l3d_segment3d& s : lines[i].collinear3Dsegments_) {
            segs.insert(segs.end(), s.P1, s.P1 + 3);
            segs.insert(segs.end(), s.P2, s.P2 + 3);
            line.push_back((uint32_t)i);
        }
}

static void put(FILE* f, const std::vector<double>& segs, const std::vector<uint32_t>& line) {
    const uint32_t n = (uint32_t)line.size();
    fwrite(&n, 4, 1, f);
    fwrite(segs.data(), 8, segs.size(), f);
    fwrite(line.data(), 4, line.size(), f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nv = 0;
    if (fread(&nv, 4, 1, f) != 1 || nv < 3) return 4;
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    std::vector<uint32_t> ids;
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
        ids.push_back(hdr[0]);
    }
    fclose(f);
    l3d_bundle_summary sum;
    std::memset(&sum, 0x5A, sizeof sum);
    const l3d_bundle_summary fill = sum;
    std::map<unsigned int, l3d_camera> cams;
    l3d.bundleModel(&cams, 2.5, 10.0, 0.5, 3, 10, false, 0.0, nullptr, nullptr, &sum);      // no lines yet: printed
    if (std::memcmp(&sum, &fill, sizeof sum) != 0 || !cams.empty()) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines own;
    l3d.get3Dlines(own);
    if (own.size() < 3) return 9;
    std::vector<double> before, after;
    std::vector<uint32_t> line, line2;
    flatten(own, before, line);
    l3d.bundleModel(&cams, 2.5, 91.0, 0.5, 3, 10, false, 0.0, nullptr, nullptr, &sum);      // an angle beyond 90 degrees: printed
    if (std::memcmp(&sum, &fill, sizeof sum) != 0 || !cams.empty()) return 10;
    Lines same;
    l3d.get3Dlines(same);
    flatten(same, after, line2);
    if (after.size() != before.size() || std::memcmp(after.data(), before.data(), 8 * before.size()) != 0) return 11;
    // one view's camera by hand (its own), the others looked up by the facade
    if (l3d_view_camera(l3d.handle(), ids[1], &cams[ids[1]]) != L3D_OK) return 12;
    l3d.bundleModel(&cams, 2.5, 10.0, 0.5, 3, 10, false, 0.0, nullptr, nullptr, &sum);
    if (sum.n_segments_before != line.size() || sum.n_lines != own.size() || cams.size() != ids.size()) return 13;
    Lines bundled;
    l3d.get3Dlines(bundled);
    after.clear(); line2.clear();
    flatten(bundled, after, line2);
    if (bundled.size() != own.size() || sum.n_segments_after != line2.size()) return 14;
    f = fopen(argv[2], "wb");
    if (!f) return 20;
    fwrite(&sum, sizeof sum, 1, f);
    put(f, before, line);
    put(f, after, line2);
    for (uint32_t id : ids) {                     // the cameras the context holds and the ones the call returned
        l3d_camera cam;
        if (l3d_view_camera(l3d.handle(), id, &cam) != L3D_OK) return 21;
        fwrite(&id, 4, 1, f);
        fwrite(&cam, sizeof cam, 1, f);
        fwrite(&cams[id], sizeof cam, 1, f);
    }
    fclose(f);
    printf("RESULT views=%u lines=%u bundled=%u iterations=%u\n", nv, (unsigned)own.size(), (unsigned)sum.n_status[L3D_BUNDLE_BUNDLED],
           sum.iterations);
    return 0;
}
