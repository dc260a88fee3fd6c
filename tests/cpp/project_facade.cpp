// project_facade.cpp -- projectLines and drawLines of the C++ facade (include/line3dpp/line3D.h) on a scene file written
// by the Python test (the format facade_smoke.cpp reads), with ImageBuf8U images:
//   project_facade <scene> <grey image, raw> <rgb image, raw> <out>
// Written to <out>: the records of the first view by camID, the records of the second view by its K, R, t, the first
// view's overlay of the grey image (thickness 1, alpha 255) and the second view's overlay of the RGB image by K, R, t
// (thickness 3, alpha 128).  The test compares the bytes with the Python front end's.
#include <cstdio>
#include <cstdlib>
#include <list>
#include <string>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Vec4f { float v[4]; float operator[](int i) const { return v[i]; } };

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nv = 0;
    if (fread(&nv, 4, 1, f) != 1 || nv < 2) return 4;
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    std::vector<uint32_t> cams;
    std::vector<Mat3> Ks, Rs; std::vector<Vec3> ts;
    uint32_t width = 0, height = 0;
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
        cams.push_back(hdr[0]); Ks.push_back(K); Rs.push_back(R); ts.push_back(t);
        width = hdr[2]; height = hdr[3];
    }
    fclose(f);
    L3DPP_HIP::ImageBuf8U grey((int)height, (int)width, 0), rgb((int)height, (int)width, 16), out_grey, out_rgb;
    f = fopen(argv[2], "rb");
    if (!f || fread(grey.data, 1, (size_t)width * height, f) != (size_t)width * height) return 8;
    fclose(f);
    f = fopen(argv[3], "rb");
    if (!f || fread(rgb.data, 1, 3 * (size_t)width * height, f) != 3 * (size_t)width * height) return 9;
    fclose(f);
    // before reconstruct3Dlines there are no lines: the error is printed, the outputs stay empty
    std::vector<l3d_projected_segment> none(1);
    l3d.projectLines(cams[0], none);
    l3d.drawLines(cams[0], grey, out_grey);
    if (!none.empty() || !out_grey.empty()) return 10;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    std::vector<l3d_projected_segment> by_id, by_krt;
    l3d.projectLines(cams[0], by_id);
    l3d.projectLines(Ks[1], Rs[1], ts[1], width, height, by_krt);
    l3d.drawLines(cams[0], grey, out_grey);
    l3d.drawLines(Ks[1], Rs[1], ts[1], rgb, out_rgb, 3, 128);
    if (out_grey.empty() || out_rgb.empty() || out_grey.type() != 16 || out_grey.cols != (int)width || out_rgb.rows != (int)height) return 11;
    f = fopen(argv[4], "wb");
    if (!f) return 12;
    const uint32_t n[2] = {(uint32_t)by_id.size(), (uint32_t)by_krt.size()};
    fwrite(n, 4, 2, f);
    fwrite(by_id.data(), sizeof(l3d_projected_segment), by_id.size(), f);
    fwrite(by_krt.data(), sizeof(l3d_projected_segment), by_krt.size(), f);
    fwrite(out_grey.data, 1, 3 * (size_t)width * height, f);
    fwrite(out_rgb.data, 1, 3 * (size_t)width * height, f);
    fclose(f);
    printf("RESULT records=%u,%u\n", n[0], n[1]);
    return 0;
}
