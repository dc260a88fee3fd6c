// lsd_facade.cpp -- addImage with an image and no segments through the C++ facade (include/line3dpp/line3D.h), as the
// reference's main_*.cpp call it: the segments are detected on the GPU.  The same views are added once as Image8U with
// no segments and once as ImageSize with the segments detect_line_segments returned (scene file written by
// tests/test_gpu_lsd.py); matchImages + reconstruct3Dlines must give byte-identical 3D lines.  The image views are
// added from one thread each, as the reference's front ends call addImage from an OpenMP loop: every view must then
// report its own segment count through matches(camID).
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <thread>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Vec4f { float v[4]; float operator[](int i) const { return v[i]; } };

struct View {
    uint32_t cam, cols, rows;
    Mat3 K, R; Vec3 t; float md;
    std::vector<uint32_t> nb;
    std::vector<unsigned char> pix;
    std::vector<Vec4f> segs;
};

static bool read(const char* path, std::vector<View>& vs) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t nv = 0;
    if (fread(&nv, 4, 1, f) != 1) return false;
    vs.resize(nv);
    for (View& v : vs) {
        uint32_t hdr[5];  // cam, cols, rows, n_nb, M
        if (fread(hdr, 4, 5, f) != 5 || fread(v.K.m, 8, 9, f) != 9 || fread(v.R.m, 8, 9, f) != 9 ||
            fread(v.t.v, 8, 3, f) != 3 || fread(&v.md, 4, 1, f) != 1) return false;
        v.cam = hdr[0]; v.cols = hdr[1]; v.rows = hdr[2];
        v.nb.resize(hdr[3]); v.pix.resize((size_t)v.cols * v.rows); v.segs.resize(hdr[4]);
        if (fread(v.nb.data(), 4, hdr[3], f) != hdr[3] || fread(v.pix.data(), 1, v.pix.size(), f) != v.pix.size() ||
            fread(v.segs.data(), 16, hdr[4], f) != hdr[4]) return false;
    }
    fclose(f);
    return true;
}

static bool run(const std::vector<View>& vs, bool detect, std::vector<L3DPP_HIP::Line3D::FinalLine3D>& out) {
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    std::vector<std::thread> threads;
    for (const View& v : vs) {
        if (detect) {
            threads.emplace_back([&l3d, &v] {
                const std::list<unsigned int> nb(v.nb.begin(), v.nb.end());
                L3DPP_HIP::Image8U img{v.pix.data(), (int)v.cols, (int)v.rows, 1, (size_t)v.cols};
                l3d.addImage(v.cam, img, v.K, v.R, v.t, v.md, nb, std::vector<Vec4f>());
            });
        } else {
            const std::list<unsigned int> nb(v.nb.begin(), v.nb.end());
            L3DPP_HIP::ImageSize img{(int)v.cols, (int)v.rows};
            l3d.addImage(v.cam, img, v.K, v.R, v.t, v.md, nb, v.segs);
        }
    }
    for (std::thread& t : threads) t.join();
    l3d.matchImages();
    bool counts = l3d.numImages() == vs.size();
    for (const View& v : vs) {
        const size_t m = l3d.matches(v.cam).size();
        if (m != v.segs.size()) {
            std::printf("view %u: %zu segments reported, %zu detected\n", v.cam, m, v.segs.size());
            counts = false;
        }
    }
    l3d.reconstruct3Dlines();
    l3d.get3Dlines(out);
    return counts;
}

int main(int argc, char** argv) {
    std::vector<View> vs;
    if (argc < 2 || !read(argv[1], vs)) { std::printf("cannot read the scene\n"); return 2; }
    std::vector<L3DPP_HIP::Line3D::FinalLine3D> a, b;
    const bool counts = run(vs, true, a) && run(vs, false, b);
    bool same = counts && a.size() == b.size();
    for (size_t i = 0; same && i < a.size(); ++i) {
        const l3d_segment3d sa = a[i].underlyingCluster_.seg3D(), sb = b[i].underlyingCluster_.seg3D();
        same = std::memcmp(&sa, &sb, sizeof sa) == 0 && a[i].underlyingCluster_.size() == b[i].underlyingCluster_.size() &&
               a[i].collinear3Dsegments_.size() == b[i].collinear3Dsegments_.size();
        auto ra = a[i].underlyingCluster_.residuals()->begin(), rb = b[i].underlyingCluster_.residuals()->begin();
        for (; same && ra != a[i].underlyingCluster_.residuals()->end(); ++ra, ++rb)
            same = ra->camID_ == rb->camID_ && ra->segID_ == rb->segID_;
    }
    std::printf("RESULT lines=%zu counts=%d identical=%d\n", a.size(), counts ? 1 : 0, same ? 1 : 0);
    return same ? 0 : 1;
}
