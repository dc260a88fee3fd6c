// undistort_facade.cpp -- Line3D::undistortImage through the C++ facade (include/line3dpp/line3D.h) as the reference's
// front ends call it: from several threads at once (their OpenMP loops), into an owning ImageBuf8U, which then goes to
// addImage with no segments.  Input (written by tests/test_gpu_undistort.py): n, then per image cols, rows, channels,
// K[9], radial[3], tangential[2] (doubles) and the pixels.  Output: every undistorted image's bytes, then per view the
// first 3001 segments addImage detected (getSegmentCoords2D; zeros past the last one).  An image of an unsupported
// type must print an error and leave the output empty.
#include <cstdio>
#include <list>
#include <thread>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vec { double v[3]; double operator()(int i) const { return v[i]; } };
struct Vec4f { float v[4]; float operator[](int i) const { return v[i]; } };

struct Input {
    uint32_t cols, rows, ch;
    Mat3 K; Vec radial, tangential;
    std::vector<unsigned char> pix;
};

static bool read(const char* path, std::vector<Input>& ins) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return false;
    ins.resize(n);
    for (Input& in : ins) {
        uint32_t hdr[3];
        double d[14];
        if (fread(hdr, 4, 3, f) != 3 || fread(d, 8, 14, f) != 14) return false;
        in.cols = hdr[0]; in.rows = hdr[1]; in.ch = hdr[2];
        for (int k = 0; k < 9; ++k) in.K.m[k] = d[k];
        for (int k = 0; k < 3; ++k) in.radial.v[k] = d[9 + k];
        for (int k = 0; k < 2; ++k) in.tangential.v[k] = d[12 + k];
        in.pix.resize((size_t)in.cols * in.rows * in.ch);
        if (fread(in.pix.data(), 1, in.pix.size(), f) != in.pix.size()) return false;
    }
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    std::vector<Input> ins;
    if (argc < 3 || !read(argv[1], ins)) { std::printf("cannot read the input\n"); return 2; }
    const size_t n = ins.size();
    std::vector<L3DPP_HIP::ImageBuf8U> outs(n);
    std::vector<std::thread> threads;
    for (size_t k = 0; k < n; ++k)
        threads.emplace_back([&ins, &outs, k] {
            const Input& in = ins[k];
            const L3DPP_HIP::Image8U img{in.pix.data(), (int)in.cols, (int)in.rows, (int)in.ch, (size_t)in.cols * in.ch};
            L3DPP_HIP::Line3D::undistortImage(img, outs[k], in.radial, in.tangential, in.K);
        });
    for (std::thread& t : threads) t.join();
    size_t ok = 0;
    for (size_t k = 0; k < n; ++k)
        ok += !outs[k].empty() && outs[k].cols == (int)ins[k].cols && outs[k].rows == (int)ins[k].rows &&
              outs[k].channels() == (int)ins[k].ch;

    FILE* f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (const L3DPP_HIP::ImageBuf8U& o : outs) fwrite(o.data, 1, o.step * o.rows, f);
    // the undistorted images as views with no segments: addImage detects on them
    L3DPP_HIP::Line3D l3d("/tmp", false, -1, 3000, false, true);
    const Mat3 R{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    for (size_t k = 0; k < n; ++k) {
        std::list<unsigned int> nb;
        for (size_t j = 0; j < n; ++j) if (j != k) nb.push_back((unsigned)j);
        const Vec t{{0.5 * k, 0.0, 0.0}};
        l3d.addImage((unsigned)k, outs[k], ins[k].K, R, t, 5.0f, nb, std::vector<Vec4f>());
    }
    for (size_t k = 0; k < n; ++k)
        for (unsigned s = 0; s < 3001; ++s) fwrite(l3d.getSegmentCoords2D((unsigned)k, s).v, 4, 4, f);
    fclose(f);

    // an unsupported image type: the reference's error line, and the output is left empty
    std::vector<unsigned char> two(64 * 48 * 2, 7);
    const L3DPP_HIP::Image8U bad{two.data(), 64, 48, 2, 128};
    L3DPP_HIP::ImageBuf8U left(48, 64, 0);
    L3DPP_HIP::Line3D::undistortImage(bad, left, ins[0].radial, ins[0].tangential, ins[0].K);
    std::printf("RESULT undistorted=%zu error_left_empty=%d\n", ok, left.empty() ? 1 : 0);
    return ok == n && left.empty() ? 0 : 1;
}
