// undistort_models_facade.cpp -- Line3D::undistortImage(inImg, outImg, model, params, K[, K_new]) through the C++ facade
// (include/line3dpp/line3D.h) from four threads at once.  Input (written by tests/test_gpu_undistort_models.py): n, then
// per image cols, rows, channels, model (L3D_CAM_*), has_K_new, K[9], K_new[9], params[8] (doubles) and the pixels.
// Output: every undistorted image's bytes.  An unknown model must print an error and leave the output empty; so must a
// parameter list of more than 8 values.
#include <cstdio>
#include <thread>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat3 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };

struct Input {
    uint32_t cols, rows, ch, model, has_new;
    Mat3 K, K_new;
    std::vector<double> params;
    std::vector<unsigned char> pix;
};

static bool read(const char* path, std::vector<Input>& ins) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return false;
    ins.resize(n);
    for (Input& in : ins) {
        uint32_t hdr[5];
        double d[26];
        if (fread(hdr, 4, 5, f) != 5 || fread(d, 8, 26, f) != 26) return false;
        in.cols = hdr[0]; in.rows = hdr[1]; in.ch = hdr[2]; in.model = hdr[3]; in.has_new = hdr[4];
        for (int k = 0; k < 9; ++k) { in.K.m[k] = d[k]; in.K_new.m[k] = d[9 + k]; }
        in.params.assign(d + 18, d + 26);
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
            if (in.has_new) L3DPP_HIP::Line3D::undistortImage(img, outs[k], in.model, in.params, in.K, in.K_new);
            else L3DPP_HIP::Line3D::undistortImage(img, outs[k], in.model, in.params, in.K);
        });
    for (std::thread& t : threads) t.join();
    size_t ok = 0;
    for (size_t k = 0; k < n; ++k)
        ok += !outs[k].empty() && outs[k].cols == (int)ins[k].cols && outs[k].rows == (int)ins[k].rows &&
              outs[k].channels() == (int)ins[k].ch;
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (const L3DPP_HIP::ImageBuf8U& o : outs) fwrite(o.data, 1, o.step * o.rows, f);
    fclose(f);

    // the constants of l3dpp_hip.h and a braced list go straight in; an unknown model and a list that is too long print
    // the error line and leave the output empty
    const Input& in = ins[0];
    const L3DPP_HIP::Image8U img{in.pix.data(), (int)in.cols, (int)in.rows, (int)in.ch, (size_t)in.cols * in.ch};
    L3DPP_HIP::ImageBuf8U braced, unknown(48, 64, 0), too_long(48, 64, 0);
    L3DPP_HIP::Line3D::undistortImage(img, braced, L3D_CAM_FOV, {0.0}, in.K);
    const bool identity = !braced.empty() && std::memcmp(braced.data, in.pix.data(), in.pix.size()) == 0;
    L3DPP_HIP::Line3D::undistortImage(img, unknown, 77, in.params, in.K);
    L3DPP_HIP::Line3D::undistortImage(img, too_long, L3D_CAM_FULL_OPENCV, std::vector<double>(9, 0.0), in.K);
    std::printf("RESULT undistorted=%zu fov_zero_is_identity=%d errors_left_empty=%d\n", ok, identity ? 1 : 0,
                unknown.empty() && too_long.empty() ? 1 : 0);
    return ok == n && identity && unknown.empty() && too_long.empty() ? 0 : 1;
}
