// pose_smoke.cpp -- refineCameras of the C++ facade (include/line3dpp/line3D.h) on a scene file written by the Python
// test (the format facade_smoke.cpp reads):
//   pose_smoke <scene> <out>
// Checked here: a call before reconstruct3Dlines and one with an angle beyond 90 degrees print an error and leave the
// outputs as they were; the facade returns the same bytes as the C-ABI call l3d_refine_view_cameras with the same
// parameters, for all views and for a subset in reversed order; the model and the views' cameras are left as they were.
// Written to <out>: the parameters, the number of views, the model as flat segments and line indices, and per view its
// camID, the camera the context holds, the number of its segments, the refined camera, the summary and the associations;
// the test compares them with the model.
#include <algorithm>
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
    // before reconstruct3Dlines there are no lines: the error is printed, the outputs stay as they were
    std::map<unsigned int, l3d_camera> cams;
    std::map<unsigned int, l3d_pose_summary> sums;
    l3d.refineCameras(cams, sums);
    if (!cams.empty() || !sums.empty()) return 8;
    l3d.matchImages();
    l3d.reconstruct3Dlines(3);
    Lines own;
    l3d.get3Dlines(own);
    if (own.size() < 3) return 9;
    std::vector<double> before;
    std::vector<uint32_t> line;
    flatten(own, before, line);
    const double max_distance = 2.5, start_distance = 10.0, max_angle = 10.0, min_overlap = 0.5;
    l3d.refineCameras(cams, sums, max_distance, start_distance, 91.0);         // an angle beyond 90 degrees: printed
    if (!cams.empty() || !sums.empty()) return 10;
    std::map<unsigned int, std::vector<l3d_association>> assoc;
    l3d.refineCameras(cams, sums, max_distance, start_distance, max_angle, min_overlap, nullptr, &assoc);
    if (cams.size() != nv || sums.size() != nv || assoc.size() != nv) return 11;
    // the C-ABI call itself
    const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
    const l3d_pose_params par{max_distance, cosine * cosine, min_overlap, start_distance, 1e-4, 1e-9, 1e-6, 50u, 8u, {0u, 0u}};
    std::vector<uint32_t> sorted(ids);
    std::sort(sorted.begin(), sorted.end());
    std::vector<uint64_t> off(nv + 1);
    size_t room = 0;
    for (uint32_t id : sorted) room += assoc[id].size();
    std::vector<l3d_camera> c2(nv); std::vector<l3d_pose_summary> s2(nv); std::vector<l3d_association> a2(room + 1);
    if (l3d_refine_view_cameras(l3d.handle(), nv, sorted.data(), &par, c2.data(), s2.data(), off.data(), a2.data(), nullptr) != L3D_OK) return 12;
    if (off[nv] != room) return 13;
    for (uint32_t k = 0; k < nv; ++k) {
        const uint32_t id = sorted[k];
        if (std::memcmp(&cams[id], &c2[k], sizeof(l3d_camera)) != 0 || std::memcmp(&sums[id], &s2[k], sizeof(l3d_pose_summary)) != 0) return 14;
        if (assoc[id].size() != off[k + 1] - off[k]) return 15;
        if (!assoc[id].empty() && std::memcmp(assoc[id].data(), a2.data() + off[k], sizeof(l3d_association) * assoc[id].size()) != 0) return 16;
    }
    // a subset in reversed order: every camera gets what it got among all
    const std::vector<unsigned int> pick = {sorted[2], sorted[0]};
    std::map<unsigned int, l3d_camera> cams3;
    std::map<unsigned int, l3d_pose_summary> sums3;
    l3d.refineCameras(cams3, sums3, max_distance, start_distance, max_angle, min_overlap, &pick);
    if (cams3.size() != 2) return 17;
    for (unsigned int id : pick)
        if (std::memcmp(&cams3[id], &cams[id], sizeof(l3d_camera)) != 0 || std::memcmp(&sums3[id], &sums[id], sizeof(l3d_pose_summary)) != 0) return 18;
    // the model and the views have not moved
    Lines after;
    l3d.get3Dlines(after);
    std::vector<double> q2;
    std::vector<uint32_t> line2;
    flatten(after, q2, line2);
    if (q2.size() != before.size() || std::memcmp(q2.data(), before.data(), 8 * before.size()) != 0) return 19;
    f = fopen(argv[2], "wb");
    if (!f) return 20;
    fwrite(&par, sizeof par, 1, f);
    fwrite(&nv, 4, 1, f);
    const uint32_t n_model = (uint32_t)line.size();
    fwrite(&n_model, 4, 1, f);
    fwrite(before.data(), 8, before.size(), f);
    fwrite(line.data(), 4, line.size(), f);
    uint32_t converged = 0;
    for (uint32_t k = 0; k < nv; ++k) {
        const uint32_t id = sorted[k];
        l3d_camera in;
        if (l3d_view_camera(l3d.handle(), id, &in) != L3D_OK) return 21;
        const uint32_t m = (uint32_t)assoc[id].size();
        fwrite(&id, 4, 1, f);
        fwrite(&in, sizeof in, 1, f);
        fwrite(&m, 4, 1, f);
        fwrite(&cams[id], sizeof(l3d_camera), 1, f);
        fwrite(&sums[id], sizeof(l3d_pose_summary), 1, f);
        fwrite(assoc[id].data(), sizeof(l3d_association), m, f);
        converged += sums[id].status == L3D_POSE_CONVERGED;
    }
    fclose(f);
    printf("RESULT views=%u converged=%u\n", nv, converged);
    return 0;
}
