// l3d_io.hip -- the input side of the matching path behind the C-ABI (host code; line3dpp_amd/io.py reads through it,
// and tests/test_input_formats.py holds it against the Python model of the formats, tests/sfm_readers_model.py):
//   * VisualSfM .nvm as main_vsfm.cpp:144-250 reads it (two ignored lines, the number of cameras, one line per camera:
//     file name, focal length, quaternion w x y z, centre, radial distortion; an ignored line, the number of points, one
//     line per point: position, colour, number of measurements, then camera index, feature index, x, y each) with what
//     main_vsfm.cpp derives per camera: R from the quaternion (:188-199), t = -R C, the ids of the points it sees
//     (= the worldpoint list handed to addImage) and the median of their distances (:300-303)
//   * the segment cache of Line3D::detectLineSegments (line3D.cc:295-309, 362-366): the boost binary archive of a
//     one-row L3DPP::DataArray<float4> (dataArray.h:352-374; host row padded to 32 bytes, :111-122)
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

#include "l3d_ctx.h"

struct l3d_nvm {
    struct Cam {
        std::string filename;
        float focal = 0, distortion = 0, median_depth = 0;
        double R[9], t[3], C[3];
        std::vector<uint32_t> worldpoints;
        std::vector<float> depths;
    };
    std::vector<Cam> cams;
};

extern "C" {

int l3d_nvm_open(const char* path, l3d_nvm** out) {
    if (!path || !out) return fail(L3D_ERR_ARG, "null argument");
    *out = nullptr;
    std::ifstream f(path);
    if (!f) return fail(L3D_ERR_ARG, std::string("cannot open ") + path);
    std::string line;
    std::getline(f, line); std::getline(f, line);             // two ignored lines
    std::getline(f, line);
    unsigned n_cams = 0;
    { std::stringstream s(line); s >> n_cams; }
    if (n_cams == 0) return fail(L3D_ERR_NO_VIEWS, "No aligned cameras in NVM file!");   // main_vsfm.cpp:157-161
    auto nvm = std::make_unique<l3d_nvm>();
    nvm->cams.resize(n_cams);
    for (unsigned i = 0; i < n_cams; ++i) {
        std::getline(f, line);
        std::stringstream s(line);
        double focal = 0, qw = 0, qx = 0, qy = 0, qz = 0, cx = 0, cy = 0, cz = 0, dist = 0;
        l3d_nvm::Cam& c = nvm->cams[i];
        s >> c.filename >> focal >> qw >> qx >> qy >> qz >> cx >> cy >> cz >> dist;
        c.focal = (float)focal; c.distortion = (float)dist;   // kept in float vectors there
        double* R = c.R;
        R[0] = 1.0 - 2.0 * qy * qy - 2.0 * qz * qz; R[1] = 2.0 * qx * qy - 2.0 * qz * qw; R[2] = 2.0 * qx * qz + 2.0 * qy * qw;
        R[3] = 2.0 * qx * qy + 2.0 * qz * qw; R[4] = 1.0 - 2.0 * qx * qx - 2.0 * qz * qz; R[5] = 2.0 * qy * qz - 2.0 * qx * qw;
        R[6] = 2.0 * qx * qz - 2.0 * qy * qw; R[7] = 2.0 * qy * qz + 2.0 * qx * qw; R[8] = 1.0 - 2.0 * qx * qx - 2.0 * qy * qy;
        c.C[0] = cx; c.C[1] = cy; c.C[2] = cz;
        const d3 rc = mul33(R, d3{cx, cy, cz});
        c.t[0] = -rc.x; c.t[1] = -rc.y; c.t[2] = -rc.z;
    }
    std::getline(f, line);                                    // ignored
    std::getline(f, line);
    unsigned n_pts = 0;
    { std::stringstream s(line); s >> n_pts; }
    for (unsigned i = 0; i < n_pts; ++i) {
        if (!std::getline(f, line)) break;
        std::istringstream s(line);
        double px = 0, py = 0, pz = 0, cr, cg, cb;
        unsigned n_meas = 0;
        s >> px >> py >> pz >> cr >> cg >> cb >> n_meas;
        for (unsigned j = 0; j < n_meas; ++j) {
            unsigned cam = 0, feat = 0; float x, y;
            s >> cam >> feat >> x >> y;
            if (!s || cam >= n_cams) return fail(L3D_ERR_ARG, "malformed measurement in NVM file");
            l3d_nvm::Cam& c = nvm->cams[cam];
            c.worldpoints.push_back(i);
            c.depths.push_back((float)norm(d3{px, py, pz} - d3{c.C[0], c.C[1], c.C[2]}));
        }
    }
    for (auto& c : nvm->cams)
        if (!c.depths.empty()) {                              // main_vsfm.cpp:300-303
            std::sort(c.depths.begin(), c.depths.end());
            c.median_depth = c.depths[c.depths.size() / 2];
        }
    *out = nvm.release();
    return L3D_OK;
}

uint32_t l3d_nvm_num_cameras(const l3d_nvm* n) { return n ? (uint32_t)n->cams.size() : 0u; }

int l3d_nvm_get_camera(const l3d_nvm* n, uint32_t i, l3d_nvm_camera* out) {
    if (!n || !out || i >= n->cams.size()) return fail(L3D_ERR_ARG, "bad argument");
    const l3d_nvm::Cam& c = n->cams[i];
    out->filename = c.filename.c_str();
    out->focal = c.focal; out->distortion = c.distortion; out->median_depth = c.median_depth;
    std::memcpy(out->R, c.R, 72); std::memcpy(out->t, c.t, 24); std::memcpy(out->C, c.C, 24);
    out->n_worldpoints = (uint32_t)c.worldpoints.size();
    return L3D_OK;
}

int l3d_nvm_get_worldpoints(const l3d_nvm* n, uint32_t i, uint32_t* out, uint32_t cap) {
    if (!n || i >= n->cams.size() || (cap && !out)) return fail(L3D_ERR_ARG, "bad argument");
    const auto& w = n->cams[i].worldpoints;
    if (cap && !w.empty()) std::memcpy(out, w.data(), 4 * (size_t)std::min<size_t>(cap, w.size()));
    return w.size() > cap ? fail(L3D_ERR_LIMIT, "worldpoint buffer too small") : L3D_OK;
}

void l3d_nvm_close(l3d_nvm* n) { delete n; }

// K as main_vsfm.cpp:272-282 builds it: principal point at the image centre, in float arithmetic
void l3d_nvm_intrinsics(float focal, uint32_t width, uint32_t height, double K[9]) {
    const float px = float(width) / 2.0f, py = float(height) / 2.0f;
    for (int i = 0; i < 9; ++i) K[i] = 0.0;
    K[0] = focal; K[4] = focal; K[2] = px; K[5] = py; K[8] = 1.0;
}

// ---- COLMAP result and bundler file: one handle type, one record per image ---------------------------------------------
// l3d_sfm_open_colmap: cameras.txt / images.txt / points3D.txt of a COLMAP result folder as main_colmap.cpp:136-348 reads
// them -- lines that start with '#' are skipped in the first two files; camera models SIMPLE_PINHOLE, PINHOLE,
// SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV (:177-219; the reference drops FULL_OPENCV's k4 k5 k6, here they are kept in
// the parameter list and l3d_sfm_get_camera_model hands them to the undistortion by camera model) and, beyond
// the reference, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE and FOV (K from their focal lengths and principal
// point, the five coefficients zero); anything else, THIN_PRISM_FISHEYE included, is an error (-3 there); without a
// cameras.txt, cameras.bin / images.bin / points3D.bin (COLMAP's binary model) fill the same records; images.txt alternates an
// image line (id, quaternion w x y z, t, camera id, name) with a line of 2D points (x y POINT3D_ID ...), of which the
// non-negative ids are the worldpoint list handed to addImage; an image whose camera is unknown is dropped (:281);
// R = rotationFromQ (line3D.cc:2730-2754: s = 2 / |q|^2, 0 for a vanishing quaternion), C = R^T (-t); points3D.txt: EVERY
// line is parsed as "id X Y Z" (the comment test there looks at the last line of images.txt, :333 -- a line that does
// not parse is left alone here); median depth = sorted float distances |C - X| [n / 2] over the image's list (:390-406,
// a point without a points3D entry sits at the origin like in the reference's map); images are kept in file order
// (img_seq), an image without worldpoints has n_worldpoints == 0 and is skipped by the caller like :389-410 does.
// l3d_sfm_open_bundler: bundle.rd.out as main_bundler.cpp:147-252 reads it -- an ignored line, "num_cams num_points",
// per camera focal / two radial coefficients, three rotation rows and the translation with the y and z rows / entries
// negated (:192-212), C = R^T (-t); per point a position line, an ignored colour line and the view list
// (count, then camera, key, x, y each); camera index = camID; median depth as above (:371-373).  K is built by the
// caller from the image size (l3d_nvm_intrinsics: the same construction, :341-350).
struct l3d_sfm {
    struct Img {
        uint32_t id = 0, cam = 0, width = 0, height = 0;
        std::string name;
        double K[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3], C[3], radial[3] = {0, 0, 0}, tangential[2] = {0, 0};
        float focal = 0, median_depth = 0;
        std::vector<uint32_t> worldpoints;
        std::string model;                                      // COLMAP's name of the camera model ("" for bundler)
        double params[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // cameras.txt's parameter list
        uint32_t n_params = 0;
    };
    std::vector<Img> imgs;
};

// Line3D::rotationFromQ, line3D.cc:2730-2754
static void rotation_from_q(double w, double x, double y, double z, double R[9]) {
    const double n = w * w + x * x + y * y + z * z;
    const double s = std::fabs(n) < kEps ? 0.0 : 2.0 / n;
    const double wx = s * w * x, wy = s * w * y, wz = s * w * z, xx = s * x * x, xy = s * x * y, xz = s * x * z;
    const double yy = s * y * y, yz = s * y * z, zz = s * z * z;
    R[0] = 1.0 - (yy + zz); R[1] = xy - wz; R[2] = xz + wy;
    R[3] = xy + wz; R[4] = 1.0 - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy; R[7] = yz + wx; R[8] = 1.0 - (xx + yy);
}
static void centre_from(const double R[9], const double t[3], double C[3]) {   // R^T (-1 t), Eigen's product order
    const M3 Rm{{R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]}};
    const d3 c = mul33(m3_t(Rm).m, d3{-1.0 * t[0], -1.0 * t[1], -1.0 * t[2]});
    C[0] = c.x; C[1] = c.y; C[2] = c.z;
}
static float median_of(std::vector<float>& d) { std::sort(d.begin(), d.end()); return d[d.size() / 2]; }

// ---- COLMAP: the records both parsers fill, and the code behind them -----------------------------------------------
extern "C++" {
namespace {

// COLMAP's camera models in the order of their binary ids, with the length of their parameter lists.  Models 0-4 and 6
// are main_colmap.cpp's (:177-219); 5, 7, 8, 9 are undistorted by camera model; 10 stays unknown.
struct ColmapModel { const char* name; uint32_t n_params; bool known; };
const ColmapModel kColmapModels[] = {
    {"SIMPLE_PINHOLE", 3, true}, {"PINHOLE", 4, true}, {"SIMPLE_RADIAL", 4, true}, {"RADIAL", 5, true},
    {"OPENCV", 8, true}, {"OPENCV_FISHEYE", 8, true}, {"FULL_OPENCV", 12, true}, {"FOV", 5, true},
    {"SIMPLE_RADIAL_FISHEYE", 4, true}, {"RADIAL_FISHEYE", 5, true}, {"THIN_PRISM_FISHEYE", 12, false}};

struct ColmapCam {
    std::string model;
    uint32_t w = 0, h = 0, n_params = 0;
    double params[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double K[9], radial[3], tangential[2];
};
struct ColmapImage {                       // an image of images.txt / images.bin
    uint32_t id = 0, cam = 0;
    double q[4] = {0, 0, 0, 0}, t[3] = {0, 0, 0};
    std::string name;
    bool has_points = false;               // the line of 2D points was there (text: the file may end before it)
    std::vector<int> point_ids;            // POINT3D_ID of every 2D point, as atoi gives it
};
struct ColmapPoint { uint32_t id; double X, Y, Z; };

// K and the five coefficients of undistortImage from a model's parameter list (p: 12 values, missing ones 0)
bool colmap_camera(const std::string& model, const double* p, ColmapCam& c) {
    double fx = 0, fy = 0, cx = 0, cy = 0, k1 = 0, k2 = 0, k3 = 0, p1 = 0, p2 = 0;
    uint32_t idx = 0;
    for (; idx < 11; ++idx)
        if (model == kColmapModels[idx].name) break;
    if (idx == 11 || !kColmapModels[idx].known) return false;
    if (model == "SIMPLE_PINHOLE") { fx = p[0]; cx = p[1]; cy = p[2]; fy = fx; }
    else if (model == "PINHOLE" || model == "FOV" || model == "OPENCV_FISHEYE") { fx = p[0]; fy = p[1]; cx = p[2]; cy = p[3]; }
    else if (model == "SIMPLE_RADIAL") { fx = p[0]; cx = p[1]; cy = p[2]; k1 = p[3]; fy = fx; }
    else if (model == "RADIAL") { fx = p[0]; cx = p[1]; cy = p[2]; k1 = p[3]; k2 = p[4]; fy = fx; }
    else if (model == "SIMPLE_RADIAL_FISHEYE" || model == "RADIAL_FISHEYE") { fx = p[0]; cx = p[1]; cy = p[2]; fy = fx; }
    else if (model == "OPENCV") { fx = p[0]; fy = p[1]; cx = p[2]; cy = p[3]; k1 = p[4]; k2 = p[5]; p1 = p[6]; p2 = p[7]; }
    else { fx = p[0]; fy = p[1]; cx = p[2]; cy = p[3]; k1 = p[4]; k2 = p[5]; p1 = p[6]; p2 = p[7]; k3 = p[8]; }   // FULL_OPENCV
    c.model = model;
    c.n_params = kColmapModels[idx].n_params;
    for (uint32_t k = 0; k < 12; ++k) c.params[k] = k < c.n_params ? p[k] : 0.0;
    const double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    std::memcpy(c.K, K, 72);
    c.radial[0] = k1; c.radial[1] = k2; c.radial[2] = k3; c.tangential[0] = p1; c.tangential[1] = p2;
    return true;
}

// what main_colmap.cpp derives from the three files (:236-348, :390-406), whichever form they were read in
void colmap_build(const std::map<uint32_t, ColmapCam>& cams, const std::vector<ColmapImage>& images,
                  const std::vector<ColmapPoint>& points, l3d_sfm& sfm) {
    std::map<uint32_t, size_t> by_id;                          // image id -> record (a repeated id overwrites, like the maps there)
    std::map<uint32_t, d3> wps;                                // worldpoints seen in the images (origin until points3D says otherwise)
    for (const ColmapImage& r : images) {
        auto ci = cams.find(r.cam);
        if (ci == cams.end()) continue;                        // unknown camera: dropped (:281)
        const ColmapCam& cam = ci->second;
        l3d_sfm::Img im;
        im.id = r.id; im.cam = r.cam; im.name = r.name; im.width = cam.w; im.height = cam.h;
        std::memcpy(im.K, cam.K, 72); std::memcpy(im.radial, cam.radial, 24); std::memcpy(im.tangential, cam.tangential, 16);
        im.model = cam.model; im.n_params = cam.n_params; std::memcpy(im.params, cam.params, 96);
        rotation_from_q(r.q[0], r.q[1], r.q[2], r.q[3], im.R);
        im.t[0] = r.t[0]; im.t[1] = r.t[1]; im.t[2] = r.t[2];
        centre_from(im.R, im.t, im.C);
        im.focal = (float)im.K[0];
        auto it = by_id.find(r.id);
        if (it == by_id.end()) { by_id[r.id] = sfm.imgs.size(); sfm.imgs.push_back(im); }
        else { im.worldpoints = sfm.imgs[it->second].worldpoints; sfm.imgs[it->second] = im; sfm.imgs.push_back(im); by_id[r.id] = sfm.imgs.size() - 1; }
        if (r.has_points) {
            std::vector<uint32_t> list;
            for (int id : r.point_ids)
                if (id >= 0) { list.push_back((uint32_t)id); wps[(uint32_t)id] = d3{0, 0, 0}; }
            sfm.imgs[by_id[r.id]].worldpoints = list;
        }
    }
    for (const ColmapPoint& p : points) {
        auto it = wps.find(p.id);
        if (it != wps.end()) it->second = d3{p.X, p.Y, p.Z};
    }
    // a repeated image id: img_seq holds it twice, both entries see the LAST pose and list (the maps are keyed by id)
    for (auto& im : sfm.imgs) { const l3d_sfm::Img& last = sfm.imgs[by_id[im.id]]; if (&last != &im) im = last; }
    for (auto& im : sfm.imgs) {
        std::vector<float> depths;
        for (uint32_t w : im.worldpoints) depths.push_back((float)norm(d3{im.C[0], im.C[1], im.C[2]} - wps[w]));
        if (!depths.empty()) im.median_depth = median_of(depths);
    }
}

// a COLMAP binary file in memory, read with a cursor that never passes its end
struct BinFile {
    std::string name;
    std::vector<char> buf;
    size_t pos = 0;
    bool open(const std::string& dir, const char* file) {
        name = file;
        std::ifstream f(dir + "/" + file, std::ios::binary);
        if (!f) return false;
        buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        return true;
    }
    size_t left() const { return buf.size() - pos; }
    template <class T> bool get(T& v) {
        if (left() < sizeof(T)) return false;
        std::memcpy(&v, buf.data() + pos, sizeof(T));          // (little-endian, as the hosts of this library are)
        pos += sizeof(T);
        return true;
    }
    bool doubles(double* v, size_t n) {
        if (left() / 8 < n) return false;
        std::memcpy(v, buf.data() + pos, 8 * n);
        pos += 8 * n;
        return true;
    }
    int truncated() const { return fail(L3D_ERR_IO, name + ": the file ends inside a record (truncated?)"); }
    int too_many(uint64_t n, const char* what) const {
        return fail(L3D_ERR_IO, name + ": " + std::to_string(n) + " " + what + " cannot fit in the " + std::to_string(left()) + " bytes that follow");
    }
    int finish() const { return pos == buf.size() ? L3D_OK : fail(L3D_ERR_IO, name + ": " + std::to_string(left()) + " bytes behind the last record"); }
};

// POINT3D_ID of images.bin as the text reader's atoi sees the same number in decimal: strtol saturates at LONG_MAX and
// the int keeps its low 32 bits, so 2^64 - 1 ("no point") is -1
int atoi_of(uint64_t id) { return (int)(long)std::min<uint64_t>(id, (uint64_t)LONG_MAX); }

int colmap_read_binary(const std::string& dir, std::map<uint32_t, ColmapCam>& cams, std::vector<ColmapImage>& images,
                       std::vector<ColmapPoint>& points) {
    BinFile fc, fi, fp;
    if (!fc.open(dir, "cameras.bin") || !fi.open(dir, "images.bin") || !fp.open(dir, "points3D.bin"))
        return fail(L3D_ERR_ARG, "at least one of the colmap result files does not exist in sfm folder: " + dir);
    uint64_t n = 0;
    if (!fc.get(n)) return fc.truncated();
    if (n > fc.left() / 48) return fc.too_many(n, "cameras");           // a camera is at least 24 + 3 x 8 bytes
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t id = 0; int32_t model = 0; uint64_t w = 0, h = 0;
        if (!fc.get(id) || !fc.get(model) || !fc.get(w) || !fc.get(h)) return fc.truncated();
        if (model < 0 || model > 10 || !kColmapModels[model].known)
            return fail(L3D_ERR_ARG, "camera model " + (model >= 0 && model <= 10 ? std::string(kColmapModels[model].name) : std::to_string(model)) + " unknown!");
        if (w > UINT32_MAX || h > UINT32_MAX) return fail(L3D_ERR_IO, fc.name + ": image size of camera " + std::to_string(id) + " beyond 32 bits");
        double p[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!fc.doubles(p, kColmapModels[model].n_params)) return fc.truncated();
        ColmapCam c;
        colmap_camera(kColmapModels[model].name, p, c);
        c.w = (uint32_t)w; c.h = (uint32_t)h;
        cams[id] = c;
    }
    if (int rc = fc.finish()) return rc;
    if (!fi.get(n)) return fi.truncated();
    if (n > fi.left() / 73) return fi.too_many(n, "images");            // an image with an empty name and no points
    images.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        ColmapImage r;
        uint64_t m = 0;
        if (!fi.get(r.id) || !fi.doubles(r.q, 4) || !fi.doubles(r.t, 3) || !fi.get(r.cam)) return fi.truncated();
        const char* s = fi.buf.data() + fi.pos;
        const void* z = std::memchr(s, 0, fi.left());
        if (!z) return fi.truncated();
        r.name.assign(s, (const char*)z);
        fi.pos += r.name.size() + 1;
        if (!fi.get(m)) return fi.truncated();
        if (m > fi.left() / 24) return fi.too_many(m, "2D points");
        r.has_points = true;
        r.point_ids.reserve(m);
        for (uint64_t k = 0; k < m; ++k) {
            double xy[2]; uint64_t pid = 0;
            if (!fi.doubles(xy, 2) || !fi.get(pid)) return fi.truncated();
            r.point_ids.push_back(atoi_of(pid));
        }
        images.push_back(std::move(r));
    }
    if (int rc = fi.finish()) return rc;
    if (!fp.get(n)) return fp.truncated();
    if (n > fp.left() / 51) return fp.too_many(n, "3D points");         // a point with an empty track
    points.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t id = 0, track = 0; double xyz[3], err = 0; uint8_t rgb[3];
        if (!fp.get(id) || !fp.doubles(xyz, 3) || !fp.get(rgb) || !fp.get(err) || !fp.get(track)) return fp.truncated();
        if (track > fp.left() / 8) return fp.too_many(track, "track elements");
        fp.pos += 8 * track;
        if (id <= UINT32_MAX) points.push_back(ColmapPoint{(uint32_t)id, xyz[0], xyz[1], xyz[2]});   // (the text reader's `>> uint32_t` fails beyond)
    }
    return fp.finish();
}

}  // namespace
}  // extern "C++"

int l3d_sfm_open_colmap(const char* folder, l3d_sfm** out) {
    if (!folder || !out) return fail(L3D_ERR_ARG, "null argument");
    *out = nullptr;
    const std::string dir(folder);
    std::map<uint32_t, ColmapCam> cams;
    std::vector<ColmapImage> images;
    std::vector<ColmapPoint> points;
    std::ifstream fc(dir + "/cameras.txt");
    if (!fc) {
        // COLMAP's binary model, its default output: taken when there is no cameras.txt and all three .bin files exist
        const bool bin = std::ifstream(dir + "/cameras.bin").good() && std::ifstream(dir + "/images.bin").good() &&
                         std::ifstream(dir + "/points3D.bin").good();
        if (!bin) return fail(L3D_ERR_ARG, "at least one of the colmap result files does not exist in sfm folder: " + dir);
        if (int rc = colmap_read_binary(dir, cams, images, points)) return rc;
    } else {
        std::ifstream fi(dir + "/images.txt"), fp(dir + "/points3D.txt");
        if (!fi || !fp) return fail(L3D_ERR_ARG, "at least one of the colmap result files does not exist in sfm folder: " + dir);
        std::string line;
        while (std::getline(fc, line)) {
            if (line.substr(0, 1) == "#") continue;
            std::stringstream s(line);
            uint32_t id = 0, w = 0, h = 0; std::string model;
            s >> id >> model >> w >> h;
            double p[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t np = 0;
            for (const ColmapModel& m : kColmapModels)
                if (m.known && model == m.name) np = m.n_params;
            for (uint32_t k = 0; k < np; ++k) {
                double v = 0;
                s >> v;
                p[k] = v;
            }
            ColmapCam c;
            if (!colmap_camera(model, p, c)) return fail(L3D_ERR_ARG, "camera model " + model + " unknown!");
            c.w = w; c.h = h;
            cams[id] = c;
        }
        bool first = true;
        uint32_t img_id = 0, cam_id = 0;                       // (outside the loop as there: a line that does not parse keeps the last camera id)
        while (std::getline(fi, line)) {
            if (line.substr(0, 1) == "#") continue;
            std::stringstream s(line);
            if (first) {
                ColmapImage r;
                s >> img_id >> r.q[0] >> r.q[1] >> r.q[2] >> r.q[3] >> r.t[0] >> r.t[1] >> r.t[2] >> cam_id >> r.name;
                r.id = img_id; r.cam = cam_id;
                images.push_back(r);
                first = false;
            } else {
                ColmapImage& r = images.back();
                if (cams.count(r.cam)) {
                    r.has_points = true;
                    for (;;) {
                        double x, y; std::string wp;
                        s >> x >> y >> wp;
                        if (wp.empty()) break;
                        r.point_ids.push_back(std::atoi(wp.c_str()));
                    }
                }
                first = true;
            }
        }
        while (std::getline(fp, line)) {
            std::stringstream s(line);
            uint32_t id = 0; double X = 0, Y = 0, Z = 0;
            s >> id >> X >> Y >> Z;
            if (!s) continue;                                  // (a comment or malformed line)
            points.push_back(ColmapPoint{id, X, Y, Z});
        }
    }
    auto sfm = std::make_unique<l3d_sfm>();
    colmap_build(cams, images, points, *sfm);
    *out = sfm.release();
    return L3D_OK;
}

int l3d_sfm_open_bundler(const char* path, l3d_sfm** out) {
    if (!path || !out) return fail(L3D_ERR_ARG, "null argument");
    *out = nullptr;
    std::ifstream f(path);
    if (!f) return fail(L3D_ERR_ARG, std::string("bundle file '") + path + "' does not exist!");
    std::string line;
    std::getline(f, line); std::getline(f, line);             // first line ignored
    uint32_t n_cams = 0, n_pts = 0;
    { std::stringstream s(line); s >> n_cams >> n_pts; }
    if (n_cams == 0 || n_pts == 0) return fail(L3D_ERR_NO_VIEWS, "No cameras and/or points in bundle file!");   // main_bundler.cpp:160-164
    auto sfm = std::make_unique<l3d_sfm>();
    sfm->imgs.resize(n_cams);
    auto next = [&](std::stringstream& s) { std::getline(f, line); s.str(""); s.clear(); s.str(line); };
    std::stringstream s;
    for (uint32_t i = 0; i < n_cams; ++i) {
        l3d_sfm::Img& im = sfm->imgs[i];
        im.id = i; im.cam = i;
        double focal = 0, d1 = 0, d2 = 0;
        next(s); s >> focal >> d1 >> d2;
        im.focal = (float)focal; im.radial[0] = (double)(float)d1; im.radial[1] = (double)(float)d2;   // (float pairs there, :170-176)
        for (int j = 0; j < 3; ++j) { next(s); s >> im.R[3 * j] >> im.R[3 * j + 1] >> im.R[3 * j + 2]; }
        for (int k = 3; k < 9; ++k) im.R[k] *= -1.0;          // flip 2nd and 3rd line
        next(s); s >> im.t[0] >> im.t[1] >> im.t[2];
        im.t[1] *= -1.0; im.t[2] *= -1.0;
        centre_from(im.R, im.t, im.C);
    }
    std::vector<std::vector<float>> depths(n_cams);
    for (uint32_t i = 0; i < n_pts; ++i) {
        double px = 0, py = 0, pz = 0;
        if (!std::getline(f, line)) break;
        { std::istringstream p(line); p >> px >> py >> pz; }
        std::getline(f, line);                                // colour
        std::getline(f, line);
        std::istringstream v(line);
        uint32_t n_views = 0;
        v >> n_views;
        for (uint32_t j = 0; j < n_views; ++j) {
            uint32_t cam = 0, key = 0; float x, y;
            v >> cam >> key >> x >> y;
            if (!v || cam >= n_cams) return fail(L3D_ERR_ARG, "malformed view list in bundle file");
            sfm->imgs[cam].worldpoints.push_back(i);
            depths[cam].push_back((float)norm(d3{px, py, pz} - d3{sfm->imgs[cam].C[0], sfm->imgs[cam].C[1], sfm->imgs[cam].C[2]}));
        }
    }
    for (uint32_t i = 0; i < n_cams; ++i) if (!depths[i].empty()) sfm->imgs[i].median_depth = median_of(depths[i]);
    *out = sfm.release();
    return L3D_OK;
}

uint32_t l3d_sfm_num_images(const l3d_sfm* s) { return s ? (uint32_t)s->imgs.size() : 0u; }

int l3d_sfm_get_image(const l3d_sfm* s, uint32_t i, l3d_sfm_image* out) {
    if (!s || !out || i >= s->imgs.size()) return fail(L3D_ERR_ARG, "bad argument");
    const l3d_sfm::Img& im = s->imgs[i];
    out->id = im.id; out->camera = im.cam; out->width = im.width; out->height = im.height; out->name = im.name.c_str();
    out->focal = im.focal; out->median_depth = im.median_depth; out->n_worldpoints = (uint32_t)im.worldpoints.size();
    std::memcpy(out->K, im.K, 72); std::memcpy(out->R, im.R, 72); std::memcpy(out->t, im.t, 24); std::memcpy(out->C, im.C, 24);
    std::memcpy(out->radial, im.radial, 24); std::memcpy(out->tangential, im.tangential, 16);
    return L3D_OK;
}

int l3d_sfm_get_worldpoints(const l3d_sfm* s, uint32_t i, uint32_t* out, uint32_t cap) {
    if (!s || i >= s->imgs.size() || (cap && !out)) return fail(L3D_ERR_ARG, "bad argument");
    const auto& w = s->imgs[i].worldpoints;
    if (cap && !w.empty()) std::memcpy(out, w.data(), 4 * (size_t)std::min<size_t>(cap, w.size()));
    return w.size() > cap ? fail(L3D_ERR_LIMIT, "worldpoint buffer too small") : L3D_OK;
}

void l3d_sfm_close(l3d_sfm* s) { delete s; }

int l3d_sfm_get_camera_model(const l3d_sfm* s, uint32_t i, l3d_camera_model* out) {
    if (!s || !out || i >= s->imgs.size()) return fail(L3D_ERR_ARG, "bad argument");
    const l3d_sfm::Img& im = s->imgs[i];
    *out = l3d_camera_model{};
    std::memcpy(out->K, im.K, 72);
    // (model, first distortion parameter in the list, their number)
    struct { const char* name; uint32_t model, first, n; } const forms[] = {
        {"FULL_OPENCV", L3D_CAM_FULL_OPENCV, 4, 8}, {"OPENCV_FISHEYE", L3D_CAM_OPENCV_FISHEYE, 4, 4},
        {"SIMPLE_RADIAL_FISHEYE", L3D_CAM_SIMPLE_RADIAL_FISHEYE, 3, 1}, {"RADIAL_FISHEYE", L3D_CAM_RADIAL_FISHEYE, 3, 2},
        {"FOV", L3D_CAM_FOV, 4, 1}};
    for (const auto& f : forms)
        if (im.model == f.name) {
            out->model = f.model;
            for (uint32_t k = 0; k < f.n; ++k) out->params[k] = im.params[f.first + k];
        }
    return L3D_OK;
}

const char* l3d_sfm_get_camera_params(const l3d_sfm* s, uint32_t i, double* params, uint32_t cap, uint32_t* n) {
    if (n) *n = 0;
    if (!s || i >= s->imgs.size() || (cap && !params)) { fail(L3D_ERR_ARG, "bad argument"); return nullptr; }
    const l3d_sfm::Img& im = s->imgs[i];
    if (n) *n = im.n_params;
    for (uint32_t k = 0; k < std::min(cap, im.n_params); ++k) params[k] = im.params[k];
    return im.model.c_str();
}



// ---- segment cache ----------------------------------------------------------------------------------------------------
static const char kArchiveSig[] = "serialization::archive";            // 22 characters
static const unsigned char kPlatform[8] = {4, 8, 4, 8, 1, 0, 0, 0};   // sizes of int, long, float, double; endianness
static const unsigned char kClassHdr[5] = {0, 0, 0, 0, 0};

int l3d_segment_cache_name(uint32_t camID, uint32_t width, uint32_t height, uint32_t max_segments, char* out, uint32_t cap) {
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    const int n = std::snprintf(out, cap, "segments_L3D++_%u_%ux%u_%u.bin", camID, width, height, max_segments);   // line3D.cc:300
    return (n < 0 || (uint32_t)n >= cap) ? fail(L3D_ERR_LIMIT, "name buffer too small") : L3D_OK;
}

int l3d_write_segment_cache(const char* path, const float* segs4, uint32_t n) {
    if (!path || (n && !segs4)) return fail(L3D_ERR_ARG, "null argument");
    const uint32_t real = n + (((uint64_t)n * 16) % 32 ? 1u : 0u);     // host row padded to 32 bytes
    std::string b;
    auto put = [&](const void* p, size_t k) { b.append((const char*)p, k); };
    const uint64_t sig_len = sizeof(kArchiveSig) - 1; const uint16_t lib_version = 10;
    put(&sig_len, 8); put(kArchiveSig, sig_len); put(&lib_version, 2); put(kPlatform, 8);
    put(kClassHdr, 5);
    const uint32_t w = n, h = 1; const uint64_t pitch = (uint64_t)real * 16, stride = real, zero = 0;
    put(&w, 4); put(&h, 4); put(&real, 4); put(&pitch, 8); put(&stride, 8); put(&zero, 8); put(&zero, 8);
    if (real) put(kClassHdr, 5);
    if (n) put(segs4, (size_t)n * 16);
    if (real > n) { const float pad[4] = {0, 0, 0, 0}; put(pad, 16); }
    std::ofstream f(path, std::ios::binary);
    if (!f || !f.write(b.data(), (std::streamsize)b.size())) return fail(L3D_ERR_ARG, std::string("cannot write ") + path);
    return L3D_OK;
}

int l3d_read_segment_cache(const char* path, float* segs4, uint32_t cap, uint32_t* n) {
    if (!path || !n) return fail(L3D_ERR_ARG, "null argument");
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail(L3D_ERR_ARG, std::string("cannot open ") + path);
    std::string b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t p = 0;
    auto take = [&](void* dst, size_t k) { if (p + k > b.size()) return false; std::memcpy(dst, b.data() + p, k); p += k; return true; };
    auto expect = [&](const void* want, size_t k) { if (p + k > b.size() || std::memcmp(b.data() + p, want, k)) return false; p += k; return true; };
    uint64_t sig_len = 0; uint16_t lib_version = 0;
    if (!take(&sig_len, 8) || sig_len != sizeof(kArchiveSig) - 1 || !expect(kArchiveSig, sig_len) || !take(&lib_version, 2))
        return fail(L3D_ERR_ARG, "not a boost binary archive");
    if (!expect(kPlatform, 8)) return fail(L3D_ERR_ARG, "written on a platform with other type sizes / endianness");
    uint32_t w = 0, h = 0, real = 0; uint64_t pitch = 0, stride = 0, pg = 0, sg = 0;
    if (!expect(kClassHdr, 5) || !take(&w, 4) || !take(&h, 4) || !take(&real, 4) || !take(&pitch, 8) || !take(&stride, 8) ||
        !take(&pg, 8) || !take(&sg, 8))
        return fail(L3D_ERR_ARG, "truncated DataArray<float4> header");
    if (h != 1 || real < w || pitch != (uint64_t)real * 16 || stride != real)
        return fail(L3D_ERR_ARG, "not a one-row DataArray<float4>");
    if (real && !expect(kClassHdr, 5)) return fail(L3D_ERR_ARG, "unexpected class header for float4");
    if (p + (size_t)real * 16 != b.size()) return fail(L3D_ERR_ARG, "wrong archive length");
    *n = w;
    if (segs4) std::memcpy(segs4, b.data() + p, 16 * (size_t)std::min(cap, w));
    return (segs4 && w > cap) ? fail(L3D_ERR_LIMIT, "segment buffer too small") : L3D_OK;
}

}  // extern "C"
