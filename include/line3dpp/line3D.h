// line3dpp/line3D.h -- header-only C++ facade over the C-ABI (include/l3dpp_hip.h) that mirrors the
// public interface of the reference's class L3DPP::Line3D (line3D.h:61-424) for the hot path:
//
//     Line3D(output_folder, load_segments, max_img_width, max_line_segments,
//            neighbors_by_worldpoints=false, use_GPU=true)
//     static undistortImage(inImg, outImg, radial_coeffs, tangential_coeffs, K)
//     static undistortImage(inImg, outImg, model, params, K[, K_new])   (COLMAP's camera models beyond five coefficients)
//     addImage(camID, image, K, R, t, median_depth, wps_or_neighbors, line_segments)
//     matchImages(sigma_position, sigma_angle, num_neighbors, epipolar_overlap, kNN, const_regularization_depth)
//     computeAffinityMatrix()            // the affinity part of reconstruct3Dlines()
//     projectLines(camID | K, R, t, width, height, out)    (no reference counterpart: the 3D lines as a camera sees them)
//     drawLines(camID | K, R, t, inImg, outImg, thickness, alpha)      (... drawn over an image)
//     associateSegments([camID,] out, max_distance, max_angle, min_overlap)   (... and the 2D segments that observe them)
//     compareLines(other, mine, theirs, max_distance, max_angle, min_overlap)   (... and compared with another model)
//     mergeLines(max_distance, max_angle, min_overlap)                           (... and their near-duplicates merged)
//     alignLines(other, similarity, summary, max_distance, start_distance, ...)  (... and aligned to a model in another frame)
//     refineCameras(cameras, summaries, max_distance, start_distance, ...)       (... and the views' poses refined against them)
//     refitLines(cameras, max_distance, max_angle, min_overlap, visibility, ...) (... and the lines refit against the views' segments)
//     bundleModel(cameras, max_distance, max_angle, min_overlap, visibility, ...) (cameras and lines bundled jointly)
//     wireframe(max_distance, max_extension, min_angle)                          (... and where they meet: junctions, vertices, edges)
//     detectPlanes(max_distance, junction_distance, junction_extension, min_angle, ...)   (... and the planes they lie in)
//     detectDirections(max_angle, min_length, min_segments, max_directions, max_tests, frame_angle)   (... the directions they run in)
//
// Same names, argument order, defaults (commons.h:40-70) and error behaviour as the reference: errors
// are printed with the "[L3D++] ERROR:" prefix and the call returns (void), no exceptions
// (line3D.cc:119-126, 385-391).  The matrix/vector/image types are template parameters, so Eigen
// (Matrix3d / Vector3d: operator()(r,c), operator()(i)) and OpenCV (cv::Mat: .cols/.rows; cv::Vec4f:
// operator[]) objects can be passed exactly as to the reference without this header depending on
// either library.  After matchImages()/computeAffinityMatrix() the results are available in the
// reference's own container types -- see matches(), estimatedPosition3D(), affinity() -- so the
// reference's clusterSegments()/optimizeClusters() stages can consume them unchanged
// (INTEGRATION.md shows the ten-line patch).
#ifndef L3DPP_HIP_FACADE_LINE3D_H_
#define L3DPP_HIP_FACADE_LINE3D_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <iostream>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../l3dpp_hip.h"

namespace L3DPP_HIP {

// defaults, commons.h:40-70
constexpr float L3D_DEF_SCORING_POS_REGULARIZER = 2.5f;
constexpr float L3D_DEF_SCORING_ANG_REGULARIZER = 10.0f;
constexpr unsigned L3D_DEF_MATCHING_NEIGHBORS = 10;
constexpr float L3D_DEF_EPIPOLAR_OVERLAP = 0.25f;
constexpr int L3D_DEF_KNN = 10;

struct ImageSize { int cols, rows; };  // stand-in for cv::Mat when OpenCV is not around (size only: give segments)

// stand-in for an 8-bit cv::Mat with pixels: grey (channels 1, CV_8U) or RGB (channels 3, CV_8UC3, first channel = R);
// step = bytes per row.  addImage detects the segments of such an image when it is given none.
struct Image8U {
    const unsigned char* data;
    int cols, rows, channels_;
    size_t step;
    int channels() const { return channels_; }
    int type() const { return channels_ == 1 ? 0 : channels_ == 3 ? 16 : -1; }   // CV_8U, CV_8UC3
};

// owning stand-in for an 8-bit cv::Mat with pixels, for users without OpenCV: what undistortImage writes into (create /
// release as cv::Mat has them).  It has data, cols, rows, step and type(), so addImage detects on it as it is.
class ImageBuf8U {
public:
    unsigned char* data = nullptr;
    int cols = 0, rows = 0;
    size_t step = 0;

    ImageBuf8U() = default;
    ImageBuf8U(int rows_, int cols_, int type_) { create(rows_, cols_, type_); }
    ImageBuf8U(const ImageBuf8U& o) : data(nullptr), cols(o.cols), rows(o.rows), step(o.step), buf_(o.buf_), type_(o.type_) {
        if (!buf_.empty()) data = buf_.data();
    }
    ImageBuf8U(ImageBuf8U&& o) noexcept : ImageBuf8U() { swap(o); }
    ImageBuf8U& operator=(ImageBuf8U o) noexcept { swap(o); return *this; }
    void swap(ImageBuf8U& o) noexcept {
        std::swap(data, o.data); std::swap(cols, o.cols); std::swap(rows, o.rows); std::swap(step, o.step);
        buf_.swap(o.buf_); std::swap(type_, o.type_);
    }

    // cv::Mat::create: rows x cols pixels of type CV_8U (0) or CV_8UC3 (16), rows packed; kept when they already are
    void create(int rows_, int cols_, int type) {
        const size_t ch = type == 16 ? 3 : 1;
        if (rows_ == rows && cols_ == cols && type == type_ && data) return;
        buf_.assign((size_t)rows_ * cols_ * ch, 0);
        rows = rows_; cols = cols_; type_ = type; step = (size_t)cols_ * ch;
        data = buf_.empty() ? nullptr : buf_.data();
    }
    void release() { ImageBuf8U().swap(*this); }
    bool empty() const { return data == nullptr; }
    int channels() const { return type_ == 16 ? 3 : 1; }
    int type() const { return type_; }

private:
    std::vector<unsigned char> buf_;
    int type_ = 0;
};

namespace detail {
template <class I, class = void> struct has_pixels : std::false_type {};
template <class I>
struct has_pixels<I, std::void_t<decltype(std::declval<const I&>().data), decltype(std::declval<const I&>().type()),
                                 decltype(std::declval<const I&>().step)>> : std::true_type {};
}  // namespace detail

class Line3D {
public:
    Line3D(const std::string& output_folder, const bool load_segments = true, const int max_img_width = -1,
           const unsigned int max_line_segments = 3000, const bool neighbors_by_worldpoints = false,
           const bool use_GPU = true, const int device = 0, void* hip_stream = nullptr)
        : prefix_("[L3D++] "), prefix_err_("[L3D++] ERROR: ") {
        (void)use_GPU;
        output_folder_ = output_folder;
        load_segments_ = load_segments;
        max_img_width_ = max_img_width;
        max_line_segments_ = max_line_segments;
        // addImage's list is a worldpoint list; neighbours from the worldpoint overlap at every matchImages
        // (Line3D::findVisualNeighborsFromWPs, line3D.cc:578-699 -> l3d_add_view_worldpoints)
        neighbors_by_worldpoints_ = neighbors_by_worldpoints;
        ctx_ = l3d_create(device, hip_stream);
        if (!ctx_) std::cout << prefix_err_ << l3d_last_error() << std::endl;
    }
    ~Line3D() { l3d_destroy(ctx_); }
    Line3D(const Line3D&) = delete;
    Line3D& operator=(const Line3D&) = delete;

    // void Line3D::addImage(...), line3D.h:104-108.  Image: anything with .cols/.rows; Mat3: K(r,c);
    // Vec3: t(i); Seg: s[0..3] (cv::Vec4f).  Empty `line_segments` and an image with pixels (.data, .step, .type() as
    // cv::Mat, Image8U or ImageBuf8U has them): the segments are detected on the GPU, or read from the segment cache with
    // load_segments (line3D.cc:168-173, 243-370).  Detection expects undistorted pixels: undistortImage below is what the
    // reference's front ends call first.  A size-only image (ImageSize) needs its segments.  [multithreading safe like the reference;
    // detection holds the context mutex, so image views added from several threads are detected one after another:
    // about 7 s per 3072x2304 image.  A front end with many images detects them in one batch with
    // l3d_detect_view_segments and hands each view its segments -- the batch costs about what one image does.]
    template <class Image, class Mat3, class Vec3, class Seg>
    void addImage(const unsigned int camID, const Image& image, const Mat3& K, const Mat3& R, const Vec3& t,
                  const float median_depth, const std::list<unsigned int>& wps_or_neighbors,
                  const std::vector<Seg>& line_segments) {
        double k[9], r[9], tt[3];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { k[3 * i + j] = K(i, j); r[3 * i + j] = R(i, j); }
            tt[i] = t(i);
        }
        std::vector<uint32_t> nb(wps_or_neighbors.begin(), wps_or_neighbors.end());
        if constexpr (detail::has_pixels<Image>::value) {
            if (line_segments.empty()) {
                const int ty = image.type();
                const l3d_image im{(const uint8_t*)image.data, (uint32_t)image.cols, (uint32_t)image.rows,
                                   ty == 0 ? 1u : ty == 16 ? 3u : 0u, (uint32_t)(size_t)image.step};
                const l3d_detect_options o{output_folder_.c_str(), load_segments_ ? 1 : 0, max_img_width_, max_line_segments_};
                uint32_t n = 0;     // this view's own segment count, set by the call that added it
                const int rc = (neighbors_by_worldpoints_ ? l3d_add_view_image_worldpoints : l3d_add_view_image)(
                    ctx_, camID, &im, &o, k, r, tt, median_depth, nb.data(), (uint32_t)nb.size(), &n);
                if (rc == L3D_ERR_NO_SEGMENTS)
                    std::cout << "[L3D++] WARNING: no line segments found in image [" << camID << "]!" << std::endl;
                else if (rc != L3D_OK) std::cout << prefix_err_ << "view [" << camID << "]: " << l3d_last_error() << std::endl;
                else { std::lock_guard<std::mutex> lk(lines_mu_); num_lines_[camID] = n; }
                return;
            }
        }
        std::vector<float> segs(4 * line_segments.size());
        for (size_t i = 0; i < line_segments.size(); ++i)
            for (int j = 0; j < 4; ++j) segs[4 * i + j] = line_segments[i][j];
        const int rc = (neighbors_by_worldpoints_ ? l3d_add_view_worldpoints : l3d_add_view)(
            ctx_, camID, segs.data(), (uint32_t)line_segments.size(), k, r, tt, (uint32_t)image.cols, (uint32_t)image.rows,
            median_depth, nb.data(), (uint32_t)nb.size());
        if (rc != L3D_OK) std::cout << prefix_err_ << "view [" << camID << "]: " << l3d_last_error() << std::endl;
        else { std::lock_guard<std::mutex> lk(lines_mu_); num_lines_[camID] = (uint32_t)line_segments.size(); }
    }

    // (the third argument tells the two forms of undistortImage apart: a vector of coefficients or an L3D_CAM_* value)
    template <class T> using IfModel = typename std::enable_if<std::is_integral<T>::value || std::is_enum<T>::value>::type;
    template <class T> using IfNotModel = typename std::enable_if<!std::is_integral<T>::value && !std::is_enum<T>::value>::type;

    // static void Line3D::undistortImage(inImg, outImg, radial_coeffs, tangential_coeffs, K), line3D.h:110-122, on the GPU
    // (l3d_undistort_images).  InImage: cv::Mat, Image8U or ImageBuf8U (8-bit, 1 or 3 channels); OutImage:
    // cv::Mat or ImageBuf8U, made with outImg.create(rows, cols, inImg.type()) and written at outImg.step (it may be the
    // input itself).  Vec3 / Vec2: radial(i), tangential(i) (Eigen vectors); Mat3: K(r, c).  Errors are printed and leave
    // outImg empty.  Static like the reference's, so there is no instance context: one process-wide context on device 0,
    // made by the first call.  Calls from several threads (the front ends' OpenMP loops) run one after another on it.
    template <class InImage, class OutImage, class Vec3, class Vec2, class Mat3, class = IfNotModel<Vec3>>
    static void undistortImage(const InImage& inImg, OutImage& outImg, const Vec3& radial_coeffs,
                               const Vec2& tangential_coeffs, const Mat3& K) {
        const int ty = inImg.type();
        const uint32_t ch = ty == 0 ? 1u : ty == 16 ? 3u : 0u;
        const l3d_image in{(const uint8_t*)inImg.data, (uint32_t)inImg.cols, (uint32_t)inImg.rows, ch,
                           (uint32_t)(size_t)inImg.step};
        l3d_distortion d{};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) d.K[3 * r + c] = K(r, c);
        for (int i = 0; i < 3; ++i) d.radial[i] = radial_coeffs(i);
        for (int i = 0; i < 2; ++i) d.tangential[i] = tangential_coeffs(i);
        const size_t row = (size_t)in.cols * ch;
        std::vector<uint8_t> tmp;
        uint8_t* dst = nullptr;
        if (ch) {
            outImg.create(inImg.rows, inImg.cols, ty);
            if ((size_t)outImg.step == row) dst = (uint8_t*)outImg.data;
            else { tmp.resize(row * in.rows); dst = tmp.data(); }
        }
        l3d_ctx* ctx = undistort_context();
        const int rc = ctx ? l3d_undistort_images(ctx, 1, &in, &d, &dst) : L3D_ERR_HIP;
        if (rc != L3D_OK) {
            std::cout << "[L3D++] ERROR: undistortImage: "
                      << (ctx ? l3d_last_error() : "no HIP context on device 0") << std::endl;
            outImg.release();
            return;
        }
        if (!tmp.empty())
            for (uint32_t r = 0; r < in.rows; ++r)
                std::memcpy((uint8_t*)outImg.data + r * (size_t)outImg.step, tmp.data() + r * row, row);
    }

    // undistortImage by camera model (l3d_undistort_images_model) for COLMAP's models beyond the reference's
    // five coefficients: model = L3D_CAM_FULL_OPENCV, _OPENCV_FISHEYE, _SIMPLE_RADIAL_FISHEYE, _RADIAL_FISHEYE or _FOV;
    // params: the model's distortion parameters in COLMAP's order (std::vector<double>, an initializer list, anything
    // with begin() / end(); at most 8, missing ones are 0); K: the camera matrix of inImg; K_new: that of outImg (left
    // out: K).  Images, errors, threads and the context are those of the overload above.
    template <class InImage, class OutImage, class Model, class Params, class Mat3, class = IfModel<Model>>
    static void undistortImage(const InImage& inImg, OutImage& outImg, Model model, const Params& params, const Mat3& K,
                               const Mat3& K_new) {
        undistort_model(inImg, outImg, (uint32_t)model, params, K, &K_new);
    }
    template <class InImage, class OutImage, class Model, class Params, class Mat3, class = IfModel<Model>>
    static void undistortImage(const InImage& inImg, OutImage& outImg, Model model, const Params& params, const Mat3& K) {
        undistort_model(inImg, outImg, (uint32_t)model, params, K, (const Mat3*)nullptr);
    }
    template <class InImage, class OutImage, class Model, class Mat3, class = IfModel<Model>>
    static void undistortImage(const InImage& inImg, OutImage& outImg, Model model, std::initializer_list<double> params,
                               const Mat3& K, const Mat3& K_new) {
        undistort_model(inImg, outImg, (uint32_t)model, params, K, &K_new);
    }
    template <class InImage, class OutImage, class Model, class Mat3, class = IfModel<Model>>
    static void undistortImage(const InImage& inImg, OutImage& outImg, Model model, std::initializer_list<double> params,
                               const Mat3& K) {
        undistort_model(inImg, outImg, (uint32_t)model, params, K, (const Mat3*)nullptr);
    }

    // static Eigen::Matrix3d Line3D::rotationFromRPY(roll, pitch, yaw) and rotationFromQ(Qw, Qx, Qy, Qz), line3D.h:220-226
    // (line3D.cc:2714-2754).  Mat3: the matrix type to return, default-constructible with R(r, c) (Eigen::Matrix3d):
    // Line3D::rotationFromRPY<Eigen::Matrix3d>(r, p, y)
    template <class Mat3>
    static Mat3 rotationFromRPY(const double roll, const double pitch, const double yaw) {
        double r[9];
        l3d_rotation_from_rpy(roll, pitch, yaw, r);
        Mat3 R;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R(i, j) = r[3 * i + j];
        return R;
    }
    template <class Mat3>
    static Mat3 rotationFromQ(const double Qw, const double Qx, const double Qy, const double Qz) {
        double r[9];
        l3d_rotation_from_q(Qw, Qx, Qy, Qz, r);
        Mat3 R;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R(i, j) = r[3 * i + j];
        return R;
    }

    // static void Line3D::decomposeProjectionMatrix(P_in, K_out, R_out, t_out), line3D.h:228-232 (line3D.cc:2784-2853):
    // P = K [R | t].  MatP: anything with (r, c), rows() and cols() (Eigen::MatrixXd); a P that is neither 3 rows nor 4
    // columns is reported and leaves the outputs alone, the reference's own test (:2789)
    template <class MatP, class Mat3, class Vec3>
    static void decomposeProjectionMatrix(const MatP& P_in, Mat3& K_out, Mat3& R_out, Vec3& t_out) {
        if (P_in.rows() != 3 && P_in.cols() != 4) {
            std::cout << "P is not a 3x4 matrix! (" << P_in.rows() << "x" << P_in.cols() << ")" << std::endl;
            return;
        }
        double p[12], k[9], r[9], t[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) p[4 * i + j] = P_in(i, j);
        l3d_decompose_projection_matrix(p, k, r, t);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { K_out(i, j) = k[3 * i + j]; R_out(i, j) = r[3 * i + j]; }
            t_out(i) = t[i];
        }
    }

    // void Line3D::matchImages(...), line3D.h:143-148
    void matchImages(const float sigma_position = L3D_DEF_SCORING_POS_REGULARIZER,
                     const float sigma_angle = L3D_DEF_SCORING_ANG_REGULARIZER,
                     const unsigned int num_neighbors = L3D_DEF_MATCHING_NEIGHBORS,
                     const float epipolar_overlap = L3D_DEF_EPIPOLAR_OVERLAP, const int kNN = L3D_DEF_KNN,
                     const float const_regularization_depth = -1.0f) {
        std::cout << std::endl << prefix_ << "[2] LINE MATCHING ================================" << std::endl;
        l3d_match_params p{sigma_position, sigma_angle, num_neighbors, epipolar_overlap, kNN, const_regularization_depth};
        const int rc = l3d_match_images(ctx_, &p);
        if (rc != L3D_OK) std::cout << prefix_err_ << l3d_last_error() << std::endl;
    }

    // the affinity part of void Line3D::reconstruct3Dlines(...), line3D.cc:1749-1778
    void computeAffinityMatrix() {
        const int rc = l3d_compute_affinity(ctx_);
        if (rc != L3D_OK) std::cout << prefix_err_ << l3d_last_error() << std::endl;
    }

    // void Line3D::reconstruct3Dlines(...), line3D.h:162-166: affinity matrix, graph clustering, 3D line per
    // cluster, collinear 3D segments; perform_diffusion runs the replicator-dynamics diffusion (performRDD) on the
    // GPU like a CUDA build of the reference; use_CERES bundles the 3D lines (optimizeClusters) on the GPU, one
    // Levenberg-Marquardt solve per line of the reference's cost (include/l3dpp_hip.h).  use_CERES defaults to false
    // as in a reference build without Ceres (a build with Ceres defaults to true, commons.h:84)
    void reconstruct3Dlines(const unsigned int visibility_t = 3, const bool perform_diffusion = false,
                            const float collinearity_t = -1.0f, const bool use_CERES = false,
                            const unsigned int max_iter_CERES = 250) {
        std::cout << std::endl << prefix_ << "[3] RECONSTRUCTION ===============================" << std::endl;
        const int rc = l3d_reconstruct_3d_lines(ctx_, visibility_t, perform_diffusion, collinearity_t, use_CERES, max_iter_CERES);
        if (rc != L3D_OK) { std::cout << prefix_err_ << l3d_last_error() << std::endl; return; }
        if (use_CERES) {   // optimization.cc:190
            l3d_line_opt_summary st{};
            l3d_line_opt_stats(ctx_, &st);
            std::cout << prefix_ << "#unoptimizable_lines = " << st.lines_constant << std::endl;
        }
    }

    // void Line3D::get3Dlines(std::vector<FinalLine3D>&), line3D.h:173.  FinalLine3D / LineCluster3D with the reference's member
    // and accessor names (segment3D.h:120-178), so that a consumer written against them compiles unchanged:
    // line.underlyingCluster_.seg3D(), .residuals(), .size(), .reference_view(); the 3D segments and 2D segment ids are the
    // C-ABI's PODs (reference layouts: l3d_segment3d = Segment3D's P1, P2, dir; l3d_segment2d = camID, segID)
    class LineCluster3D {
    public:
        LineCluster3D() : reference_view_(0) {}
        LineCluster3D(const l3d_segment3d& seg3D, const std::list<l3d_segment2d>& residuals, const unsigned int ref_view)
            : seg3D_(seg3D), residuals_(residuals), reference_view_(ref_view) {}
        l3d_segment3d seg3D() const { return seg3D_; }
        const std::list<l3d_segment2d>* residuals() const { return &residuals_; }
        size_t size() const { return residuals_.size(); }
        unsigned int reference_view() const { return reference_view_; }
        void update3Dline(const l3d_segment3d& seg3D) { seg3D_ = seg3D; }
    private:
        l3d_segment3d seg3D_{};
        std::list<l3d_segment2d> residuals_;
        unsigned int reference_view_;
    };
    struct FinalLine3D {
        std::list<l3d_segment3d> collinear3Dsegments_;
        LineCluster3D underlyingCluster_;
    };
    void get3Dlines(std::vector<FinalLine3D>& result) {
        result.clear();
        uint32_t nl = 0, ns = 0, nr = 0;
        if (l3d_num_3d_lines(ctx_, &nl, &ns, &nr) != L3D_OK) return;
        std::vector<uint32_t> so(nl + 1), ro(nl + 1), rv(nl);
        std::vector<l3d_segment3d> segs(ns), cl(nl);
        std::vector<l3d_segment2d> res(nr);
        l3d_get_3d_lines(ctx_, so.data(), segs.data(), ro.data(), res.data(), cl.data(), rv.data());
        result.resize(nl);
        for (uint32_t i = 0; i < nl; ++i) {
            result[i].collinear3Dsegments_.assign(segs.begin() + so[i], segs.begin() + so[i + 1]);
            result[i].underlyingCluster_ = LineCluster3D(cl[i], std::list<l3d_segment2d>(res.begin() + ro[i], res.begin() + ro[i + 1]), rv[i]);
        }
    }

    // void Line3D::save3DLinesAsTXT(const std::string& output_folder), line3D.h:176
    void save3DLinesAsTXT(const std::string& output_folder) {
        if (l3d_save_3d_lines_txt(ctx_, output_folder.c_str(), max_img_width_) != L3D_OK)
            std::cout << prefix_ << "WARNING: " << l3d_last_error() << std::endl;
    }

    // void Line3D::save3DLinesAsBIN(const std::string& output_folder), line3D.h:185
    void save3DLinesAsBIN(const std::string& output_folder) {
        if (l3d_save_3d_lines_bin(ctx_, output_folder.c_str(), max_img_width_) != L3D_OK)
            std::cout << prefix_ << "WARNING: " << l3d_last_error() << std::endl;
    }

    // std::string Line3D::createOutputFilename(), line3D.h:226
    std::string createOutputFilename() {
        char buf[512];
        return l3d_output_filename(ctx_, max_img_width_, buf, sizeof(buf)) == L3D_OK ? std::string(buf) : std::string();
    }
    // getSegmentCoords2D(camID, segID), line3D.h:195-197: (x1, y1, x2, y2)
    struct Coords2D { float v[4]; float operator()(int i) const { return v[i]; } };
    Coords2D getSegmentCoords2D(const unsigned int camID, const unsigned int segID) {
        Coords2D c{};
        l3d_get_segment_coords2d(ctx_, camID, segID, c.v);
        return c;
    }

    // saveResultAsSTL / saveResultAsOBJ, line3D.h:174-175
    void saveResultAsSTL(const std::string& output_folder) {
        if (l3d_save_result_stl(ctx_, output_folder.c_str(), max_img_width_) != L3D_OK)
            std::cout << prefix_ << "WARNING: " << l3d_last_error() << std::endl;
    }
    void saveResultAsOBJ(const std::string& output_folder) {
        if (l3d_save_result_obj(ctx_, output_folder.c_str(), max_img_width_) != L3D_OK)
            std::cout << prefix_ << "WARNING: " << l3d_last_error() << std::endl;
    }

    size_t numImages() const { std::lock_guard<std::mutex> lk(lines_mu_); return num_lines_.size(); }

    // matches_[camID] rebuilt in the reference's container type (line3D.h:348)
    std::vector<std::list<l3d_match>> matches(const unsigned int camID) {
        std::vector<std::list<l3d_match>> out;
        uint32_t M = 0;
        {
            std::lock_guard<std::mutex> lk(lines_mu_);
            auto f = num_lines_.find(camID);
            if (f == num_lines_.end()) return out;
            M = f->second;
        }
        uint64_t n = 0;
        std::vector<uint32_t> off(M + 1);
        if (l3d_get_matches(ctx_, camID, nullptr, 0, off.data(), &n) != L3D_OK) return out;
        std::vector<l3d_match> flat(n);
        if (n) l3d_get_matches(ctx_, camID, flat.data(), n, off.data(), &n);
        out.resize(M);
        for (uint32_t s = 0; s < M; ++s) out[s].assign(flat.begin() + off[s], flat.begin() + off[s + 1]);
        return out;
    }

    // estimated_position3D_ + entry_map_ (line3D.h:352-356): (Segment2D, Segment3D members, best Match)
    struct Hypothesis { l3d_segment2d seg2D; l3d_segment3d seg3D; l3d_match match; };
    std::vector<Hypothesis> estimatedPosition3D() {
        uint32_t n = 0;
        l3d_num_best(ctx_, &n);
        std::vector<l3d_segment2d> a(n); std::vector<l3d_segment3d> b(n); std::vector<l3d_match> m(n);
        std::vector<Hypothesis> out(n);
        if (n && l3d_get_best(ctx_, a.data(), b.data(), m.data()) == L3D_OK)
            for (uint32_t i = 0; i < n; ++i) out[i] = Hypothesis{a[i], b[i], m[i]};
        return out;
    }

    // A_ (std::list<CLEdge>), local2global_, as clusterSegments() consumes them (line3D.cc:2079-2090)
    void affinity(std::list<l3d_cledge>& A, std::map<int, l3d_segment2d>& local2global) {
        A.clear(); local2global.clear();
        uint32_t ne = 0, nr = 0;
        if (l3d_num_affinity(ctx_, &ne, &nr) != L3D_OK) return;
        std::vector<l3d_cledge> e(ne); std::vector<l3d_segment2d> l(nr);
        float msdl = 0;
        l3d_get_affinity(ctx_, e.data(), l.data(), &msdl);
        A.assign(e.begin(), e.end());
        for (uint32_t i = 0; i < nr; ++i) local2global[(int)i] = l[i];
    }

    // The 3D lines of the last reconstruct3Dlines as a camera sees them (no reference counterpart; DESIGN §16,
    // k_project.hip): one l3d_projected_segment per visible 3D segment, clipped at the near plane and at the image, in
    // ascending segment order.  The camera is an added view (camID) or any K, R, t with an image size.  Errors are
    // printed and leave `out` empty.
    template <class Mat3, class Vec3>
    void projectLines(const Mat3& K, const Mat3& R, const Vec3& t, const unsigned int width, const unsigned int height,
                      std::vector<l3d_projected_segment>& out, const double near_plane = 1e-6) {
        project_camera(make_camera(K, R, t, width, height), out, near_plane);
    }
    void projectLines(const unsigned int camID, std::vector<l3d_projected_segment>& out, const double near_plane = 1e-6) {
        out.clear();
        l3d_camera cam{};
        if (l3d_view_camera(ctx_, camID, &cam) != L3D_OK) {
            std::cout << prefix_err_ << "projectLines [" << camID << "]: " << l3d_last_error() << std::endl;
            return;
        }
        project_camera(cam, out, near_plane);
    }

    // The 2D segments that support each 3D line (no reference counterpart; DESIGN §17, k_associate.hip): every segment of
    // the added view camID is assigned the 3D line of the last reconstruct3Dlines it observes -- out[segID].record is the
    // index among the view's projected records (projectLines(camID, ...)), -1 where the segment observes none; .line the
    // 3D line.  max_distance in pixels, max_angle in degrees [0, 90], min_overlap = the share of the 2D segment that has
    // to lie within the projected 3D segment.  Errors are printed and leave `out` empty.
    void associateSegments(const unsigned int camID, std::vector<l3d_association>& out, const double max_distance = 2.5,
                           const double max_angle = 10.0, const double min_overlap = 0.5, const double near_plane = 1e-6) {
        std::map<unsigned int, std::vector<l3d_association>> all;
        associate_views(std::vector<uint32_t>(1, camID), all, max_distance, max_angle, min_overlap, near_plane);
        out.clear();
        if (!all.empty()) out.swap(all.begin()->second);
    }
    // ... of every added view: out[camID][segID]
    void associateSegments(std::map<unsigned int, std::vector<l3d_association>>& out, const double max_distance = 2.5,
                           const double max_angle = 10.0, const double min_overlap = 0.5, const double near_plane = 1e-6) {
        std::vector<uint32_t> ids;
        {
            std::lock_guard<std::mutex> lk(lines_mu_);
            for (const auto& kv : num_lines_) ids.push_back(kv.first);
        }
        associate_views(ids, out, max_distance, max_angle, min_overlap, near_plane);
    }

    // This model compared with another one (no reference counterpart; DESIGN §18, k_compare.hip): `other` as get3Dlines
    // hands a model out, in the same frame.  mine[k]: the counterpart in `other` of this model's k-th flat segment (the
    // collinear3Dsegments_ of get3Dlines, line after line); theirs[k]: the counterpart in this model of other's k-th.
    // .segment is the index among the flat segments of the opposite side (-1: none), .line the index of its line.
    // max_distance in model units -- a 3D model has no natural unit, so there is no default --, max_angle in degrees
    // [0, 90], min_overlap = the share of a segment inside its counterpart's extent.  Errors are printed and leave both
    // outputs empty.
    void compareLines(const std::vector<FinalLine3D>& other, std::vector<l3d_line_match>& mine, std::vector<l3d_line_match>& theirs,
                      const double max_distance, const double max_angle = 10.0, const double min_overlap = 0.5) {
        mine.clear();
        theirs.clear();
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "compareLines: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_compare_params par{max_distance, cosine * cosine, min_overlap, 0u, 0u};
        std::vector<double> segs;
        std::vector<uint32_t> line;
        for (size_t i = 0; i < other.size(); ++i)
            for (const l3d_segment3d& s : other[i].collinear3Dsegments_) {
                segs.insert(segs.end(), s.P1, s.P1 + 3);
                segs.insert(segs.end(), s.P2, s.P2 + 3);
                line.push_back((uint32_t)i);
            }
        uint32_t ns = 0;
        if (l3d_num_3d_lines(ctx_, nullptr, &ns, nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "compareLines: " << l3d_last_error() << std::endl;
            return;
        }
        std::vector<l3d_line_match> a(ns ? ns : 1), b(line.empty() ? 1 : line.size());
        if (l3d_compare_lines(ctx_, (uint32_t)line.size(), segs.data(), line.data(), &par, a.data(), b.data(), nullptr, nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "compareLines: " << l3d_last_error() << std::endl;
            return;
        }
        a.resize(ns);
        b.resize(line.size());
        mine.swap(a);
        theirs.swap(b);
    }

    // This model aligned to another one (no reference counterpart; DESIGN §23, k_align.hip): the similarity transform
    // y = scale * R(q) x + t that moves the lines of the last reconstruct3Dlines onto `other`, a model of the same scene
    // in another frame, by iterated closest lines from `initial` (null: identity); the gate of a match halves from
    // start_distance (0: none) down to max_distance, both in the units of `other`.  similarity and summary receive the
    // result; moved (may be null): this model's flat segments under the transform, 6 doubles each; mine / theirs (may be
    // null): the comparison of the aligned models at max_distance, as compareLines returns it.  The model itself is NOT
    // changed.  Errors are printed and leave every output as it was.
    void alignLines(const std::vector<FinalLine3D>& other, l3d_similarity& similarity, l3d_align_summary& summary,
                    const double max_distance, const double start_distance = 0.0, const l3d_similarity* initial = nullptr,
                    const bool estimate_scale = true, const double max_angle = 10.0, const double min_overlap = 0.5,
                    std::vector<double>* moved = nullptr, std::vector<l3d_line_match>* mine = nullptr,
                    std::vector<l3d_line_match>* theirs = nullptr) {
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "alignLines: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_align_params par{max_distance, cosine * cosine, min_overlap, start_distance, 1e-9, 50u, 8u, estimate_scale ? 1u : 0u, 0u, {0u, 0u}};
        std::vector<double> segs;
        std::vector<uint32_t> line;
        for (size_t i = 0; i < other.size(); ++i)
            for (const l3d_segment3d& s : other[i].collinear3Dsegments_) {
                segs.insert(segs.end(), s.P1, s.P1 + 3);
                segs.insert(segs.end(), s.P2, s.P2 + 3);
                line.push_back((uint32_t)i);
            }
        uint32_t ns = 0;
        if (l3d_num_3d_lines(ctx_, nullptr, &ns, nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "alignLines: " << l3d_last_error() << std::endl;
            return;
        }
        std::vector<double> m(6 * (size_t)(ns ? ns : 1));
        std::vector<l3d_line_match> a(ns ? ns : 1), b(line.empty() ? 1 : line.size());
        l3d_similarity sim;
        l3d_align_summary sum;
        if (l3d_align_lines(ctx_, (uint32_t)line.size(), segs.data(), line.data(), &par, initial, &sim, &sum, m.data(), a.data(),
                            b.data(), nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "alignLines: " << l3d_last_error() << std::endl;
            return;
        }
        similarity = sim;
        summary = sum;
        m.resize(6 * (size_t)ns);
        a.resize(ns);
        b.resize(line.size());
        if (moved) moved->swap(m);
        if (mine) mine->swap(a);
        if (theirs) theirs->swap(b);
    }

    // The views' cameras refined against this model (no reference counterpart; DESIGN §27, k_pose.hip): the pose of every
    // added view (or of the views camIDs) is refined against the lines of the last reconstruct3Dlines from the view's own
    // segments, by iterated closest lines; the gate of a match halves from start_distance (0: none) down to max_distance,
    // both in pixels, whenever the step stalls.  cameras[camID] receives the refined l3d_camera (K unchanged),
    // summaries[camID] its l3d_pose_summary; associations (may be null): [camID][segID], what associateSegments would
    // return for the refined camera.  Neither the views nor the model are changed.  Errors are printed and leave every
    // output as it was.
    void refineCameras(std::map<unsigned int, l3d_camera>& cameras, std::map<unsigned int, l3d_pose_summary>& summaries,
                       const double max_distance = 2.5, const double start_distance = 0.0, const double max_angle = 10.0,
                       const double min_overlap = 0.5, const std::vector<unsigned int>* camIDs = nullptr,
                       std::map<unsigned int, std::vector<l3d_association>>* associations = nullptr, const double near_plane = 1e-6) {
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "refineCameras: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_pose_params par{max_distance, cosine * cosine, min_overlap, start_distance, 1e-4, 1e-9, near_plane, 50u, 8u, {0u, 0u}};
        std::vector<uint32_t> ids;
        if (camIDs) ids.assign(camIDs->begin(), camIDs->end());
        else {
            std::lock_guard<std::mutex> lk(lines_mu_);
            for (const auto& kv : num_lines_) ids.push_back(kv.first);
        }
        uint64_t room = 0;
        {
            std::lock_guard<std::mutex> lk(lines_mu_);
            for (uint32_t id : ids) {
                const auto f = num_lines_.find(id);
                if (f != num_lines_.end()) room += f->second;
            }
        }
        std::vector<l3d_camera> cams(ids.size() + 1);
        std::vector<l3d_pose_summary> sums(ids.size() + 1);
        std::vector<uint64_t> off(ids.size() + 1, 0);
        std::vector<l3d_association> assoc((size_t)room + 1);
        if (l3d_refine_view_cameras(ctx_, (uint32_t)ids.size(), ids.data(), &par, cams.data(), sums.data(), off.data(), assoc.data(),
                                    nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "refineCameras: " << l3d_last_error() << std::endl;
            return;
        }
        for (size_t k = 0; k < ids.size(); ++k) {
            cameras[ids[k]] = cams[k];
            summaries[ids[k]] = sums[k];
            if (associations) (*associations)[ids[k]].assign(assoc.begin() + (size_t)off[k], assoc.begin() + (size_t)off[k + 1]);
        }
    }

    // This model refit against the views (no reference counterpart; DESIGN §28, k_refit.hip): every line of the last
    // reconstruct3Dlines is re-estimated from the 2D segments of the added views (or of the views camIDs) that observe it
    // within max_distance pixels -- in `cameras` (by camID; null or a missing camID: the view's own, e.g. what
    // refineCameras returned) -- by the solver of the line bundling, and cut anew where at least `visibility` views see
    // it.  The refit model takes the place of lines3D_, as mergeLines' does; a line that cannot be refit stays as it is.
    // Saved files carry REFIT_<max_distance>__ in their name until the next reconstruct3Dlines.  summary (may be null):
    // the counts of the refit.  Errors are printed and leave the model as it was.
    void refitLines(const std::map<unsigned int, l3d_camera>* cameras = nullptr, const double max_distance = 2.5,
                    const double max_angle = 10.0, const double min_overlap = 0.5, const unsigned int visibility = 3,
                    const unsigned int max_iterations = 50, const bool use_ambiguous = false, const double min_length = 0.0,
                    const std::vector<unsigned int>* camIDs = nullptr, l3d_refit_summary* summary = nullptr,
                    const double near_plane = 1e-6) {
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "refitLines: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_refit_params par{max_distance, cosine * cosine, min_overlap, near_plane, min_length, visibility, max_iterations,
                                   use_ambiguous ? 1u : 0u, {0u, 0u, 0u}};
        std::vector<uint32_t> ids;
        if (camIDs) ids.assign(camIDs->begin(), camIDs->end());
        else {
            std::lock_guard<std::mutex> lk(lines_mu_);
            for (const auto& kv : num_lines_) ids.push_back(kv.first);
        }
        std::vector<l3d_camera> cams(ids.size() + 1);
        for (size_t k = 0; k < ids.size(); ++k) {
            if (cameras) {
                const auto f = cameras->find(ids[k]);
                if (f != cameras->end()) { cams[k] = f->second; continue; }
            }
            if (l3d_view_camera(ctx_, ids[k], &cams[k]) != L3D_OK) {
                std::cout << prefix_err_ << "refitLines: " << l3d_last_error() << std::endl;
                return;
            }
        }
        if (l3d_refit_view_lines(ctx_, (uint32_t)ids.size(), ids.data(), cams.data(), &par, summary, nullptr) != L3D_OK)
            std::cout << prefix_err_ << "refitLines: " << l3d_last_error() << std::endl;
    }

    // This model and the views' cameras bundled jointly (no reference counterpart; DESIGN §29, k_bundle.hip): one
    // association of the lines of the last reconstruct3Dlines with the 2D segments of the added views (or of the views
    // camIDs) within max_distance pixels, in `cameras` (by camID; null or a missing camID: the view's own), then
    // Levenberg-Marquardt jointly over the poses of the cameras that are not in `fixed` and the lines that at least
    // max(2, visibility) views see, and the lines cut anew.  The bundled model takes the place of lines3D_, as refitLines'
    // does; saved files carry BUNDLE_<max_distance>__ in their name until the next reconstruct3Dlines.  The new cameras are
    // written into `cameras` where it is given (every camID of the call); the views keep theirs.  summary (may be null): the
    // counts of the call.  Errors are printed and leave the model and `cameras` as they were.
    void bundleModel(std::map<unsigned int, l3d_camera>* cameras = nullptr, const double max_distance = 2.5,
                     const double max_angle = 10.0, const double min_overlap = 0.5, const unsigned int visibility = 3,
                     const unsigned int max_iterations = 10, const bool use_ambiguous = false, const double min_length = 0.0,
                     const std::vector<unsigned int>* camIDs = nullptr, const std::vector<unsigned int>* fixed = nullptr,
                     l3d_bundle_summary* summary = nullptr, const double near_plane = 1e-6) {
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "bundleModel: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_bundle_params par{max_distance, cosine * cosine, min_overlap, near_plane, min_length, 1e-4, 1e-9, 1e8, 1e-6,
                                    visibility, max_iterations, use_ambiguous ? 1u : 0u, 0u, {0u, 0u, 0u, 0u}};
        std::vector<uint32_t> ids;
        if (camIDs) ids.assign(camIDs->begin(), camIDs->end());
        else {
            std::lock_guard<std::mutex> lk(lines_mu_);
            for (const auto& kv : num_lines_) ids.push_back(kv.first);
        }
        std::vector<l3d_camera> cams(ids.size() + 1);
        std::vector<uint8_t> fix(ids.size() + 1, 0);
        for (size_t k = 0; k < ids.size(); ++k) {
            if (fixed)
                for (const unsigned int id : *fixed)
                    if (id == ids[k]) fix[k] = 1;
            if (cameras) {
                const auto f = cameras->find(ids[k]);
                if (f != cameras->end()) { cams[k] = f->second; continue; }
            }
            if (l3d_view_camera(ctx_, ids[k], &cams[k]) != L3D_OK) {
                std::cout << prefix_err_ << "bundleModel: " << l3d_last_error() << std::endl;
                return;
            }
        }
        l3d_bundle* h = nullptr;
        if (l3d_bundle_view_lines(ctx_, (uint32_t)ids.size(), ids.data(), cams.data(), fix.data(), &par, summary, &h) != L3D_OK) {
            std::cout << prefix_err_ << "bundleModel: " << l3d_last_error() << std::endl;
            return;
        }
        if (cameras) {
            l3d_bundle_get(h, nullptr, nullptr, nullptr, nullptr, nullptr, cams.data(), nullptr, nullptr, nullptr, nullptr);
            for (size_t k = 0; k < ids.size(); ++k) (*cameras)[ids[k]] = cams[k];
        }
        l3d_bundle_close(h);
    }

    // The near-duplicate lines of this model merged (no reference counterpart; DESIGN §19, k_merge.hip): lines joined by
    // accepted pairs of segments -- compareLines' pair test, between different lines -- become one line, and the merged
    // model takes the place of lines3D_: get3Dlines, the writers, projectLines, associateSegments and compareLines see
    // it; saved files carry MERGED_<max_distance>__ in their name until the next reconstruct3Dlines.  max_distance in
    // model units, max_angle in degrees [0, 90], min_overlap = the share of a segment inside its counterpart's extent.
    // summary (may be null): the counts of the merge.  Errors are printed and leave the model as it was.
    void mergeLines(const double max_distance, const double max_angle = 10.0, const double min_overlap = 0.5,
                    l3d_merge_summary* summary = nullptr) {
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "mergeLines: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_merge_params par{max_distance, cosine * cosine, min_overlap, 0u, 0u};
        if (l3d_merge_lines(ctx_, &par, summary) != L3D_OK) std::cout << prefix_err_ << "mergeLines: " << l3d_last_error() << std::endl;
    }

    // Where the lines of this model meet (no reference counterpart; DESIGN §24, k_wireframe.hip): two segments of
    // different lines whose carriers come within max_distance of each other, at an angle of at least min_angle, at a
    // point on both or at most max_extension beyond an end, form a junction; the junctions and the ends that meet nothing
    // are the vertices, the pieces of the segments between them the edges.  Segments are the flat collinear3Dsegments_ of
    // get3Dlines, line after line.  max_distance and max_extension (negative: max_distance) in model units, min_angle in
    // degrees [0, 90].  The model itself is NOT changed.  Errors are printed and give an empty result with ok = false.
    struct Wireframe {
        bool ok = false;
        std::vector<l3d_wf_junction> junctions;
        std::vector<l3d_wf_vertex> vertices;
        std::vector<l3d_wf_edge> edges;
        l3d_wireframe_summary summary{};
    };
    Wireframe wireframe(const double max_distance, const double max_extension = -1.0, const double min_angle = 10.0) {
        Wireframe w;
        if (!(min_angle >= 0.0 && min_angle <= 90.0)) {
            std::cout << prefix_err_ << "wireframe: min_angle must lie in [0, 90] degrees" << std::endl;
            return w;
        }
        const double sine = std::sin(min_angle * (3.14159265358979323846 / 180.0));
        const l3d_wireframe_params par{max_distance, max_extension < 0.0 ? max_distance : max_extension, sine * sine, 0u, 0u};
        l3d_wireframe* h = nullptr;
        if (l3d_wireframe_lines(ctx_, &par, &h) != L3D_OK) {
            std::cout << prefix_err_ << "wireframe: " << l3d_last_error() << std::endl;
            return w;
        }
        uint64_t nj = 0, nv = 0, ne = 0;
        l3d_wireframe_counts(h, &nj, &nv, &ne);
        w.junctions.resize(nj); w.vertices.resize(nv); w.edges.resize(ne);
        l3d_wireframe_get(h, w.junctions.data(), w.vertices.data(), w.edges.data(), &w.summary);
        l3d_wireframe_close(h);
        w.ok = true;
        return w;
    }

    // The planes the lines of this model lie in (no reference counterpart; DESIGN §25, k_planes.hip): every pair of lines
    // that meet (as for wireframe, with junction_distance and junction_extension) spans a plane; a segment belongs to it
    // when both its end points lie within max_distance of it; the best-supported planes with at least min_segments members
    // of at least min_length in all are kept.  A segment may lie in several planes.  Distances in model units (negative
    // junction_distance / junction_extension: max_distance), min_angle in degrees [0, 90].  The model itself is NOT
    // changed.  Errors are printed and give an empty result with ok = false.
    struct Planes {
        bool ok = false;
        std::vector<l3d_pl_plane> planes;
        std::vector<l3d_pl_member> members;       // (plane, segment), in that order
        std::vector<uint32_t> seg_planes;         // per segment: the number of its planes
        std::vector<l3d_pl_score> scores;         // per hypothesis
        l3d_planes_summary summary{};
    };
    Planes detectPlanes(const double max_distance, const double junction_distance = -1.0, const double junction_extension = -1.0,
                        const double min_angle = 10.0, const double min_length = 0.0, const unsigned int min_segments = 4,
                        const unsigned int max_planes = 64, const unsigned int max_tests = 4096) {
        Planes p;
        if (!(min_angle >= 0.0 && min_angle <= 90.0)) {
            std::cout << prefix_err_ << "detectPlanes: min_angle must lie in [0, 90] degrees" << std::endl;
            return p;
        }
        const double sine = std::sin(min_angle * (3.14159265358979323846 / 180.0));
        const l3d_planes_params par{max_distance, junction_distance < 0.0 ? max_distance : junction_distance,
                                    junction_extension < 0.0 ? max_distance : junction_extension, sine * sine, min_length,
                                    min_segments, max_planes, max_tests, 0u, {0u, 0u}};
        l3d_planes* h = nullptr;
        if (l3d_plane_lines(ctx_, &par, &h) != L3D_OK) {
            std::cout << prefix_err_ << "detectPlanes: " << l3d_last_error() << std::endl;
            return p;
        }
        uint64_t np = 0, nm = 0, nh = 0;
        l3d_planes_counts(h, &np, &nm, &nh);
        l3d_planes_get(h, nullptr, nullptr, nullptr, nullptr, &p.summary);
        p.planes.resize(np); p.members.resize(nm); p.seg_planes.resize(p.summary.n_segments); p.scores.resize(nh);
        l3d_planes_get(h, p.planes.data(), p.members.data(), p.seg_planes.data(), p.scores.data(), nullptr);
        l3d_planes_close(h);
        p.ok = true;
        return p;
    }

    // The directions the lines of this model run in (no reference counterpart; DESIGN §26, k_directions.hip): the direction of
    // every segment is a hypothesis; a segment belongs to it when the angle between them is at most max_angle, either way
    // round; the best-supported directions with at least min_segments members of at least min_length in all are kept.  A
    // segment may belong to several.  summary.R is the rotation (row-major, p' = R p) that turns the heaviest directions
    // that are orthogonal within frame_angle into the coordinate axes.  Angles in degrees [0, 90].  The model itself is
    // NOT changed.  Errors are printed and give an empty result with ok = false.
    struct Directions {
        bool ok = false;
        std::vector<l3d_dir_direction> directions;
        std::vector<l3d_dir_member> members;      // (direction, segment), in that order
        std::vector<uint32_t> seg_directions;     // per segment: the number of its directions
        std::vector<l3d_dir_score> scores;        // per hypothesis = per segment
        l3d_directions_summary summary{};
    };
    Directions detectDirections(const double max_angle, const double min_length = 0.0, const unsigned int min_segments = 4,
                                const unsigned int max_directions = 16, const unsigned int max_tests = 4096,
                                const double frame_angle = 5.0) {
        Directions d;
        if (!(max_angle >= 0.0 && max_angle <= 90.0) || !(frame_angle >= 0.0 && frame_angle <= 90.0)) {
            std::cout << prefix_err_ << "detectDirections: max_angle and frame_angle must lie in [0, 90] degrees" << std::endl;
            return d;
        }
        const double sine = std::sin(max_angle * (3.14159265358979323846 / 180.0));
        const double frame_sine = std::sin(frame_angle * (3.14159265358979323846 / 180.0));
        const l3d_directions_params par{sine * sine, min_length, frame_sine * frame_sine, min_segments, max_directions, max_tests,
                                        0u, 16u, {0u, 0u, 0u, 0u, 0u}};
        l3d_directions* h = nullptr;
        if (l3d_direction_lines(ctx_, &par, &h) != L3D_OK) {
            std::cout << prefix_err_ << "detectDirections: " << l3d_last_error() << std::endl;
            return d;
        }
        uint64_t nd = 0, nm = 0, nh = 0;
        l3d_directions_counts(h, &nd, &nm, &nh);
        l3d_directions_get(h, nullptr, nullptr, nullptr, nullptr, &d.summary);
        d.directions.resize(nd); d.members.resize(nm); d.seg_directions.resize(d.summary.n_segments); d.scores.resize(nh);
        l3d_directions_get(h, d.directions.data(), d.members.data(), d.seg_directions.data(), d.scores.data(), nullptr);
        l3d_directions_close(h);
        d.ok = true;
        return d;
    }

    // The 3D lines drawn over inImg (cv::Mat, Image8U or ImageBuf8U, 8-bit with 1 or 3 channels, of the camera's size):
    // outImg.create(rows, cols, 16) -- RGB -- as undistortImage makes its output; thickness in pixels (odd), alpha 0..255,
    // one colour per line from a fixed palette.  Errors are printed and leave outImg empty.
    template <class InImage, class OutImage>
    void drawLines(const unsigned int camID, const InImage& inImg, OutImage& outImg, const unsigned int thickness = 1,
                   const unsigned int alpha = 255) {
        l3d_camera cam{};
        if (l3d_view_camera(ctx_, camID, &cam) != L3D_OK) {
            std::cout << prefix_err_ << "drawLines [" << camID << "]: " << l3d_last_error() << std::endl;
            outImg.release();
            return;
        }
        draw_camera(cam, inImg, outImg, thickness, alpha);
    }
    template <class Mat3, class Vec3, class InImage, class OutImage>
    void drawLines(const Mat3& K, const Mat3& R, const Vec3& t, const InImage& inImg, OutImage& outImg,
                   const unsigned int thickness = 1, const unsigned int alpha = 255) {
        draw_camera(make_camera(K, R, t, (unsigned int)inImg.cols, (unsigned int)inImg.rows), inImg, outImg, thickness, alpha);
    }

    l3d_ctx* handle() { return ctx_; }

private:
    template <class Mat3, class Vec3>
    static l3d_camera make_camera(const Mat3& K, const Mat3& R, const Vec3& t, unsigned int width, unsigned int height) {
        l3d_camera cam{};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { cam.K[3 * i + j] = K(i, j); cam.R[3 * i + j] = R(i, j); }
            cam.t[i] = t(i);
        }
        cam.width = width; cam.height = height;
        return cam;
    }
    void project_camera(const l3d_camera& cam, std::vector<l3d_projected_segment>& out, double near_plane) {
        out.clear();
        uint32_t count = 0;
        uint64_t n = 0;
        if (l3d_project_lines(ctx_, 1, &cam, near_plane, &count) != L3D_OK) {
            std::cout << prefix_err_ << "projectLines: " << l3d_last_error() << std::endl;
            return;
        }
        out.resize(count);
        l3d_get_projected_lines(ctx_, out.data(), out.size(), &n);
    }
    void associate_views(const std::vector<uint32_t>& ids, std::map<unsigned int, std::vector<l3d_association>>& out,
                         double max_distance, double max_angle, double min_overlap, double near_plane) {
        out.clear();
        if (!(max_angle >= 0.0 && max_angle <= 90.0)) {
            std::cout << prefix_err_ << "associateSegments: max_angle must lie in [0, 90] degrees" << std::endl;
            return;
        }
        const double cosine = std::cos(max_angle * (3.14159265358979323846 / 180.0));
        const l3d_associate_params par{max_distance, cosine * cosine, min_overlap};
        std::vector<uint64_t> off(ids.size() + 1, 0);
        if (l3d_associate_view_segments(ctx_, (uint32_t)ids.size(), ids.data(), &par, near_plane, off.data(), nullptr, nullptr, nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "associateSegments: " << l3d_last_error() << std::endl;
            return;
        }
        std::vector<l3d_association> flat(off.back() ? off.back() : 1);
        if (l3d_associate_view_segments(ctx_, (uint32_t)ids.size(), ids.data(), &par, near_plane, off.data(), flat.data(), nullptr, nullptr) != L3D_OK) {
            std::cout << prefix_err_ << "associateSegments: " << l3d_last_error() << std::endl;
            return;
        }
        for (size_t k = 0; k < ids.size(); ++k) out[ids[k]].assign(flat.begin() + off[k], flat.begin() + off[k + 1]);
    }
    template <class InImage, class OutImage>
    void draw_camera(const l3d_camera& cam, const InImage& inImg, OutImage& outImg, unsigned int thickness, unsigned int alpha) {
        const int ty = inImg.type();
        const l3d_image in{(const uint8_t*)inImg.data, (uint32_t)inImg.cols, (uint32_t)inImg.rows, ty == 0 ? 1u : ty == 16 ? 3u : 0u,
                           (uint32_t)(size_t)inImg.step};
        const size_t row = 3 * (size_t)in.cols;
        std::vector<uint8_t> tmp(row * in.rows);      // (the input may be the output: composed here, copied when done)
        uint8_t* dst = tmp.data();
        if (l3d_draw_lines(ctx_, 1, &cam, &in, 1e-6, thickness, alpha, nullptr, &dst) != L3D_OK) {
            std::cout << prefix_err_ << "drawLines: " << l3d_last_error() << std::endl;
            outImg.release();
            return;
        }
        outImg.create((int)in.rows, (int)in.cols, 16);
        for (uint32_t r = 0; r < in.rows; ++r)
            std::memcpy((uint8_t*)outImg.data + r * (size_t)outImg.step, tmp.data() + r * row, row);
    }

    template <class InImage, class OutImage, class Params, class Mat3>
    static void undistort_model(const InImage& inImg, OutImage& outImg, uint32_t model, const Params& params, const Mat3& K,
                                const Mat3* K_new) {
        const int ty = inImg.type();
        const uint32_t ch = ty == 0 ? 1u : ty == 16 ? 3u : 0u;
        const l3d_image in{(const uint8_t*)inImg.data, (uint32_t)inImg.cols, (uint32_t)inImg.rows, ch,
                           (uint32_t)(size_t)inImg.step};
        l3d_camera_model m{};
        m.model = model;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                m.K[3 * r + c] = K(r, c);
                if (K_new) m.K_new[3 * r + c] = (*K_new)(r, c);
            }
        size_t n_params = 0;
        for (double v : params) {
            if (n_params < 8) m.params[n_params] = v;
            ++n_params;
        }
        const size_t row = (size_t)in.cols * ch;
        std::vector<uint8_t> tmp;
        uint8_t* dst = nullptr;
        if (ch) {
            outImg.create(inImg.rows, inImg.cols, ty);
            if ((size_t)outImg.step == row) dst = (uint8_t*)outImg.data;
            else { tmp.resize(row * in.rows); dst = tmp.data(); }
        }
        l3d_ctx* ctx = undistort_context();
        const int rc = n_params > 8 ? L3D_ERR_ARG : ctx ? l3d_undistort_images_model(ctx, 1, &in, &m, &dst) : L3D_ERR_HIP;
        if (rc != L3D_OK) {
            std::cout << "[L3D++] ERROR: undistortImage: "
                      << (n_params > 8 ? "more than 8 distortion parameters" : ctx ? l3d_last_error() : "no HIP context on device 0")
                      << std::endl;
            outImg.release();
            return;
        }
        if (!tmp.empty())
            for (uint32_t r = 0; r < in.rows; ++r)
                std::memcpy((uint8_t*)outImg.data + r * (size_t)outImg.step, tmp.data() + r * row, row);
    }

    // the context of the static undistortImage: made once, thread-safely, by the first call; it lives as long as the
    // process (destroying it from a static destructor could run after the HIP runtime's own teardown)
    static l3d_ctx* undistort_context() {
        static l3d_ctx* const ctx = l3d_create(0, nullptr);
        return ctx;
    }

    l3d_ctx* ctx_ = nullptr;
    std::string output_folder_;
    bool load_segments_ = true;
    int max_img_width_ = -1;
    unsigned int max_line_segments_ = 3000;
    bool neighbors_by_worldpoints_ = false;
    std::map<unsigned int, uint32_t> num_lines_;    // segments per added view (addImage may run on several threads)
    mutable std::mutex lines_mu_;
    std::string prefix_, prefix_err_;
};

}  // namespace L3DPP_HIP

#endif  // L3DPP_HIP_FACADE_LINE3D_H_
