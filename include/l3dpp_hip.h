/* =============================================================================
 * l3dpp_hip.h -- C-ABI of the MI355X-native Line3D++ matching/scoring hot path.
 *
 * Shared library: line3dpp_amd/csrc/libl3dpp_hip.so (hand-written HIP, gfx950).
 * Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository manhofer/Line3Dpp).  Two layers are exported:
 *
 *   (1) context layer  -- replaces the slice of class L3DPP::Line3D that drives the hot
 *       path: addImage (explicit segments) / matchImages / the affinity part of
 *       reconstruct3Dlines, with accessors that hand back matches_, estimated_position3D_
 *       and A_ in the reference's own POD layouts (Match, Segment3D fields, CLEdge,
 *       SparseMatrix COO) so clustering / optimisation can run unchanged.
 *   (2) seam layer     -- replaces the accelerator seam the reference already has in
 *       cudawrapper.h:54-80 (match_lines_GPU / score_matches_GPU), for a maintainer who
 *       wants to keep Line3D's own driver loop and only swap the kernels.
 *
 * All functions return 0 on success or a negative l3d_status; l3d_last_error() gives text.
 * Semantics follow the reference CPU path (line3D.cc), not its CUDA path.
 * ===========================================================================*/
#ifndef L3DPP_HIP_H_
#define L3DPP_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- PODs with the reference's exact layout -------------------------------------- */

/* L3DPP::Match, commons.h:186-203 (40 bytes) */
typedef struct l3d_match {
    uint32_t src_camID_, src_segID_, tgt_camID_, tgt_segID_;
    float overlap_score_, score3D_;
    float depth_p1_, depth_p2_, depth_q1_, depth_q2_;
} l3d_match;

/* L3DPP::Segment2D, commons.h:104-131 */
typedef struct l3d_segment2d { uint32_t camID_, segID_; } l3d_segment2d;

/* the data members of L3DPP::Segment3D, segment3D.h:99-115 (P1,P2,dir double; length float; valid) */
typedef struct l3d_segment3d {
    double P1[3], P2[3], dir[3];
    float length_;
    uint32_t valid_;
} l3d_segment3d;

/* L3DPP::CLEdge, clustering.h:47-51 */
typedef struct l3d_cledge { int32_t i_, j_; float w_; } l3d_cledge;

/* float4 entry of L3DPP::SparseMatrix (sparsematrix.cc:40: (i, j, w, 0)) */
typedef struct l3d_float4 { float x, y, z, w; } l3d_float4;

/* one phase-A result slot: what a (src segment, rank) of a directed view pair holds.
 * 32 bytes; this is also the record the multi-GPU all-gather exchanges. */
typedef struct l3d_slot {
    uint32_t tgt_seg;   /* 0xFFFFFFFF = empty */
    float overlap;
    float depth_p1, depth_p2, depth_q1, depth_q2;
    float score3D;      /* written when the src view is processed (scoringCPU) */
    uint32_t flags;     /* bit0: survived the src view's orientation filter (checkMatchOrientation); bit1: so did
                         * its inverse copy in the tgt view.  Set by phase A itself when kNN > 0. */
} l3d_slot;

typedef enum l3d_status {
    L3D_OK = 0,
    L3D_ERR_ARG = -1,          /* bad argument */
    L3D_ERR_IMAGE_SMALL = -2,  /* line3D.cc:119 */
    L3D_ERR_ID_IN_USE = -3,    /* line3D.cc:130 */
    L3D_ERR_NO_NEIGHBORS = -4, /* line3D.cc:154 */
    L3D_ERR_NO_SEGMENTS = -5,  /* line3D.cc:188 */
    L3D_ERR_NO_VIEWS = -6,     /* line3D.cc:385 */
    L3D_ERR_STATE = -7,        /* call order */
    L3D_ERR_HIP = -8,          /* HIP runtime error */
    L3D_ERR_LIMIT = -9,        /* size limit of this build */
    L3D_ERR_RETRY = -10,       /* l3d_match_finish after l3d_lists_shard: the record pools were enlarged, repeat
                                * l3d_lists_shard + the exchange of its slabs + l3d_match_finish (every rank gets it) */
    L3D_ERR_IO = -11           /* a binary input file is truncated, over-long or states a count it cannot hold */
} l3d_status;

typedef struct l3d_ctx l3d_ctx;

/* Line3D::matchImages arguments, line3D.h:143-148 (defaults commons.h:51-55) */
typedef struct l3d_match_params {
    float sigma_position;             /* 2.5  */
    float sigma_angle;                /* 10.0 */
    uint32_t num_neighbors;           /* 10   */
    float epipolar_overlap;           /* 0.25 */
    int32_t kNN;                      /* 10   */
    float const_regularization_depth; /* -1   */
} l3d_match_params;

const char* l3d_last_error(void);
/* build info: "gfx950;..." */
const char* l3d_build_info(void);
/* Device and pinned blocks that contexts release are kept in a process-wide cache for the next context (hipFree /
 * hipHostMalloc cost milliseconds per scene otherwise): at most a quarter of the device's memory (L3D_CACHE_MAX_MB) and
 * 1 GiB pinned; emptied automatically when an allocation fails.  l3d_trim_cache() hands everything cached back to the
 * runtime now (returns the bytes freed) -- for a process that shares the device with other allocators. */
uint64_t l3d_trim_cache(void);

/* ---- (1) context layer ------------------------------------------------------------- */

/* Line3D::Line3D (line3D.cc:6-69) with use_GPU=true (neighbours: per view, l3d_add_view / l3d_add_view_worldpoints).
 * `device` = HIP device ordinal.  `stream` = hipStream_t to launch on (0 = default stream). */
l3d_ctx* l3d_create(int device, void* stream);
void l3d_destroy(l3d_ctx*);

/* Line3D::addImage (line3D.cc:112-227) with explicit `line_segments` and explicit neighbour
 * list; the image contributes only width/height.  segs4 = M x (x1,y1,x2,y2) pixels. */
int l3d_add_view(l3d_ctx*, uint32_t camID, const float* segs4, uint32_t M, const double K[9],
                 const double R[9], const double t[3], uint32_t width, uint32_t height,
                 float median_depth, const uint32_t* neighbors, uint32_t n_neighbors);

/* The same with a WORLDPOINT list instead of the neighbour list: Line3D::addImage on an instance constructed with
 * neighbors_by_worldpoints=true (line3D.cc:216-219, processWPlist :230-240).  The view's visual neighbours are then
 * found from the worldpoint overlap inside every matchImages / l3d_match_begin: Line3D::findVisualNeighborsFromWPs
 * (line3D.cc:578-699; host code, line3dpp_amd/csrc/l3d_neighbors.hip). */
int l3d_add_view_worldpoints(l3d_ctx*, uint32_t camID, const float* segs4, uint32_t M, const double K[9],
                             const double R[9], const double t[3], uint32_t width, uint32_t height,
                             float median_depth, const uint32_t* worldpoints, uint32_t n_worldpoints);
/* visual_neighbors_[camID] (line3D.h:352) as the last matchImages / l3d_match_begin left it, ascending; *n = its size
 * (out may be NULL or shorter: the first `cap` are written) */
int l3d_get_visual_neighbors(l3d_ctx*, uint32_t camID, uint32_t* out, uint32_t cap, uint32_t* n);
/* Line3D::findVisualNeighborsFromWPs for a set of cameras without a context (and without a GPU): cameras as handed to
 * addImage (row-major K, R, t per view), worldpoint lists in CSR form (wp_offsets[n_views + 1]); the neighbour sets come
 * back in CSR form (nb_offsets[n_views + 1]; neighbors may be NULL to ask for the sizes).  The cameras are moved by
 * the median of their centres for the computation, as matchImages does (line3D.cc:436, 500-536). */
int l3d_neighbors_from_worldpoints(uint32_t n_views, const uint32_t* cam_ids, const double* K9, const double* R9,
                                   const double* t3, const uint64_t* wp_offsets, const uint32_t* worldpoints,
                                   uint32_t num_neighbors, uint64_t* nb_offsets, uint32_t* neighbors, uint64_t cap);

/* ---- input side (host code, no GPU) ---------------------------------------------------------------------------------
 * VisualSfM .nvm exactly as main_vsfm.cpp:144-250 reads it, with what it derives per camera (:188-206, :300-303).  The
 * camera index is the camID main_vsfm.cpp passes to addImage; a camera that sees no point has n_worldpoints == 0 and
 * is skipped there (:258). */
typedef struct l3d_nvm l3d_nvm;
typedef struct l3d_nvm_camera {
    const char* filename;             /* valid while the handle lives */
    float focal, distortion;          /* (float vectors in main_vsfm.cpp:164-169) */
    float median_depth;               /* sorted point distances [n/2], the value handed to addImage */
    uint32_t n_worldpoints;
    double R[9], t[3], C[3];          /* row-major R from the quaternion, t = -R C */
} l3d_nvm_camera;
int l3d_nvm_open(const char* path, l3d_nvm** out);    /* L3D_ERR_NO_VIEWS: "No aligned cameras in NVM file!" (:157-161) */
uint32_t l3d_nvm_num_cameras(const l3d_nvm*);
int l3d_nvm_get_camera(const l3d_nvm*, uint32_t index, l3d_nvm_camera* out);
int l3d_nvm_get_worldpoints(const l3d_nvm*, uint32_t index, uint32_t* out, uint32_t cap);   /* = addImage's wps list */
void l3d_nvm_close(l3d_nvm*);
void l3d_nvm_intrinsics(float focal, uint32_t width, uint32_t height, double K[9]);          /* main_vsfm.cpp:272-282 */
/* COLMAP results (cameras.txt / images.txt / points3D.txt of a folder, main_colmap.cpp:136-348; where cameras.txt is
 * absent and cameras.bin, images.bin and points3D.bin all exist, COLMAP's binary form of the same: DESIGN §15) and bundler files
 * (bundle.rd.out, main_bundler.cpp:147-252) with what those front ends derive per image: K (COLMAP; bundler builds it
 * from the image size: l3d_nvm_intrinsics), R, t, C = R^T (-t), the distortion coefficients handed to undistortImage,
 * the worldpoint list and the median worldpoint distance handed to addImage.  Images in file order; `id` is the camID
 * the front end passes to addImage (COLMAP: IMAGE_ID, bundler: the camera index); n_worldpoints == 0: skipped there. */
typedef struct l3d_sfm l3d_sfm;
typedef struct l3d_sfm_image {
    uint32_t id, camera;              /* camID for addImage; COLMAP CAMERA_ID (bundler: = id) */
    uint32_t width, height;           /* COLMAP: from cameras.txt (the reference takes the size from the image file); bundler: 0 */
    const char* name;                 /* COLMAP image name (valid while the handle lives); bundler: "" */
    float focal;                      /* bundler focal length (float there); COLMAP: (float)fx */
    float median_depth;
    uint32_t n_worldpoints;
    double K[9];                      /* COLMAP; bundler: zeros */
    double R[9], t[3], C[3];
    double radial[3], tangential[2];  /* k1 k2 k3, p1 p2 */
} l3d_sfm_image;
int l3d_sfm_open_colmap(const char* folder, l3d_sfm** out);
int l3d_sfm_open_bundler(const char* bundle_file, l3d_sfm** out);   /* L3D_ERR_NO_VIEWS: "No cameras and/or points in bundle file!" */
uint32_t l3d_sfm_num_images(const l3d_sfm*);
int l3d_sfm_get_image(const l3d_sfm*, uint32_t index, l3d_sfm_image* out);
int l3d_sfm_get_worldpoints(const l3d_sfm*, uint32_t index, uint32_t* out, uint32_t cap);
void l3d_sfm_close(l3d_sfm*);
/* COLMAP's camera model of image `index` as l3d_undistort_images_model takes it (K_new all zero).  A model that has no
 * l3d_camera_model form (SIMPLE_PINHOLE .. OPENCV, which l3d_sfm_image's five coefficients describe in full) and a
 * bundler handle: model = L3D_CAM_NONE, K as in l3d_sfm_image, params zero.  The declaration of l3d_camera_model is
 * with the undistortion entries below. */
struct l3d_camera_model;
int l3d_sfm_get_camera_model(const l3d_sfm*, uint32_t index, struct l3d_camera_model* out);
/* COLMAP's name of the camera model of image `index` ("" for a bundler handle) and its raw parameter list in
 * cameras.txt's order: up to `cap` values to params (may be NULL), *n = their number. */
const char* l3d_sfm_get_camera_params(const l3d_sfm*, uint32_t index, double* params, uint32_t cap, uint32_t* n);
/* The segment cache Line3D::detectLineSegments loads / stores per image when load_segments is set (line3D.cc:295-309,
 * 362-366): "<data folder>/segments_L3D++_<camID>_<width>x<height>_<max segments>.bin", the boost binary archive of a
 * one-row L3DPP::DataArray<float4> (dataArray.h:352-374).  segs4 = n x (x1, y1, x2, y2). */
int l3d_segment_cache_name(uint32_t camID, uint32_t width, uint32_t height, uint32_t max_segments, char* out, uint32_t cap);
int l3d_read_segment_cache(const char* path, float* segs4 /* may be NULL */, uint32_t cap, uint32_t* n);
int l3d_write_segment_cache(const char* path, const float* segs4, uint32_t n);

/* ---- line-segment detection (Line3D::detectLineSegments, line3D.cc:243-370; GPU: k_lsd.hip) ------------------------
 * An 8-bit image: channels 1 (CV_8U, grey) or 3 (CV_8UC3; converted with CV_RGB2GRAY, the first channel counts as R);
 * any other count is "image type not supported" (L3D_ERR_ARG).  row_stride in bytes (>= cols * channels).  Detection
 * expects undistorted pixels: a front end that calls Line3D::undistortImage first does so with l3d_undistort_images. */
typedef struct l3d_image {
    const uint8_t* data;
    uint32_t cols, rows, channels, row_stride;
} l3d_image;
/* the constructor arguments of Line3D that detection reads (line3D.cc:6-12) */
typedef struct l3d_detect_options {
    const char* output_folder;        /* the cache lives in <output_folder>/L3D++_data/ */
    int32_t load_segments;            /* load the segment cache if it exists, store it after detecting */
    int32_t max_image_width;          /* <= 0: no downscale */
    uint32_t max_line_segments;       /* cap on segments per image (3000 in the reference) */
} l3d_detect_options;
/* per image of the last detection */
typedef struct l3d_detect_stats {
    uint32_t width, height;           /* image handed to LSD (after the max-width downscale) */
    uint32_t raw_segments;            /* LSD output before the length filter and the cap */
    uint32_t segments;                /* what the call returned */
    uint32_t from_cache;              /* 1: loaded from the segment cache, LSD did not run */
    uint32_t seeds;                   /* regions grown */
    uint32_t nfa_evals;               /* rect_nfa evaluations */
    uint32_t reserved;
    double max_grad;                  /* ll_angle's largest defined gradient norm (-1: none) */
} l3d_detect_stats;
/* LSD with the reference's filter, order and cap on a batch of images (one launch set for all of them); no cache.
 * counts[n_images] = segments per image; the segments themselves: l3d_get_detected_segments. */
int l3d_detect_segments(l3d_ctx*, uint32_t n_images, const l3d_image* images, int max_image_width,
                        uint32_t max_segments, uint32_t* counts);
/* The same with the segment cache as Line3D::detectLineSegments uses it (opts->load_segments): a cached image is read,
 * the others are detected in one batch and stored.  camIDs name the cache files. */
int l3d_detect_view_segments(l3d_ctx*, uint32_t n_images, const uint32_t* camIDs, const l3d_image* images,
                             const l3d_detect_options* opts, uint32_t* counts);
/* segments of the last detection on this context, image after image: n x (x1, y1, x2, y2); *n = their number.  "Last"
 * is context-wide: with several threads detecting on one context, the caller must order the two calls itself. */
int l3d_get_detected_segments(l3d_ctx*, float* segs4 /* may be NULL */, uint64_t cap, uint64_t* n);
int l3d_get_detect_stats(l3d_ctx*, l3d_detect_stats* out, uint32_t cap, uint32_t* n);
/* Line3D::addImage with empty line_segments: detect (or load from the cache), then add the view as l3d_add_view /
 * l3d_add_view_worldpoints do.  No segment survives: L3D_ERR_NO_SEGMENTS, the view is not added (line3D.cc:184-190).
 * *n_segments (may be NULL) = the number of segments THIS view was added with (0 when it was not added), set inside the
 * call: concurrent callers must take it from here, not from l3d_get_detected_segments, which another thread's call may
 * have replaced in between.  The call holds the context mutex for the whole detection, so concurrent calls on one
 * context run one after another; to detect many images at once, use l3d_detect_view_segments (one batch) and add the
 * views with their segments. */
int l3d_add_view_image(l3d_ctx*, uint32_t camID, const l3d_image* image, const l3d_detect_options* opts,
                       const double K[9], const double R[9], const double t[3], float median_depth,
                       const uint32_t* neighbors, uint32_t n_neighbors, uint32_t* n_segments);
int l3d_add_view_image_worldpoints(l3d_ctx*, uint32_t camID, const l3d_image* image, const l3d_detect_options* opts,
                                   const double K[9], const double R[9], const double t[3], float median_depth,
                                   const uint32_t* worldpoints, uint32_t n_worldpoints, uint32_t* n_segments);

/* ---- undistortion (Line3D::undistortImage, line3D.cc:83-109; GPU: k_undistort.hip) ---------------------------------
 * The arguments of undistortImage: K row-major (only fx = K[0], fy = K[4], cx = K[2], cy = K[5] are read: cvK drops
 * the skew), radial = (k1, k2, k3), tangential = (p1, p2), i.e. OpenCV's (k1, k2, p1, p2, k3).  DESIGN §12 defines the
 * arithmetic (initUndistortRectifyMap with CV_16SC2 maps, remap INTER_LINEAR with a border of 0).  Images as for
 * detection (l3d_image: 8-bit, 1 or 3 channels, else L3D_ERR_ARG); a non-finite coefficient or fx, fy, cx, cy, or
 * fx * fy == 0: L3D_ERR_ARG; a side of 32767 or more: L3D_ERR_LIMIT.  Every image is checked before any is read. */
typedef struct l3d_distortion { double K[9]; double radial[3]; double tangential[2]; } l3d_distortion;
/* Line3D::undistortImage (line3D.cc:83-109) for a batch of images in one launch.  out[i] receives rows x
   cols*channels bytes, packed, and may be the input's own host memory.  Calls on one context are serialised. */
int l3d_undistort_images(l3d_ctx*, uint32_t n_images, const l3d_image* in, const l3d_distortion* dist,
                         uint8_t* const* out);
/* Undistortion by camera model: COLMAP's models beyond the five OpenCV coefficients.  params in COLMAP's
 * order behind the focal lengths and the principal point, unused ones 0:
 *   L3D_CAM_FULL_OPENCV            k1 k2 p1 p2 k3 k4 k5 k6
 *   L3D_CAM_OPENCV_FISHEYE         k1 k2 k3 k4
 *   L3D_CAM_SIMPLE_RADIAL_FISHEYE  k
 *   L3D_CAM_RADIAL_FISHEYE         k1 k2
 *   L3D_CAM_FOV                    omega
 * K is the camera matrix of the input image, K_new that of the output image (all zero: K, which is what
 * Line3D::undistortImage passes to initUndistortRectifyMap); of both only fx, fy, cx, cy are read. */
enum { L3D_CAM_NONE = 0, L3D_CAM_FULL_OPENCV = 1, L3D_CAM_OPENCV_FISHEYE = 2, L3D_CAM_SIMPLE_RADIAL_FISHEYE = 3,
       L3D_CAM_RADIAL_FISHEYE = 4, L3D_CAM_FOV = 5 };
typedef struct l3d_camera_model {
    uint32_t model;
    uint32_t reserved;
    double K[9];
    double params[8];
    double K_new[9];
} l3d_camera_model;
/* A batch in one launch; models and sizes may be mixed.  The checks of l3d_undistort_images (on K, on a non-zero K_new
 * and on the model's parameters) and an unknown model (L3D_ERR_ARG) are made for every image before any pixel is
 * read.  out[i] as for l3d_undistort_images. */
int l3d_undistort_images_model(l3d_ctx*, uint32_t n_images, const l3d_image* in, const l3d_camera_model* cams,
                               uint8_t* const* out);

/* Line3D::matchImages (line3D.cc:375-497): the whole call on this context's GPU. */
int l3d_match_images(l3d_ctx*, const l3d_match_params*);

/* matchImages split in three for pair-sharded multi-GPU runs (one process per GPU):
 *   l3d_match_begin   param clamps, translate(), per-view k, neighbour sets, directed pair
 *                     list (line3D.cc:394-485, 704-741), upload + per-view precompute
 *   l3d_match_pairs   matchingCPU (line3D.cc:900-1015) for the pairs [first, first+count) of
 *                     the pair list -> their slots in the slot buffer
 *   (exchange: all-gather of the slot buffer, done by the caller, e.g. RCCL through
 *    torch.distributed on the device pointer l3d_slot_buffer() returns)
 *   l3d_match_finish  per view, ascending camID: checkMatchOrientation, scoringCPU,
 *                     storeInverseMatches, filterMatches (line3D.cc:745-773); untranslate() */
int l3d_match_begin(l3d_ctx*, const l3d_match_params*);
int l3d_num_pairs(l3d_ctx*, uint32_t* n);
int l3d_get_pairs(l3d_ctx*, uint32_t* src_cam, uint32_t* tgt_cam, uint64_t* slot_offset /* in slots */);
int l3d_match_pairs(l3d_ctx*, uint32_t first, uint32_t count);
int l3d_slot_buffer(l3d_ctx*, void** dev_ptr, uint64_t* n_slots);   /* (halo form of a multi-GPU call: only the regions of
                                                                       * the pairs this rank matched or received hold slots) */
/* test hook: copies the fresh-hypothesis stream the list pass reads to the host, out[2 i], out[2 i + 1] = (depth_p1, depth_p2)
 * of slot i of the slot buffer when the slot is alive (kSlotAlive in its flags), NaN otherwise; n = n_slots of
 * l3d_slot_buffer.  Read only; meaningful after l3d_match_finish / l3d_lists_shard* of the current call. */
int l3d_get_fresh_hyp(l3d_ctx*, float* out, uint64_t n);
/* (kNN <= 0, keep every match -- line3D.cc:982-992: the device buffer is RAGGED, a row holds exactly its matches in ascending
 *  target order and n_slots is their number; l3d_get_pairs' slot_offset is the pair's first slot; l3d_get_pair_slots below
 *  hands a pair out in the padded Ms x K form, K = its longest row.  The mode runs unsharded.) */
/* tell the context that the caller's exchange has filled in the slots of all other pairs */
int l3d_slots_exchanged(l3d_ctx*);
/* Compact form of the same exchange (kNN > 0): only the target index of every slot travels (4 B instead of 32);
 * overlap and depths are functions of (pair, source row, target index) and are re-derived on the receiving rank by
 * the match kernel's own device functions, bit-identically.
 *   l3d_pack_slot_indices    slots of the rank's own pairs [first, first+count) -> index buffer (returns when done)
 *   (all-gather of the u32 index buffer l3d_slot_index_buffer() returns, by the caller)
 *   l3d_expand_slot_indices  index buffer -> slots of the foreign pairs [first, first+count); marks them matched
 * Replaces the host-side gather of per-view match lists a multi-GPU run of the reference would need between
 * matchingCPU and the per-view chain (line3D.cc:728-773). */
int l3d_slot_index_buffer(l3d_ctx*, void** dev_ptr, uint64_t* n_slots);
int l3d_pack_slot_indices(l3d_ctx*, uint32_t first, uint32_t count);
int l3d_expand_slot_indices(l3d_ctx*, uint32_t first, uint32_t count);
int l3d_match_finish(l3d_ctx*);
/* Phase B sharded over ranks as well (optional step between the slot exchange and l3d_match_finish; every pair must be
 * present): the dense part of phase B -- one pass over every 2D segment's hypothesis list that finds the supporting
 * pairs of similarityForScoring (line3D.cc:1208-1294, 1417-1446) -- is run for the views of rank `rank` of `world`
 * only (contiguous view ranges of equal segment count).  Its output records live in pools; rank r fills the pools
 * [r * 256/world, (r+1) * 256/world) of four arrays (edges, headers, segment headers, pool counters).  On return
 * slab_ptr[k] / slab_bytes[k] describe THIS rank's slab of array k and full_ptr[k] the array itself (device
 * pointers; rank r's slab starts at full_ptr[k] + r * slab_bytes[k]): the caller all-gathers the four arrays slab by
 * slab (e.g. ncclAllGather) and then calls l3d_match_finish, which runs the cheap sparse remainder of phase B (the
 * chain of inverse matches, scores, filterMatches, outputs) on the complete records on every rank.  Returns when the
 * slabs are complete in device memory. */
int l3d_lists_shard(l3d_ctx*, uint32_t rank, uint32_t world, void* slab_ptr[4], uint64_t slab_bytes[4], void* full_ptr[4]);
/* The same for an explicit range of views [view0, view1) (indices in ascending camID order) -- the halo form of a
 * multi-GPU run (line3dpp_amd/dist.py, tests/cpp/rccl_driver.cpp): rank r owns the views l3d_plan_shards gives it,
 * matches the pairs whose SOURCE view it owns, receives the pairs whose TARGET view it owns from their owners (compact
 * index form, l3d_pack_slot_indices / l3d_expand_slot_indices per run of consecutive pairs) and runs the list pass of its
 * views: only the pairs that touch [view0, view1) have to be present.  The records are all-gathered as above; the
 * replicated remainder of phase B works on the records alone. */
int l3d_lists_shard_views(l3d_ctx*, uint32_t rank, uint32_t world, uint32_t view0, uint32_t view1, void* slab_ptr[4],
                          uint64_t slab_bytes[4], void* full_ptr[4]);
/* The tail of phase B sharded by views as well (optional, instead of l3d_match_finish after l3d_lists_shard_views and the
 * exchange of its slabs).  The chain of storeInverseMatches (line3D.cc:1672-1699) is a global fixed point over the
 * records of all ranks and every rank runs it; scoringCPU's scores, filterMatches (:1586-1669), the surviving matches_
 * lists, estimated_position3D_ and the view medians are per view and are computed by the rank that owns the view:
 *   l3d_tail_shard_count   chain + scores + filterMatches + counts of this rank's views: counts[0] = its surviving
 *                          matches, counts[1] = its best hypotheses (L3D_ERR_RETRY as l3d_match_finish gives it)
 *   -- the caller all-gathers the two counts of every rank --
 *   l3d_tail_shard_layout  this rank's outputs, written at their places in the full arrays, and where every rank's parts
 *                          are: nine arrays (Match, target / source segment of a match, HypRec, depth pairs, the three
 *                          per-segment arrays, the view medians): base_ptr[k] device pointer, elt_bytes[k] element size,
 *                          first[9 r + k] / count[9 r + k] the elements of rank r.  view_bounds[world + 1]: the view
 *                          ranges of the ranks (those of the list pass)
 *   -- the caller exchanges the parts: rank r's part of array k to every other rank, in place --
 *   l3d_tail_shard_commit  closes the call as l3d_match_finish does (medians to the host, totals, views untranslated) */
int l3d_tail_shard_count(l3d_ctx*, uint32_t counts[2]);
/* Options of the sharded entries of this context (round 6; they hold until changed):
 *   first_needed_rank   the chain of a rank only has to cover the records its views DEPEND on: view v depends on view u < v when a
 *                       pair (u -> v) hands inverse matches over (line3D.cc:1680), transitively.  With contiguous view ranges the
 *                       ranks a rank depends on lie below it; the caller (which knows the pair list: l3d_plan_shards) passes the
 *                       lowest one.  The chain walks the pools of EVERY rank in [first_needed_rank, rank], so the caller must
 *                       deliver the record slabs of every rank in that range, including those of a rank in between that this
 *                       rank does not depend on; it may leave the record slabs of ranks outside the range unexchanged.  The
 *                       COUNTER slab (array 3 of l3d_lists_shard*) must still reach every rank, it carries the pool
 *                       overflow flags all ranks decide on alike.  0 (default): all ranks below (and the records of all ranks
 *                       must be present, as before).
 *   exchanges_stream_ordered   nonzero: the caller's exchanges are ordered behind the context's stream by themselves (RCCL
 *                       on the same stream): l3d_lists_shard*, l3d_tail_shard_layout and l3d_affinity_shard_begin then return
 *                       WITHOUT waiting for the device (three host synchronisations less per call).  0 (default): they
 *                       return when their slabs / parts are complete in device memory. */
int l3d_shard_options(l3d_ctx*, uint32_t first_needed_rank, int exchanges_stream_ordered);
int l3d_tail_shard_layout(l3d_ctx*, uint32_t world, const uint32_t* counts_all, const uint32_t* view_bounds, void* base_ptr[9],
                          uint64_t elt_bytes[9], uint64_t* first, uint64_t* count);
int l3d_tail_shard_commit(l3d_ctx*);
/* The affinity fill of Line3D::reconstruct3Dlines (computingAffinityMatrix, line3D.cc:1852-1979) sharded by the same
 * views, for a call that was closed by l3d_tail_shard_commit (the similarity of a candidate depends on its
 * two hypotheses alone).  Instead of l3d_compute_affinity:
 *   l3d_affinity_shard_begin   similarity (line3D.cc:1467-1553) of the surviving matches of this rank's views, written at
 *                              their places in the full float array *simv; first[r] / count[r]: the elements of rank r
 *   -- the caller exchanges the parts: rank r's part to every other rank, in place --
 *   l3d_affinity_shard_finish  used_ / local ids / CLEdge pairs from all similarities (every rank: same A_ everywhere)
 * Not with collinearity_t > 0 (line3D.cc:1904-1974 is sequential by definition): L3D_ERR_LIMIT, use l3d_compute_affinity. */
int l3d_affinity_shard_begin(l3d_ctx*, uint32_t rank, uint32_t world, void** simv, uint64_t* first, uint64_t* count);
int l3d_affinity_shard_finish(l3d_ctx*);
/* closes an open sharded fill without the bookkeeping pass (a peer failed, its similarities never arrived: the caller goes
 * on to l3d_compute_affinity on every rank): views untranslated, nothing else touched.  L3D_OK also when none is open. */
int l3d_affinity_shard_abort(l3d_ctx*);
/* Partition of a call over `world` ranks (host only; a function of the pair list of l3d_get_pairs): contiguous view
 * ranges whose outgoing pairs carry equal shares of the cost (pair_cost[p], e.g. Ms * Mt); pair_src_view[p] = index of
 * the pair's source view (the list is ordered by it).  view_bounds / pair_bounds receive world + 1 entries: rank r owns
 * the views [view_bounds[r], view_bounds[r+1]) and the pairs [pair_bounds[r], pair_bounds[r+1]). */
int l3d_plan_shards(uint32_t n_views, uint32_t n_pairs, const uint32_t* pair_src_view, const uint64_t* pair_cost,
                    uint32_t world, uint32_t* view_bounds, uint32_t* pair_bounds);
/* Leaves an open l3d_match_begin without results: everything queued is drained, the views are moved back
 * (matchImages translates them for its duration, line3D.cc:436/493), the context is idle again.  A no-op when no
 * begin is open.  Every failing l3d_match_begin / l3d_match_images / l3d_match_finish does this itself; callers that
 * give up between the split calls (e.g. a failed exchange in a multi-GPU run) call it explicitly. */
int l3d_match_abort(l3d_ctx*);

/* The affinity part of Line3D::reconstruct3Dlines: translate(), med_scene_depth_lines_,
 * computingAffinityMatrix(), untranslate() (line3D.cc:1749-1778, 1852-2023; collinearity off). */
int l3d_compute_affinity(l3d_ctx*);

/* Line3D::reconstruct3Dlines (line3D.cc:1702-1824) up to the final 3D segments: translate(), affinity matrix
 * (as l3d_compute_affinity), graph clustering (clustering.cc), 3D line per cluster, collinear 3D segments,
 * filterTinySegments, untranslate().  perform_diffusion != 0 runs the replicator-dynamics diffusion of A_
 * (performRDD, line3D.cc:2026-2076) on the device-resident matrix; collinearity_t > 0 adds the per-image collinearity
 * tests (View::findCollinearSegments, view.cc:150-258) and the collinear affinity links (line3D.cc:1904-1974).
 * use_CERES != 0 bundles the 3D lines between the clustering and the final 3D segments (optimizeClusters,
 * line3D.cc:1800-1805; LineOptimizer::optimize, optimization.cc): per line, the reference's robust reprojection cost
 * (Huber(2) on the squared 2-vector of end point distances, angle weighted) over its 4 Cayley parameters, cameras and
 * intrinsics constant, minimised by Levenberg-Marquardt with at most max_iter_CERES iterations -- one kernel launch for
 * all lines (k_lineopt.hip).  The reference solves all lines as one Ceres problem with one trust region and one
 * stopping test, so the per-line iterates and stopping points are not the reference's: what is kept is the cost
 * function and a per-line local optimum of it.  The output file names then carry "OPTIMIZED__" (line3D.cc:2889-2890);
 * l3d_line_opt_stats reports the stage.  use_CERES = 0 leaves the path exactly as it was.
 * The clustering / reconstruction tail is small sequential host work in the reference and runs on the host
 * here as well. */
int l3d_reconstruct_3d_lines(l3d_ctx*, uint32_t visibility_t, int perform_diffusion, float collinearity_t,
                             int use_CERES, uint32_t max_iter_CERES);
/* Line3D::get3Dlines (line3D.cc:2455-2463): lines3D_ flattened.  Line i owns the 3D segments
 * [seg_offsets[i], seg_offsets[i+1]) (collinear3Dsegments_) and the residual 2D segments
 * [res_offsets[i], res_offsets[i+1]) (underlyingCluster_.residuals_); cluster_lines[i] is
 * underlyingCluster_.seg3D_, reference_views[i] its reference_view_.  Original (untranslated) frame. */
int l3d_num_3d_lines(l3d_ctx*, uint32_t* n_lines, uint32_t* n_segments, uint32_t* n_residuals);
/* what the line bundling of the last reconstruct3Dlines did (all zero when it ran with use_CERES = 0) */
typedef struct l3d_line_opt_summary {
    uint32_t lines_bundled;   /* clusters whose parameters were optimised */
    uint32_t lines_constant;  /* clusters held constant: a NaN in their Cayley form (the reference's #unoptimizable_lines) */
    uint32_t lines_dropped;   /* clusters dropped at write-back (|P1 - P2| <= 1e-12) */
    uint32_t stop_gradient, stop_function, stop_parameter, stop_max_iter;   /* bundled lines stopped by each rule */
    uint32_t stop_other;      /* ... by a failed evaluation at the start or a collapsed trust region */
    uint32_t max_iterations;  /* largest iteration count of a line */
    uint32_t residuals;       /* residual 2D segments of all clusters */
    uint32_t lines_wide;      /* bundled lines with more than 16 residuals (one wave each; the rest: 16 lanes each) */
    uint32_t max_residuals;   /* largest residual count of a bundled line */
    double cost_before, cost_after;   /* sum of the bundled lines' robust costs at the start / at the end */
    float kernel_ms;          /* the bundling kernel (one event pair; only at timing level >= 2, else 0) */
    uint32_t reserved;
} l3d_line_opt_summary;
int l3d_line_opt_stats(l3d_ctx*, l3d_line_opt_summary* out);
int l3d_get_3d_lines(l3d_ctx*, uint32_t* seg_offsets, l3d_segment3d* segments, uint32_t* res_offsets,
                     l3d_segment2d* residuals, l3d_segment3d* cluster_lines, uint32_t* reference_views);

/* block the calling thread until everything queued on the context's stream has finished */
int l3d_synchronize(l3d_ctx*);

/* ---- accessors (host copies, reference layouts) ------------------------------------ */

/* number of directed pair tests matchImages performed: sum Ms*Mt */
int l3d_pair_tests(l3d_ctx*, uint64_t* n);
/* matches_[camID] after matchImages: CSR over the view's segments.
 * seg_offsets has M+1 entries.  Call with out=NULL to get the count. */
int l3d_get_matches(l3d_ctx*, uint32_t camID, l3d_match* out, uint64_t cap, uint32_t* seg_offsets,
                    uint64_t* n);
/* fresh phase-A slots of one directed pair: Ms x K slots (K = kNN; kNN <= 0: K = the pair's longest row, shorter rows
 * padded with empty slots) */
int l3d_get_pair_slots(l3d_ctx*, uint32_t pair_index, l3d_slot* out, uint64_t cap, uint32_t* Ms,
                       uint32_t* K);
/* estimated_position3D_ (+ entry_map_ keys), ordered by (camID, segID). Coordinates are in the
 * translated frame matchImages works in (the reference never untranslates them). */
int l3d_num_best(l3d_ctx*, uint32_t* n);
int l3d_get_best(l3d_ctx*, l3d_segment2d* seg2d, l3d_segment3d* seg3d, l3d_match* best);
/* per view: View::k(), View::median_depth() after matchImages */
int l3d_view_info(l3d_ctx*, uint32_t camID, float* k, float* median_depth);
int l3d_translation(l3d_ctx*, double t[3]);
/* A_ (CLEdge list, both (i,j) and (j,i)), local2global_ and med_scene_depth_lines_ */
int l3d_num_affinity(l3d_ctx*, uint32_t* n_edges, uint32_t* n_rows);
int l3d_get_affinity(l3d_ctx*, l3d_cledge* edges, l3d_segment2d* local2global, float* med_scene_depth_lines);
/* L3DPP::SparseMatrix(A_, n_rows, 1.0, sort_by_row) (sparsematrix.cc:8-60): entries float4(i,j,w,0)
 * sorted by row or column, start_indices[n_rows] with -1 for empty rows/columns */
int l3d_get_sparse_matrix(l3d_ctx*, int sort_by_row, l3d_float4* entries, int32_t* start_indices);

/* test hook (host only): principal direction of a row-major symmetric 3x3 scatter matrix as Line3D::get3DlineFromCluster
 * (line3D.cc:2196-2211) takes it from JacobiSVD -- this library's closed-form solver, checked against LAPACK on the CPU */
int l3d_principal_direction(const double S9[9], double dir3[3]);
/* test hooks (host only) of the line bundling: LineOptimizer::optimize's parametrisation of the line through P1, P2
 * (Plücker, then Cayley: x = (omega, s), optimization.cc:31-95; returns 1 when the line is held constant, x = (-1,0,0,0))
 * and its write-back (optimization.cc:209-295: new end points from x around the old mid point; returns 0 when the
 * cluster is dropped) */
int l3d_line_to_cayley(const double P1[3], const double P2[3], double x[4]);
int l3d_cayley_to_segment(const double x[4], const double P1_old[3], const double P2_old[3], double P1[3], double P2[3]);
/* test hook (device): the bundling kernel's own evaluator of LineReprojectionError (optimization.h) at line parameters
 * x for n observations: obs [n x 6] = (p1x, p1y, p2x, p2y, nx, ny) (end points, normal of the segment's direction),
 * cams [n x 16] = (R row-major, C, fx, fy, px, py).  residuals [2n]; jacobians [8n]: d r / d x, 2x4 row-major per
 * observation, before the loss; ok [n]: 0 where the evaluation fails (residual 0); *cost = 1/2 sum Huber2(|r_i|^2) */
int l3d_line_opt_eval(int device, uint32_t n, const double x[4], const double* obs, const double* cams, double* cost,
                      double* residuals, double* jacobians, int32_t* ok);
/* test hook (device): the bundling kernel's solver on its own -- the function the pipeline's stage calls, without a
 * context.  Line i starts at x0[4i .. 4i+3] = (omega, s) and owns the residuals [res_off[i], res_off[i+1]) (CSR, res_off[0]
 * == 0, non-decreasing; a line without residuals is legal); residual r is obs[6r .. 6r+5] = (p1x, p1y, p2x, p2y, nx, ny)
 * seen by camera obs_cam[r] < n_cams, cams [n_cams x 16] as for l3d_line_opt_eval.  The lines are solved in one launch
 * of k_lineopt in the stage's work order: a stable sort by residual count, longest first; the lines with more than
 * narrow_max residuals take a wave each, the others a 16-lane group (the stage passes 16; 0 sends every line through the
 * wave tier).  Per line, by its index in the input: x_out[4i ..] the final parameters, cost01[2i], cost01[2i + 1] the
 * robust cost at the start and at the end, iters[i] the iterations (accepted and rejected steps), status[i] the stopping
 * rule: 1 gradient, 2 function, 3 parameter, 4 max_iter, 5 other (a start point that cannot be evaluated, which keeps
 * x0 with iters 0, or a collapsed trust region).  L3D_ERR_ARG, with nothing launched and no output written: a null
 * pointer, res_off[0] != 0 or a decreasing res_off, an obs_cam[r] >= n_cams, narrow_max > 16.  n_lines == 0: L3D_OK. */
int l3d_line_opt_solve(int device, uint32_t n_lines, const double* x0, const uint32_t* res_off, const double* obs,
                       const uint32_t* obs_cam, uint32_t n_cams, const double* cams, uint32_t max_iter, uint32_t narrow_max,
                       double* x_out, double* cost01, uint32_t* iters, uint32_t* status);

/* main_pix4d.cpp's triangulation of tie points (linearHomTriangulation, main_pix4d.cpp:34-69, in the loop of :354-372)
 * on the device, one lane per point in fp64 (k_triangulate.hip).  P12: n_cameras row-major 3x4 projection matrices;
 * the observations of point i are obs_offsets[i] .. obs_offsets[i + 1] (CSR, obs_offsets[0] == 0): obs_camera names the
 * matrix, obs_xy the pixel.  Per point: the rows (0, -1, y) P_c and (1, 0, -x) P_c of every observation form A; v = the
 * singular vector of A^T A for its smallest singular value (cyclic Jacobi on the symmetric 4x4; the reference takes
 * JacobiSVD(AtA).matrixV().col(3)); X = v[0:3] / v[3].  valid[i] = 1 exactly when the point has more than two
 * observations and norm(X) > L3D_EPS in IEEE arithmetic (a NaN is invalid, an infinite X is valid); X3 holds X for a
 * valid point and zeros otherwise.  An observation of a camera >= n_cameras: L3D_ERR_ARG, nothing is launched;
 * n_points == 0: L3D_OK, nothing is launched.  Host pointers in and out. */
int l3d_triangulate_points(int device, uint32_t n_cameras, const double* P12, uint64_t n_points, const uint64_t* obs_offsets,
                           const uint32_t* obs_camera, const double* obs_xy, double* X3, uint8_t* valid);
/* Static members of the reference's Line3D (host only), row-major 3x3 out: rotationFromRPY (line3D.cc:2714-2727:
 * Rz(yaw) Ry(pitch) Rx(roll)), rotationFromQ (:2730-2754) and decomposeProjectionMatrix (:2784-2853: P = K [R | t] by
 * three Givens rotations; K with positive diagonal and K[2][2] = 1) */
int l3d_rotation_from_rpy(double roll, double pitch, double yaw, double R9[9]);
int l3d_rotation_from_q(double qw, double qx, double qy, double qz, double R9[9]);
int l3d_decompose_projection_matrix(const double P12[12], double K9[9], double R9[9], double t3[3]);

/* test hook (device): the unscaled IEEE division / square root of the exact tests (l3d_dev.h: rcp_refined, div_by,
 * sqrt_unscaled) against the compiler's own expansions on n random operand sets; counts[3] = results whose bits differ
 * (single divisions, paired divisions, square roots) -- all zero on a correct build */
int l3d_selftest_arith(int device, uint64_t n, uint64_t seed, uint64_t counts[3]);

/* test hook (device): the single-launch scan (k_scan.hip) on its own.  in: n_in elements of element_bytes (4: uint32; 8:
 * two packed 32-bit counters whose totals stay below 2^32).  Call k = 0 .. n_calls-1 scans in[0 .. n[k]) through
 * launch_scan / launch_scan64: all calls back to back on one stream and ONE work space (zeroed once, when it is
 * allocated), no host synchronisation between them.  Every call writes n[k] + 1 elements to a region of its own; `out`
 * receives the regions one after the other (sum of n[k] + 1 elements).  in_place != 0: the input is copied into the region
 * on the stream and scanned there.  pass_total != 0: the launcher is given a pointer for the total, totals[k] (n_calls
 * elements) receives what it stored; otherwise the launcher gets NULL and totals may be NULL.  After one
 * synchronisation: *ws_nonzero = 64-bit words of the work space that are not zero, *guard_changed = how many of the guard
 * words the hook put behind the work space no longer hold their pattern -- both 0 for a correct scan.
 * L3D_ERR_ARG before any device call: element_bytes other than 4 or 8, a null pointer, an n[k] above n_in. */
int l3d_selftest_scan(int device, uint32_t element_bytes, const void* in, uint32_t n_in, uint32_t n_calls, const uint32_t* n,
                      int in_place, int pass_total, void* out, void* totals, uint64_t* ws_nonzero, uint64_t* guard_changed);

/* test hook: route every segment pair through the exact double-precision test (no fp32 pre-filter);
 * used by the tests to prove that the pre-filter never loses a match */
int l3d_set_brute_force(l3d_ctx*, int on);

/* timing of the last calls, milliseconds of GPU time from HIP events on the context's stream */
typedef struct l3d_timings {
    float begin_ms;        /* upload + per-view precompute kernels */
    float match_pairs_ms;  /* phase A: pair-matching kernel(s) */
    float finish_ms;       /* phase B: per-view chain */
    float affinity_ms;
    uint32_t match_kernel_launches;
    float match_kernel_ms; /* the pair-matching kernel alone */
    float cull_prepare_ms; /* ordering of rows/targets by epipolar band (part of match_pairs_ms) */
    uint32_t culled_pairs; /* directed pairs matched with epipolar-band culling in the last matchImages */
    uint32_t list_entries; /* phase B: total length of the per-segment hypothesis lists (fresh + inverse) */
    uint32_t support_words;/* phase B: supporting (hypothesis, supporter) pairs = edges of the sparse form */
    uint32_t tied_rows;    /* phase A: source rows with equal overlaps, replayed in the reference's priority_queue order
                            * (cumulative since l3d_create) */
    uint32_t chain_sweeps; /* phase B: sweeps of the chain fixed point that still changed something (last round) */
    uint32_t chain_extra_rounds; /* phase B: extra rounds of chain sweeps beyond the ones enqueued blindly (0 normally) */
    uint32_t pool_retries; /* phase B: list passes of the last matchImages that outgrew their record pools and were repeated
                            * with larger ones (0 once the pools have the scene's size; a first call may need one) */
    float lists_ms;        /* phase B: the list pass (inverse records, candidate pairs, edges) -- the part of finish_ms that a
                            * multi-GPU run shards by views; the rest of finish_ms is the tail every rank runs */
    uint32_t record_kbytes;/* phase B: size of the four record arrays at their current pool strides, KiB: what the ranks of a
                            * multi-GPU run all-gather */
    /* round 6: what the roofline of phase B is computed from (bench.py: roofline_phase_b) */
    uint32_t list_inverse; /* phase B: of list_entries, the inverse hypotheses (storeInverseMatches, line3D.cc:1672-1699) */
    uint32_t list_candidates; /* phase B: candidate pairs the list pass handed to the exact test (similarityForScoring) */
    uint32_t list_headers; /* phase B: hypotheses with at least one supporter (headers of the sparse form) */
    uint32_t slots_lo, slots_hi; /* phase A: slots of the call = sum over directed pairs of Ms x kNN (64 bits) */
} l3d_timings;
int l3d_get_timings(l3d_ctx*, l3d_timings*);
/* How many of the context's HIP events a call records (they feed l3d_timings; the reference has no such thing: its
 * timing is the wall clock of main_*.cpp).  1 (DEFAULT since round 5: the fast setting is what a drop-in user gets): only
 * the pair around the pair-matching kernel (match_kernel_ms; the other times read 0); 2 (profiling, opt-in): all ten --
 * every field above is filled; 0: none.  An event between two kernels costs a ~6 us bubble on the stream, which a
 * 1.4 ms call notices: bench.py times the library as shipped (level 1) and takes the phase breakdown from separate
 * untimed steps at level 2. */
int l3d_set_timing_level(l3d_ctx*, int level);
/* Test hook (no reference counterpart): process-wide counters that tell a test which form of a kernel ran.
 * "csr_global_launches": launches of the global-cursor form of k_pair_csr (views beyond 32 768 segments, or
 * L3D_CSR_GLOBAL=1); "knn_replay_calls": l3d_match_begin calls whose kNN exceeded the LDS tables of the match kernel
 * (every row then takes the exact replay path); "lsd_images_detected": images LSD ran on; "lsd_cache_loads": images
 * whose segments came from the segment cache; "seam_support_wave_lists", "seam_support_group_staged_lists",
 * "seam_support_sort_only_lists", "seam_support_all_pairs_lists": lists l3d_score_matches sent down each of the four paths
 * of its support kernel (by list length; empty lists are not counted), "seam_score_unstaged_lists": lists it scored on the
 * unstaged path of the scoring kernel; "live_device_blocks", "live_pinned_blocks": blocks of device / pinned host memory
 * the library's buffers hold right now (blocks lying in its cache are not counted): equal before and after a stateless
 * call, and before l3d_create and after l3d_destroy.
 * Which forms of phase B's list pass ran (counted for the pass of a call that converged, from its flag words;
 * cumulative, tests take differences): "lists_tier2_lists", "lists_tier4_lists", "lists_huge_lists": lists the one-wave
 * tier handed to the two-wave tier, the four-wave tier and k_lists_huge; "lists_wide_passes", "lists_narrow_passes":
 * converged passes that staged 256 / 128 hypotheses per wave; "edges_global_segments": segments whose more than 512
 * candidates k_edges walked in global memory.  Passes that were REPEATED (l3d_timings.pool_retries counts them all):
 * "lists_tier_repeats": because a tier that had been left out of the launch sequence was handed a list;
 * "lists_huge_scratch_regrows": because the scratch of k_lists_huge was too small; "lists_cand_pool_regrows",
 * "lists_edge_pool_regrows": because a record pool overflowed -- the candidate (or segment-header) pools of the list
 * kernels, or only the edge / header pools of k_edges.
 * Which form a launch of the bounded-kNN pair kernel took (one count per launch of the staged kernel -- not the
 * brute-force hook, not the keep-all passes, not a call that replays every row): "match_tile_launches": the tile form,
 * 16 rows per item; "match_row2_launches": row form, two waves per item; "match_row2_cached_launches": the same with the
 * source-row cache in LDS (the launches k_order_items orders); "match_row1_launches": row form, one wave per item;
 * "match_ix32_launches": launches, of any of the four, whose LDS tables hold 32-bit indices (a target view of 65 536
 * segments or more); "match_order_launches": launches of k_order_items.  Unknown name: ~0. */
unsigned long long l3d_debug_counter(const char* name);
/* Test hook (host only, no device, no context): the form a launch of the bounded-kNN pair kernel takes and what
 * l3d_match_begin decides for the call it belongs to, computed by the functions the library itself calls.  total_items:
 * work items of the whole call (all pairs); launch_items: work items of one l3d_match_pairs range, 1 .. total_items; kNN
 * >= 1; max_target_segments: the largest target view (from 65 536 on the tables hold 32-bit indices); tile_rows: 16 = the
 * call is in the tile form, 0 = in the row form (l3d_match_tile_rows tells which, from the estimate below). */
typedef struct l3d_match_plan_info {
    uint32_t tier;             /* 0 tile form, 1 row form with two waves per item, 2 the same with the row cache, 3 one wave per item */
    uint32_t waves, row_cache, ix16;
    uint64_t lds_bytes;        /* dynamic LDS the launch asks for */
    uint32_t replay;           /* 1: l3d_match_begin sends every row of the call through the exact replay (no such launch is made) */
    uint32_t launch_accepted;  /* 0: l3d_match_pairs refuses this launch with L3D_ERR_LIMIT unless the call replays */
} l3d_match_plan_info;
int l3d_match_plan(uint64_t total_items, uint32_t launch_items, uint32_t kNN, uint32_t max_target_segments, uint32_t tile_rows,
                   l3d_match_plan_info* out);
/* ... and the form l3d_match_begin chooses for a bounded-kNN call: 16 (tile form) or 0 (row form), from est_row_items = half
 * the sum over the views of (visual neighbours x ceil(segments / 64)), rounded up.  L3D_MATCH_TILE=0|16 overrides. */
uint32_t l3d_match_tile_rows(uint64_t est_row_items);
/* Test hook (device): what every stage of a detection batch left behind.  The call makes the device work of
 * l3d_detect_segments -- the same arena, the same one launch per stage for the whole batch -- and copies out, per image,
 * the stage maps before the arena is released.  It changes nothing in the context: the segments and statistics of the
 * last detection stay.  The caller owns the buffers; with query_only != 0 nothing runs on the device and only the sizes
 * below are filled, from which the caller allocates.  Every pointer may be NULL (that map is not copied).  The input
 * checks are those of l3d_detect_segments. */
typedef struct l3d_lsd_stages {
    /* out: the geometry */
    uint32_t gw, gh;                  /* image handed to LSD (after the max-width downscale) */
    uint32_t sw, sh;                  /* after the 0.8 resample */
    uint32_t down;                    /* 1: the 8U downscale ran */
    uint32_t raw_cap;                 /* upper bound on raw_segments: what raw4 has to hold */
    /* in: host buffers */
    uint8_t* gray;                    /* rows x cols: the grey conversion */
    uint8_t* small_gray;              /* gh x gw: after the max-width downscale (== gray without it) */
    double* blur;                     /* gh x gw: the 7-tap Gaussian */
    float* deg;                       /* sh x sw: fastAtan2 degrees, -1024 where the gradient is undefined */
    double* mod;                      /* sh x sw: gradient norm */
    float* raw4;                      /* raw_cap x (x1, y1, x2, y2): LSD's output in detection order, LSD-input pixels */
    /* out: the kernel's result record */
    uint32_t raw_segments, overflow;
    uint32_t seeds, nfa_evals;
    unsigned long long max_grad_bits; /* bits of the largest defined gradient norm (0: none defined) */
    l3d_detect_stats stats;           /* as l3d_get_detect_stats reports the image, `segments` left 0 */
} l3d_lsd_stages;
int l3d_debug_lsd_stages(l3d_ctx*, uint32_t n_images, const l3d_image* images, int max_image_width, int query_only,
                         l3d_lsd_stages* out);

/* Test hook (device, read only): the records the converged list pass of the last l3d_match_images / l3d_match_finish left
 * behind -- headers, edges, segment headers of every pool (l3d_lists.h) -- and what each kernel of phase B's tail made of
 * them.  It launches nothing and writes nothing on the device; a call that never uses it makes the same
 * device calls as before.  Valid in state MATCHED (L3D_ERR_STATE otherwise) and until the next call that runs on the
 * context.  With query_only != 0 only the sizes are filled, without touching the device; the caller then allocates.  Every
 * pointer may be NULL (that array is not copied).  Records come in pool order, inside a pool in record order; a header's
 * edge_begin and the edges' edge_index are positions pool * ecap + k in the edge pools of the pass, whose strides ecap /
 * hcap / scap are those the pass ran with (the context refits its strides after every call). */
typedef struct l3d_tail_records {
    /* out: sizes */
    uint32_t G, V;                    /* 2D segments of all views, views */
    uint32_t pools, ecap, hcap, scap; /* record pools and their strides in the converged pass */
    uint32_t n_headers, n_edges, n_segs, n_surv, n_hyps, reserved;
    uint64_t n_slots;
    /* in: host buffers */
    uint32_t* seg_base;               /* V + 1: first global segment of each view */
    uint32_t* hdr_words;              /* n_headers x 16: HypHdr as it lies */
    uint32_t* hdr_pool;               /* n_headers: its pool */
    uint32_t* hdr_index;              /* n_headers: its index in the pool */
    uint8_t* hdr_positive;            /* n_headers: positive[ref] */
    uint32_t* edge_words;             /* n_edges x 4: EdgeRec as it lies */
    uint32_t* edge_index;             /* n_edges: pool * ecap + index */
    uint8_t* edge_positive;           /* n_edges: positive[ref_j] */
    uint32_t* seg_words;              /* n_segs x 4: SegHdr */
    uint32_t* max_score_bits;         /* V x 16: the replicas of each view's largest score */
    uint32_t* kept_cnt;               /* G */
    unsigned long long* best_pack;    /* G: score bits << 32 | ~canon of the best kept header */
    unsigned long long* off64s;       /* G + 1: scan of (surviving matches | best hypotheses << 32) */
    uint32_t* surv_off;               /* G + 1 */
    uint32_t* hyp_off;                /* G + 1 */
    int32_t* hyp_of_seg;              /* G */
    uint32_t* surv_sg;                /* n_surv */
    uint32_t* surv_tg;                /* n_surv */
    float* depths;                    /* 2 x n_hyps */
    float* medians;                   /* V */
} l3d_tail_records;
int l3d_debug_tail_records(l3d_ctx*, int query_only, l3d_tail_records* out);

/* Test hook (device, read only): what every stage of the affinity fill (k_affinity.hip, l3d_affinity_host.hip)
 * left behind after the last l3d_compute_affinity / l3d_affinity_shard_begin / _finish / l3d_reconstruct_3d_lines.  It
 * synchronises the stream and copies device to host; it launches nothing and writes nothing on the device.  It answers
 * L3D_ERR_STATE when no affinity step has run on the current matches, so a stale buffer is never handed out.  With
 * query_only != 0 only the sizes are filled, without touching the device; the caller then allocates.  Every pointer may
 * be NULL (that array is not copied).
 *   mode 0  the parallel path: every array up to l2g
 *   mode 1  the collinear path (collinearity_t > 0): inputs, simv, cand_*, coll_*, the child and own candidate streams
 *           (the third stream the host pass walks is the primary one: surv_off / surv_tg / simv), and the host pass's edges
 *           and l2g
 *   mode 2  between l3d_affinity_shard_begin and _finish: inputs, simv (this rank's window only) and cand_*
 * n_cand is N when the fill ran (N > 0 and H > 0) and 0 otherwise: the length of every per-candidate array; when it is 0
 * only the inputs are copied.  diffused != 0: l3d_reconstruct_3d_lines has replaced the edges on the device by the
 * diffused matrix, which is NOT the fill's output: `edges` is then left untouched. */
typedef struct l3d_affinity_records {
    /* out: sizes and scalars */
    uint32_t N, H, G, V;              /* surviving matches, best hypotheses, 2D segments of all views, views */
    uint32_t n_cand, mode, diffused;
    uint32_t n_edges, n_rows;         /* CLEdge entries (two per edge) and matrix rows; 0 in mode 2 */
    uint32_t epos_total, touch_total; /* totals of the two scans as they lie on the device (mode 0, filled by the copying call) */
    uint32_t n_coll, n_child, n_own;  /* entries of coll_idx and of the two streams (mode 1) */
    float two_sigA_sqr, med_scene_depth_lines;
    /* in: host buffers */
    float* view_k;                    /* V: View::k_ as the kernel read it */
    float* msdl_dev;                  /* 1: med_scene_depth_lines_ as the kernel read it */
    float* medians;                   /* V: the medians the kernel read */
    uint8_t* hyps;                    /* H x 128: HypRec as it lies */
    uint32_t* surv_off;               /* G + 1 */
    uint32_t* surv_sg;                /* N */
    uint32_t* surv_tg;                /* N */
    int32_t* hyp_of_seg;              /* G */
    float* simv;                      /* n_cand */
    int32_t* cand_a;                  /* n_cand */
    int32_t* cand_b;                  /* n_cand */
    uint32_t* flag;                   /* n_cand */
    uint32_t* epos;                   /* n_cand */
    uint32_t* first_touch;            /* H */
    uint32_t* touch_flag;             /* 2 n_cand + 1 */
    uint32_t* touch_rank;             /* 2 n_cand */
    l3d_cledge* edges;                /* n_edges */
    l3d_segment2d* l2g;               /* n_rows */
    uint32_t* coll_off;               /* G + 1 */
    uint32_t* coll_idx;               /* n_coll: segment index inside its view */
    uint32_t* child_off;              /* N + 1 */
    uint32_t* child_seg;              /* n_child: global segment */
    float* child_sim;                 /* n_child */
    uint32_t* own_off;                /* H + 1 */
    uint32_t* own_seg;                /* n_own: global segment */
    float* own_sim;                   /* n_own */
} l3d_affinity_records;
int l3d_debug_affinity_records(l3d_ctx*, int query_only, l3d_affinity_records* out);

/* Test hook: the layout of the RAGGED slot buffer of a keep-all call (kNN <= 0, single pass) as k_keep_pair_info and
 * k_keep_assemble left it on the device, copied out as it lies -- stream synchronisation and device-to-host copies only: no
 * kernel, nothing written on the device.  L3D_ERR_STATE unless the context's current matches are ragged (after
 * l3d_match_pairs of a keep-all call that took the single pass, until the next l3d_match_begin / l3d_match_abort).
 * Two-call form as above: query_only != 0 fills in the sizes; then the caller points the buffers at host arrays of those
 * sizes and calls again with query_only == 0.  A buffer may be NULL (that array is not copied). */
typedef struct l3d_keep_rows {
    /* out: sizes and the host's state */
    uint32_t n_rows, n_pairs;         /* source rows of all pairs of the call, pairs */
    uint32_t n_blocks;                /* blocks of 1 024 slots that hold a slot: ceil(n_slots / 1024) */
    uint32_t keep_cap;                /* records per row of the scratch, as the context keeps it for its next call */
    uint32_t tgt16, reserved;         /* the device holds inv_tgt as 16-bit entries (handed out widened) */
    uint64_t n_slots;                 /* slots of the call = what the context sizes its next call's outputs from */
    /* in: host buffers */
    uint32_t* row_start;              /* n_rows + 1: first slot of every row; [n_rows] = n_slots */
    uint32_t* row_pair;               /* n_rows: pair of a row */
    uint32_t* blk_row;                /* n_blocks: the row that holds slot 1024 b */
    uint32_t* pair_info;              /* 4 n_pairs: {first slot, longest row, slots lo, slots hi} */
    uint32_t* slot_row;               /* n_slots: source segment of a slot (row inside its pair) */
    uint32_t* inv_tgt;                /* n_slots: target segment of a slot that hands an inverse match over, 0xFFFFFFFF else */
} l3d_keep_rows;
int l3d_debug_keep_rows(l3d_ctx*, int query_only, l3d_keep_rows* out);

/* Test hook (host only, no device, no context): the epipolar-band culling set-up of one directed pair as
 * l3d_match_begin computes it -- the very function it calls.  F: the pair's fundamental matrix, row-major; ws x hs, wt x ht:
 * the source and the target image.  enabled == 0: the pair is refused and streams unculled (the forms are zero then). */
typedef struct l3d_cull_forms_info {
    uint32_t enabled, reserved;
    double As[3], Bs[3];              /* tau of the epipolar line of a source point p: (As.p) / (Bs.p) */
    double At[3], Bt[3];              /* tau of a target point q: (At.q) / (Bt.q) */
} l3d_cull_forms_info;
int l3d_cull_forms(const double F[9], double ws, double hs, double wt, double ht, l3d_cull_forms_info* out);

/* Test hook (device, read only): the tables k_cull_prepare left behind for one directed pair of the LAST launch of
 * l3d_match_pairs, copied out as they lie -- stream synchronisation and device-to-host copies only: no kernel, nothing
 * written on the device, nothing the match kernels read is changed.  The pools belong to the context and are sized by
 * l3d_match_begin; every launch of l3d_match_pairs that culls writes the regions of ITS pairs anew, and nothing after it
 * does (phase B reads the slots only).  The hook answers between that launch and l3d_match_finish / l3d_match_abort, for a
 * pair of that launch; L3D_ERR_STATE otherwise.  Two-call form: query_only != 0 fills in the sizes and the forms without
 * touching the device; then the caller points the buffers at host arrays of those sizes.  A buffer may be NULL.  A pair that
 * was not culled -- refused by make_cull, or matched by a launch that did not cull at all (brute-force hook) -- has
 * enabled == 0 and no tables: sizes 0, forms 0. */
typedef struct l3d_cull_state {
    /* out */
    uint32_t enabled;                 /* make_cull's decision for the pair (0 as well where the launch did not cull) */
    uint32_t layout_rows;             /* R of the padded class layout the launch laid the source rows out in: 16 (tile form),
                                         64 (row form); 0: the unpadded layout of the keep-all passes */
    uint32_t Ms, Mt;
    uint32_t src_len;                 /* positions of the pair's source region: Ms, or tile_src_cap(Ms, R) */
    uint32_t n_chunks;                /* ceil(Mt / 64) */
    double As[3], Bs[3], At[3], Bt[3];
    /* in: host buffers */
    uint32_t* src_perm;               /* src_len: source row at a position, 0xFFFFFFFF = padding */
    float* src_band;                  /* 2 src_len: (lo, hi) of that row */
    uint32_t* tgt_perm;               /* Mt: target segment at a sorted position */
    float* tgt_band;                  /* 2 Mt */
    float* chunk_band;                /* 2 n_chunks: hull of every 64 consecutive targets */
} l3d_cull_state;
int l3d_debug_cull(l3d_ctx*, uint32_t pair, int query_only, l3d_cull_state* out);

/* ---- (2) seam layer ------------------------------------------------------------------ */

/* Replaces match_lines_GPU (cudawrapper.h:54-63; caller Line3D::matchingGPU line3D.cc:1040-1074)
 * with CPU-path semantics (Line3D::matchingCPU line3D.cc:900-1015).  Host pointers in and out.
 * F, RtKinv_* are row-major 3x3 doubles, C_* camera centres (already translated, line3D.cc:436).
 * kNN must be > 0 here.  out_slots: Ms x kNN slots, every row in the order Line3D::matchingCPU appends it to
 * matches_[src][r] (descending overlap; equal overlaps in the pop order of its std::priority_queue).
 * Returns the number of matches in *num_matches. */
int l3d_match_lines(int device, const float* lines_src4, uint32_t Ms, const float* lines_tgt4, uint32_t Mt,
                    const double F[9], const double RtKinv_src[9], const double RtKinv_tgt[9],
                    const double C_src[3], const double C_tgt[3], uint32_t width, uint32_t height,
                    float epi_overlap, int32_t kNN, l3d_slot* out_slots, uint64_t* num_matches);

/* Line3D::createOutputFilename (line3D.cc:2853-2893): "Line3D++__W_FULL__N_10__sigmaP_2.5__..._vis_3" from the
 * parameters of the last matchImages / reconstruct3Dlines.  max_image_width <= 0 -> "W_FULL". */
int l3d_output_filename(l3d_ctx*, int max_image_width, char* buf, uint32_t cap);
/* Line3D::save3DLinesAsTXT (line3D.cc:2631-2688): <output_folder>/<output filename>.txt, one line per 3D line:
 * n_segments (P1 P2)* n_residuals (camID segID x1 y1 x2 y2)*, the format of the .txt files under testdata/Line3D++_ref. */
int l3d_save_3d_lines_txt(l3d_ctx*, const char* output_folder, int max_image_width);
/* Line3D::save3DLinesAsBIN (line3D.cc:2690-2711): <output filename>.bin = boost::archive::binary_oarchive of
 * std::vector<FinalLine3D> (serialization.h:38-45, segment3D.h:99-178), written without Boost in the byte layout of
 * the reference's own fixtures testdata/Line3D++_ref/\*vis_3.bin (doubles: the only result file that keeps full precision). */
int l3d_save_3d_lines_bin(l3d_ctx*, const char* output_folder, int max_image_width);
/* Line3D::getSegmentCoords2D (line3D.cc:2757-2772): (x1,y1,x2,y2) of a 2D segment, zeros if unknown */
int l3d_get_segment_coords2d(l3d_ctx*, uint32_t camID, uint32_t segID, float coords[4]);
/* Line3D::saveResultAsSTL (line3D.cc:2465-2531) and saveResultAsOBJ (:2579-2628): <output filename>.stl / .obj */
int l3d_save_result_stl(l3d_ctx*, const char* output_folder, int max_image_width);
int l3d_save_result_obj(l3d_ctx*, const char* output_folder, int max_image_width);

/* Replaces score_matches_GPU (cudawrapper.h:70-73; caller Line3D::scoringGPU, line3D.cc:1297-1414) with the
 * semantics of Line3D::scoringCPU (line3D.cc:1208-1294): score3D of every match of one view.  Host pointers,
 * arrays as scoringGPU marshals them: matches4[n] = (src segment, target camera, depth_p1, depth_p2), grouped per
 * segment and by target camera inside a segment (sortMatches); ranges2[M] = (first, last) inclusive, (-1,-1) if
 * none; reg_tgt2[n] = View::regularizerFrom3Dpoint of the two 3D end points in the target view; k = View::k().
 * The ranges have to partition the matches in segment order, every match inside the range of segment s has to name s as
 * its source segment (matches4[i].x == s exactly), and every target camera has to be a finite, non-negative integer value
 * below 2^32: anything else returns L3D_ERR_ARG with a message that names the first offending match, before any device
 * work, and leaves `scores` untouched. */
int l3d_score_matches(int device, const float* lines4, uint32_t M, const float* matches4, const int32_t* ranges2,
                      const float* reg_tgt2, uint32_t n, const double RtKinv[9], const double C[3], float two_sigA_sqr,
                      float k, float* scores);

/* Replaces the body of View::findCollinGPU (view.cc:173-209; find_collinear_segments_GPU, cudawrapper.h:66-68) with
 * the semantics of View::findCollinCPU (view.cc:213-258).  Host pointers.  CSR output: offsets[M+1] and, if
 * cap >= *n, idx[*n] (ascending lists; call with idx = NULL first to learn *n). */
int l3d_find_collinear_segments(int device, const float* lines4, uint32_t M, float dist_t, uint32_t* offsets,
                                uint32_t* idx, uint64_t cap, uint64_t* n);

/* Replaces the body of Line3D::performRDD (line3D.cc:2026-2076): SparseMatrix(A_, n) +
 * replicator_dynamics_diffusion_GPU (cudawrapper.h:74-75, cudawrapper.cu:708-766: row normalisation + 10
 * diffusion steps P' = P o (P W)^T with the reference's lockstep row/column walk) + the min(w12, w21)
 * symmetrisation.  Host pointers in and out; `edges` in any order with ids < n_rows; `out` receives n_edges
 * CLEdges in (i, j) ascending order (the order performRDD rebuilds A_ in).  The pattern has to be symmetric, as A_
 * always is: an edge (i, j) without (j, i) returns L3D_ERR_ARG before any device work (the reference reads out of
 * bounds on such input when a row is left empty, and otherwise returns more entries than it was given).
 * iterations = L3D_DEF_RDD_MAX_ITER (10) in the reference.  l3d_reconstruct_3d_lines(perform_diffusion != 0) runs the same kernels on the context's
 * device-resident affinity matrix. */
int l3d_diffuse_affinity(int device, const l3d_cledge* edges, uint32_t n_edges, uint32_t n_rows, uint32_t iterations,
                         l3d_cledge* out);

/* ---- projection of the 3D lines into cameras (GPU: k_project.hip) ---------------------------------------
 * No reference counterpart: the reference's only projection is the file-local helper of filterTinySegments
 * (line3D.cc:2414-2452).  Three stages, each a function of the one before it alone: 2D segments clipped at the near
 * plane and at the image rectangle; a line-id plane and an inverse-depth plane per camera; the lines drawn over an image.
 * A pinhole camera without distortion: x ~ K (R X + t), row-major K and R, the image is width x height pixels. */
typedef struct l3d_camera {
    double K[9], R[9], t[3];
    uint32_t width, height;
} l3d_camera;
/* one visible 3D segment in one camera (32 bytes): end points in pixels, 1 / depth at both, the index of its 3D line and
 * its own index in the flat segment array.  The two top bits of `segment` are flags: L3D_PROJ_CLIPPED_NEAR (bit 31) = an
 * end point was moved onto the near plane, L3D_PROJ_CLIPPED_RECT (bit 30) = an end point was moved onto the border of
 * the image; `segment & L3D_PROJ_SEGMENT_MASK` is the index. */
typedef struct l3d_projected_segment {
    float x1, y1, x2, y2;
    float inv_depth1, inv_depth2;
    uint32_t line;
    uint32_t segment;
} l3d_projected_segment;
#define L3D_PROJ_CLIPPED_NEAR 0x80000000u
#define L3D_PROJ_CLIPPED_RECT 0x40000000u
#define L3D_PROJ_SEGMENT_MASK 0x3FFFFFFFu
/* Argument checks of every entry below, L3D_ERR_ARG with a message and the outputs untouched: near <= 0 or not finite; an
 * even or zero thickness; alpha > 255; a camera with a zero side or a non-finite entry; a non-finite 3D end point or
 * record; an image whose size differs from its camera's (or that is not 8-bit with 1 or 3 channels); a null pointer where
 * one is needed.  L3D_ERR_LIMIT likewise: more than 2^30 segments, a line index of 2^31 or more, a thickness beyond 255,
 * a camera or image side of more than 65535 pixels.  A (camera, segment) whose projection is not finite in float32 (a K
 * whose third row gives 0 there, an overflow) is not visible.  Zero cameras or zero segments: L3D_OK, counts zeroed,
 * planes empty (-1 / 0), images copied.  Host pointers in and out. */
/* Stage 1.  segments[n_segments]: P1 and P2 are read (world frame, as l3d_get_3d_lines returns them); line_of_segment[i] =
 * the 3D line of segment i.  counts[n_cams] = visible segments per camera; their records camera after camera, in
 * ascending segment order inside a camera, to out (may be NULL or shorter: the first `cap` are written); *n = their
 * number over all cameras. */
int l3d_project_segments(int device, uint32_t n_cams, const l3d_camera* cams, uint32_t n_segments,
                         const l3d_segment3d* segments, const uint32_t* line_of_segment, double near_plane,
                         uint32_t* counts, l3d_projected_segment* out, uint64_t cap, uint64_t* n);
/* Stage 2.  records: n_records_per_cam[c] records of camera c, camera after camera (of the cameras only width and height
 * are read).  line_id_planes[c]: height x width int32, the line drawn at a pixel or -1; inv_depth_planes[c] (the array or
 * single entries may be NULL): height x width float, its 1 / depth there or 0.  Where lines cross the nearest wins, of
 * equal depths the smaller line index; thickness = odd number of pixels across the line. */
int l3d_render_line_maps(int device, uint32_t n_cams, const l3d_camera* cams, const uint32_t* n_records_per_cam,
                         const l3d_projected_segment* records, uint32_t thickness, int32_t* const* line_id_planes,
                         float* const* inv_depth_planes);
/* Stage 3.  images[c]: 8-bit, 1 or 3 channels, of the size of line_id_planes[c] (row_stride >= cols * channels);
 * out_rgb[c] receives rows x cols x 3 bytes, packed.  Where line_id >= 0 the pixel is blended with the line's colour,
 * (alpha * colour + (255 - alpha) * source + 127) / 255; elsewhere it is copied.  colors: n_lines RGB triples, or NULL
 * for the fixed palette of DESIGN §16 (which a line index >= n_lines takes as well). */
int l3d_draw_line_maps(int device, uint32_t n_cams, const l3d_image* images, const int32_t* const* line_id_planes,
                       uint32_t n_lines, const uint8_t* colors, uint32_t alpha, uint8_t* const* out_rgb);
/* The same over the lines the last l3d_reconstruct_3d_lines left in the context (none: L3D_ERR_STATE); `line` is the index
 * of the FinalLine3D in l3d_get_3d_lines' order, `segment` the index in its flat segment array.
 * l3d_view_camera: K, R, t and the image size of an added view (original frame), ready for the calls below.  t is the
 * view's own: after matchImages it is -R C of a centre that was moved by the scene translation and back
 * (line3D.cc:500-545), a few roundings from the t handed to addImage.  L3D_ERR_STATE while a split call is open. */
int l3d_view_camera(l3d_ctx*, uint32_t camID, l3d_camera* cam);
int l3d_project_lines(l3d_ctx*, uint32_t n_cams, const l3d_camera* cams, double near_plane, uint32_t* counts);
/* records of the last l3d_project_lines on this context, as l3d_project_segments hands them out */
int l3d_get_projected_lines(l3d_ctx*, l3d_projected_segment* out, uint64_t cap, uint64_t* n);
int l3d_render_lines(l3d_ctx*, uint32_t n_cams, const l3d_camera* cams, double near_plane, uint32_t thickness,
                     int32_t* const* line_id_planes, float* const* inv_depth_planes);
/* l3d_draw_lines: colors is NULL (the palette) or holds one RGB triple for EVERY 3D line of the context, n_lines of
 * l3d_num_3d_lines: the entry is not given the table's length and reads 3 * n_lines bytes. */
int l3d_draw_lines(l3d_ctx*, uint32_t n_cams, const l3d_camera* cams, const l3d_image* images, double near_plane,
                   uint32_t thickness, uint32_t alpha, const uint8_t* colors, uint8_t* const* out_rgb);
/* test hook: the device-memory budget under which the context forms above cut the cameras into groups (0: the default of
 * 256 MiB); a small one makes many groups.  The results do not depend on it. */
int l3d_set_projection_budget(l3d_ctx*, uint64_t bytes);

/* ---- the 2D segments that support each 3D line (GPU: k_associate.hip) ------------------------------------
 * No reference counterpart.  The way back from an image to the model: every 2D segment of a camera is tested against
 * every record of that camera (l3d_projected_segment, as stage 1 above hands them out) and assigned the record it
 * observes.  A pair (segment, record) is accepted iff the record is at least a pixel long, the segment is not a point,
 * both end points of the segment lie within max_distance pixels of the record's line, the angle between the two is at
 * most the one whose squared cosine is min_cos2, and at least min_overlap of the segment lies within the record's
 * extent.  Of the accepted records the segment is assigned the one with the smallest distance (the larger of its two
 * end points' distances), of equal distances the one with the smaller index.  fp64, the contract of DESIGN §17. */
typedef struct l3d_associate_params {
    double max_distance;   /* pixels, finite, >= 0 */
    double min_cos2;       /* in [0, 1]: cos^2 of the largest angle between segment and record */
    double min_overlap;    /* in [0, 1]: share of the 2D segment inside the record's extent */
} l3d_associate_params;
/* the result for one 2D segment (24 bytes) */
typedef struct l3d_association {
    int32_t record;        /* index among its camera's records, -1: none accepted */
    uint32_t line;         /* the record's line (0xFFFFFFFF: none) */
    uint32_t segment;      /* the record's segment & L3D_PROJ_SEGMENT_MASK (0xFFFFFFFF: none) */
    float distance;        /* pixels: the larger distance of the segment's end points from the record's line (0: none) */
    float overlap;         /* share of the 2D segment inside the record's extent (0: none) */
    uint32_t n_accepted;   /* accepted records; more than 1 marks an ambiguous segment */
} l3d_association;
/* Argument checks of both entries, the outputs untouched: L3D_ERR_ARG for a null pointer where one is needed, a
 * non-finite record or segment (the message names camera and index), max_distance negative or not finite, min_cos2 or
 * min_overlap outside [0, 1] or NaN; L3D_ERR_LIMIT for 2^31 or more records in a camera or 2^32 or more segments in
 * total.  Cameras are taken in groups under the budget of l3d_set_projection_budget; the results do not depend on it.
 * Stateless, host pointers: n_records_per_cam[c] records of camera c in `records`, camera after camera;
 * n_segments_per_cam[c] segments (x1, y1, x2, y2) of camera c in segs4, camera after camera; out: one l3d_association
 * per segment in the same order.  Zero cameras, records or segments: L3D_OK, every output "none". */
int l3d_associate_segments(int device, uint32_t n_cams, const uint32_t* n_records_per_cam,
                           const l3d_projected_segment* records, const uint32_t* n_segments_per_cam, const float* segs4,
                           const l3d_associate_params* params, l3d_association* out);
/* The same for added views (camIDs, each once) and the lines the last l3d_reconstruct_3d_lines left in the context: the
 * lines are projected into the views' own cameras (l3d_view_camera, as l3d_project_lines does: l3d_get_projected_lines
 * returns these records afterwards) and every view's own segments -- the coordinates of l3d_get_segment_coords2d, segID
 * = index -- are associated.  offsets[n_views + 1]: where every view's results begin in out; out may be NULL: the offsets
 * only, and nothing runs.  support_segments / support_views (n_lines of l3d_num_3d_lines each, may be NULL): per 3D line
 * the number of assigned (view, segment) pairs and the number of distinct views among them.  L3D_ERR_STATE without
 * reconstructed lines or while a split call is open; an unknown camID or one named twice: L3D_ERR_ARG. */
int l3d_associate_view_segments(l3d_ctx*, uint32_t n_views, const uint32_t* camIDs, const l3d_associate_params* params,
                                double near_plane, uint64_t* offsets, l3d_association* out, uint32_t* support_segments,
                                uint32_t* support_views);

/* ---- two 3D line models compared segment by segment, in both directions (GPU: k_compare.hip) ------------
 * No reference counterpart.  A model is a flat array of 3D segments (P1, P2: 6 doubles each, world frame) with a line
 * index per segment.  A pair (query q, reference r) is accepted iff neither is a point, the angle between them is at
 * most the one whose squared cosine is min_cos2, both end points of q lie within max_distance of r's line, and at least
 * min_overlap of q lies within r's extent; with exclude_same_line, iff also line(q) != line(r).  Of the accepted
 * references a query gets the one with the smallest distance (the larger of its two end points' distances), of equal
 * distances the one with the smaller index.  fp64, the contract of DESIGN §18.  The caller aligns the models: no
 * similarity transform is estimated here -- l3d_align_segments / l3d_align_lines below estimate one and
 * deliver the comparison of the aligned models. */
typedef struct l3d_compare_params {
    double max_distance;         /* model units, finite, >= 0: a 3D model has no natural unit, so there is no default */
    double min_cos2;             /* in [0, 1]: cos^2 of the largest angle between query and reference */
    double min_overlap;          /* in [0, 1]: share of the query inside the reference's extent */
    uint32_t exclude_same_line;  /* 0 or 1; 1: pairs of the same line index are not accepted (a model against itself:
                                    its near-duplicate lines) */
    uint32_t slice_chunks;       /* 0: the library chooses; else chunks of 256 references per slice.  A tuning knob and
                                    test hook: no output depends on it */
} l3d_compare_params;
/* the result for one query segment (24 bytes) */
typedef struct l3d_line_match {
    int32_t segment;       /* index of the reference segment, -1: none accepted */
    uint32_t line;         /* the reference's line (0xFFFFFFFF: none) */
    uint32_t n_accepted;   /* accepted references; more than 1 marks an ambiguous segment */
    float overlap;         /* share of the query inside the reference's extent (0: none) */
    double distance;       /* the larger distance of the query's end points from the reference's line (0: none) */
} l3d_line_match;
/* one direction summed up (56 bytes); the lengths are added sequentially in ascending index order */
typedef struct l3d_compare_summary {
    uint64_t n_segments;       /* queries */
    uint64_t n_matched;        /* ... with a reference */
    uint64_t n_ambiguous;      /* ... with n_accepted > 1 */
    uint64_t n_lines;          /* distinct line indices among the queries */
    uint64_t n_lines_matched;  /* ... with at least one matched segment */
    double length_total;       /* sum of the queries' lengths */
    double length_matched;     /* ... of the matched ones */
} l3d_compare_summary;
/* Stateless, host pointers.  q_segs6 [n_q x 6], q_line [n_q]; r_segs6, r_line alike.  out_q [n_q]: every segment of Q
 * against R; out_r [n_r]: every segment of R against Q; either may be NULL, and that direction is skipped together with
 * its summary.  summary_q / summary_r may be NULL.  One upload, one launch (pair) and one download per direction.
 * Checked before any device work, the outputs untouched: L3D_ERR_LIMIT for 2^30 or more segments on a side; L3D_ERR_ARG
 * for a null pointer where one is needed, a coordinate that is not finite or beyond 2^100 in magnitude (the message
 * names the side and the segment), max_distance negative or not finite, min_cos2 or min_overlap outside [0, 1] or NaN,
 * exclude_same_line > 1.  Zero segments on either side: L3D_OK, every record "none" and both summaries all zero: nothing was
 * compared. */
int l3d_compare_segments(int device, uint32_t n_q, const double* q_segs6, const uint32_t* q_line, uint32_t n_r,
                         const double* r_segs6, const uint32_t* r_line, const l3d_compare_params* params,
                         l3d_line_match* out_q, l3d_line_match* out_r, l3d_compare_summary* summary_q,
                         l3d_compare_summary* summary_r);
/* The same with the context's side = the flat collinear segments of the last l3d_reconstruct_3d_lines, in the order
 * and coordinates l3d_get_3d_lines returns them (n_segments of l3d_num_3d_lines; the line of a segment is the index of
 * its 3D line): out_mine [n_segments], out_other [n_other].  On the context's stream.  L3D_ERR_STATE without
 * reconstructed lines or while a split call is open. */
int l3d_compare_lines(l3d_ctx*, uint32_t n_other, const double* other_segs6, const uint32_t* other_line,
                      const l3d_compare_params* params, l3d_line_match* out_mine, l3d_line_match* out_other,
                      l3d_compare_summary* summary_mine, l3d_compare_summary* summary_other);

/* ---- near-duplicate 3D lines merged (GPU: k_merge.hip) ----------------------------------------------------
 * No reference counterpart.  One model as above: a flat array of 3D segments with a line index per segment (any values,
 * not only dense ones).  An ordered pair of segments (q, r) is accepted iff line(q) != line(r) and the pair test of
 * l3d_compare_segments accepts it with q as the query and r as the reference; one direction suffices.  Lines joined by
 * accepted pairs, directly or through a chain of them, form a component; a component of two or more lines becomes one
 * line: its live segments are projected onto a common carrier (through their length-weighted centroid, along the sum of
 * their directions) and intervals that touch or overlap are fused.  A line in no accepted pair keeps its segments
 * unchanged.  Output lines are numbered 0, 1, ... by the smallest input line index they hold.  fp64, the contract of
 * DESIGN §19. */
typedef struct l3d_merge_params {
    double max_distance;         /* as in l3d_compare_params */
    double min_cos2;
    double min_overlap;
    uint32_t slice_chunks;       /* 0: the library chooses; else chunks of 256 references per slice.  No output depends on it */
    uint32_t reserved;           /* must be 0 */
} l3d_merge_params;
/* one output line (16 bytes) */
typedef struct l3d_merge_line_info {
    uint32_t n_members;          /* input lines fused into this one; 1: an untouched line */
    uint32_t label;              /* the smallest input line index among them */
    double max_offset;           /* the largest distance of a member's end point from the fused carrier; 0 for an untouched
                                    line.  Components form by chaining: this is how a caller sees a chain that went far */
} l3d_merge_line_info;
/* (80 bytes); the lengths are added sequentially in ascending index order */
typedef struct l3d_merge_summary {
    uint64_t n_segments_in, n_segments_out;
    uint64_t n_lines_in, n_lines_out;
    uint64_t n_pairs;                /* accepted ordered pairs of segments */
    uint64_t n_merged_components;    /* output lines with n_members >= 2 */
    uint64_t largest_component;      /* the largest n_members (0: an empty model) */
    double length_in, length_out;
    double max_offset;               /* the largest of the lines' */
} l3d_merge_summary;
/* Stateless, host pointers.  segs6 [n x 6], line [n].  out_line_map [n]: the output line of every input segment (also of
 * a point segment that a fused line dropped).  out_segs6 [out_seg_cap x 6], out_seg_line [out_seg_cap]: the output
 * segments, line after line, and the output line of each; *out_n_segs <= n.  out_line_info [out_line_cap]; *out_n_lines
 * <= the number of distinct line indices, which is <= n: capacities of n are always enough.  summary may be NULL.
 * Checked before any device work, the outputs untouched: L3D_ERR_LIMIT for 2^30 or more segments; L3D_ERR_ARG for a null
 * pointer, a coordinate that is not finite or beyond 2^100 (the message names the segment), a threshold outside its
 * range, reserved != 0, out_seg_cap < n or out_line_cap < the number of distinct line indices.  More than 2^28 accepted
 * pairs: L3D_ERR_LIMIT, found after the count pass, the outputs untouched.  n = 0: L3D_OK, a summary of zeros. */
int l3d_merge_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_merge_params* params,
                       uint32_t* out_line_map, uint32_t out_seg_cap, double* out_segs6, uint32_t* out_seg_line,
                       uint32_t* out_n_segs, uint32_t out_line_cap, l3d_merge_line_info* out_line_info, uint32_t* out_n_lines,
                       l3d_merge_summary* summary);
/* The same on the context's lines (flattened as for l3d_compare_lines), which the result REPLACES: l3d_num_3d_lines,
 * l3d_get_3d_lines, the writers and the projection, association and comparison stages see the merged model.  An
 * untouched line keeps every field.  A fused line gets the fused segments (direction, length and validity as for any 3D
 * segment), the carrier from its first to its last fused end point as the cluster's segment, the residuals of its members
 * concatenated in ascending line index, and the reference view of the line of its longest member segment.  The records
 * of the last l3d_project_lines are dropped.  l3d_output_filename carries MERGED_<max_distance>__ in front of vis_ until
 * the next l3d_reconstruct_3d_lines.  L3D_ERR_STATE without reconstructed lines or while a split call is open. */
int l3d_merge_lines(l3d_ctx*, const l3d_merge_params* params, l3d_merge_summary* summary);

/* ---- two 3D line models aligned: the similarity transform between them (GPU: k_align.hip) ---------------
 * No reference counterpart.  Two models as above, Q (moved) and R (fixed), in frames that differ by a similarity
 * transform y = scale * R(q) x + t.  Iterated closest lines: per iteration Q is transformed, matched against R by the
 * pair test of l3d_compare_segments (within `gate`, which starts at start_distance, halves per iteration and ends at
 * max_distance), the 7x7 normal equations of the matched end points' distances from their reference lines are summed on
 * the device and solved on the host, and the transform is updated about the centre of R's bounding box.  fp64, the
 * contract of DESIGN §23.  A start within reach is the caller's: NULL means identity. */
typedef struct l3d_similarity {     /* 64 bytes */
    double scale;                /* finite, > 0 */
    double q[4];                 /* rotation as a quaternion (w, x, y, z); q.q finite and > 0, normalised on entry */
    double t[3];                 /* finite */
} l3d_similarity;
typedef struct l3d_align_params {   /* 64 bytes */
    double max_distance;         /* as in l3d_compare_params: the gate of the last iterations and of the delivered comparison */
    double min_cos2;
    double min_overlap;
    double start_distance;       /* 0: the gate is max_distance throughout; else finite and >= max_distance */
    double step_tolerance;       /* finite, > 0: converged when the gate is max_distance and the step is at most this */
    uint32_t max_iterations;     /* 1 .. 256 */
    uint32_t min_matches;        /* >= 1: fewer matched queries stop the iteration (L3D_ALIGN_TOO_FEW) */
    uint32_t estimate_scale;     /* 0 or 1; 0: the scale stays the initial one */
    uint32_t slice_chunks;       /* as in l3d_compare_params: no output depends on it */
    uint32_t reserved[2];        /* must be 0 */
} l3d_align_params;
enum { L3D_ALIGN_CONVERGED = 0, L3D_ALIGN_MAX_ITERATIONS = 1, L3D_ALIGN_TOO_FEW = 2, L3D_ALIGN_DEGENERATE = 3 };
typedef struct l3d_align_summary {  /* 64 bytes */
    uint32_t status;             /* L3D_ALIGN_* */
    uint32_t iterations;         /* iterations run = trace entries written (one that stopped without an update included) */
    uint64_t n_matched;          /* queries matched at max_distance under the final transform */
    double rms;                  /* sqrt(cost / (2 n_matched)) of them: the end points' distance from their reference lines */
    double last_step;            /* the step of the last update (0: none was made) */
    double diag;                 /* the diagonal of R's bounding box */
    double center[3];            /* its midpoint, about which the updates rotate and scale */
} l3d_align_summary;
/* one iteration (432 bytes).  sums: H (28, the upper triangle row by row), b (7), cost, count. */
typedef struct l3d_align_iteration {
    double gate;
    double sums[37];
    double delta[7];             /* rotation (3), scale, translation (3); all 0 where the iteration stopped without a solve */
    l3d_similarity similarity;   /* after the update (unchanged where none was made) */
    uint64_t n_matched;
} l3d_align_iteration;
/* Stateless, host pointers.  Both models are uploaded once; per iteration the transform, the comparison's launches and the
 * normal kernel run, 37 doubles per tile of 256 queries come down and the host solves.  Then the delivery pass: Q under
 * the final transform compared with R at max_distance (out_q [n_q]) and, with out_r [n_r], R with it.  initial: NULL =
 * identity.  out_similarity and summary are required; out_segs6 [n_q x 6] (the transformed Q), out_q, out_r and trace
 * [max_iterations] may be NULL.  Everything is written after all has run and stays untouched on any error.  Checked
 * before any device work: L3D_ERR_LIMIT for 2^30 or more segments on a side; L3D_ERR_ARG for a null pointer where one is
 * needed, a coordinate not finite or beyond 2^100, a threshold outside its range, start_distance below max_distance or
 * not finite, step_tolerance not finite or not > 0, max_iterations outside 1..256, min_matches 0, estimate_scale > 1,
 * reserved != 0, an initial similarity that is not finite or has scale <= 0 or a zero quaternion, and R's bounding box a
 * point.  An empty Q or R: L3D_OK, status L3D_ALIGN_TOO_FEW, the initial transform returned, zero iterations. */
int l3d_align_segments(int device, uint32_t n_q, const double* q_segs6, const uint32_t* q_line, uint32_t n_r,
                       const double* r_segs6, const uint32_t* r_line, const l3d_align_params* params,
                       const l3d_similarity* initial, l3d_similarity* out_similarity, l3d_align_summary* summary,
                       double* out_segs6, l3d_line_match* out_q, l3d_line_match* out_r, l3d_align_iteration* trace);
/* The same with Q = the context's lines, flattened as for l3d_compare_lines, aligned to the model `other` as R; on the
 * context's stream.  The context is NOT modified: out_segs6 receives the moved copy.  L3D_ERR_STATE without reconstructed
 * lines or while a split call is open. */
int l3d_align_lines(l3d_ctx*, uint32_t n_other, const double* other_segs6, const uint32_t* other_line,
                    const l3d_align_params* params, const l3d_similarity* initial, l3d_similarity* out_similarity,
                    l3d_align_summary* summary, double* out_segs6, l3d_line_match* out_mine, l3d_line_match* out_other,
                    l3d_align_iteration* trace);
/* Host only: out_segs6 [n x 6] = the similarity applied to both end points of every segment -- its quaternion divided by
 * its norm first, as every pass of the calls above applies one -- by the function the device runs: bit-equal to out_segs6
 * of an alignment that returned this similarity.  L3D_ERR_ARG for a null pointer or a similarity as refused above. */
int l3d_transform_segments(uint32_t n, const double* segs6, const l3d_similarity* similarity, double* out_segs6);

/* ---- camera poses refined against the 3D line model (GPU: k_pose.hip) ------------------------------------
 * No reference counterpart (its bundle adjustment holds every camera constant).  Given a model as above and, per camera,
 * an approximate pose (l3d_camera: K stays fixed and must be upper triangular with K22 = 1) and the camera's 2D segments,
 * every camera is refined on its own by iterated closest lines: per iteration the model is projected (stage 1 of the
 * projection, unchanged), the segments are associated with the records (l3d_associate_segments' kernel, unchanged, within
 * `gate` pixels), the 6x6 normal equations of the end points' distances from the image lines of their 3D segments are
 * summed on the device and solved on the host, and the pose is updated.  The gate starts at max(max_distance,
 * start_distance) and halves, down to max_distance, whenever the step falls to stall_tolerance.  fp64, the contract of
 * DESIGN §27.  A start within reach is the caller's. */
typedef struct l3d_pose_params {    /* 72 bytes */
    double max_distance;         /* as in l3d_associate_params: the gate of the last iterations and of the delivery pass */
    double min_cos2;
    double min_overlap;
    double start_distance;       /* 0: the gate is max_distance throughout; else finite and >= max_distance (pixels) */
    double stall_tolerance;      /* finite, > 0: the gate halves after an iteration whose step is at most this */
    double step_tolerance;       /* finite, > 0: converged when the gate is max_distance and the step is at most this */
    double near_plane;           /* finite, > 0: of the projection */
    uint32_t max_iterations;     /* 1 .. 256 */
    uint32_t min_matches;        /* >= 6: fewer matched segments stop the camera (L3D_POSE_TOO_FEW) */
    uint32_t reserved[2];        /* must be 0 */
} l3d_pose_params;
enum { L3D_POSE_CONVERGED = 0, L3D_POSE_MAX_ITERATIONS = 1, L3D_POSE_TOO_FEW = 2, L3D_POSE_DEGENERATE = 3 };
typedef struct l3d_pose_summary {   /* 88 bytes */
    uint32_t status;             /* L3D_POSE_* */
    uint32_t iterations;         /* iterations run = trace entries written (one that stopped without an update included) */
    uint64_t n_matched;          /* segments that entered the sums of the delivery pass: matched at max_distance under the final pose */
    double rms;                  /* sqrt(cost / (2 n_matched)) of them, pixels: the end points' distance from the image lines */
    double last_step;            /* the step of the last update (0: none was made) */
    double q[4];                 /* the rotation of the delta on the input pose (w, x, y, z): R = R(q) R_in */
    double t[3];                 /* its shift, in the frame about the model's centre: t' = R(q) t'_in + this */
} l3d_pose_summary;
/* one iteration of one camera (392 bytes).  sums: H (21, the upper triangle row by row), b (6), cost, count. */
typedef struct l3d_pose_iteration {
    double gate;
    double sums[29];
    double delta[6];             /* rotation (3), translation (3); all 0 where the iteration stopped without a solve */
    double R[9], t[3];           /* the pose after the update (the camera as given where none has been made yet) */
    uint64_t n_matched;
} l3d_pose_iteration;
/* Stateless, host pointers.  segs6 / line: the model, n_segments x (P1, P2) with a line index each.  cams [n_cams];
 * n_segments_per_cam[c] 2D segments (x1, y1, x2, y2) of camera c in segs4, camera after camera.  out_cams [n_cams] and
 * summaries [n_cams] are required; out_assoc (one l3d_association per 2D segment: what l3d_project_segments and
 * l3d_associate_segments return for out_cams at max_distance) and trace [n_cams x max_iterations] (camera c's entries
 * from c x max_iterations on) may be NULL.  Every camera is refined independently of the others in the call; a camera that
 * is never updated comes back bit for bit.  Everything is written after all has run and stays untouched on any error.
 * Checked before any device work: L3D_ERR_LIMIT for 2^30 or more model segments, 2^32 or more 2D segments or a camera side
 * beyond 65535; L3D_ERR_ARG for a null pointer where one is needed, a coordinate not finite or beyond 2^100, a 2D segment
 * or a camera with a non-finite entry or a side of zero pixels, a K that is not upper triangular with K22 = 1 and K00,
 * K11 != 0, a threshold outside its range, start_distance below max_distance or not finite, stall_tolerance or
 * step_tolerance not finite or not > 0, max_iterations outside 1..256, min_matches below 6, a near plane not finite or
 * not > 0, reserved != 0, and the model's bounding box a point.  An empty model, zero cameras or a camera without
 * segments: L3D_OK, status L3D_POSE_TOO_FEW, the camera returned as given, zero iterations. */
int l3d_refine_cameras(int device, uint32_t n_segments, const double* segs6, const uint32_t* line, uint32_t n_cams,
                       const l3d_camera* cams, const uint32_t* n_segments_per_cam, const float* segs4,
                       const l3d_pose_params* params, l3d_camera* out_cams, l3d_pose_summary* summaries,
                       l3d_association* out_assoc, l3d_pose_iteration* trace);
/* The same for added views (camIDs, each once) against the context's lines, flattened as for l3d_compare_lines: each view's
 * own camera (l3d_view_camera) and segments, on the context's stream.  offsets [n_views + 1] (required): where every view's
 * associations begin in out_assoc.  The context is NOT modified.  L3D_ERR_STATE without reconstructed lines or while a
 * split call is open; an unknown camID or one named twice: L3D_ERR_ARG. */
int l3d_refine_view_cameras(l3d_ctx*, uint32_t n_views, const uint32_t* camIDs, const l3d_pose_params* params,
                            l3d_camera* out_cams, l3d_pose_summary* summaries, uint64_t* offsets, l3d_association* out_assoc,
                            l3d_pose_iteration* trace);

/* ---- where 3D lines meet: junctions and the wireframe graph (GPU: k_wireframe.hip) ----------------------
 * No reference counterpart.  One model as above: a flat array of 3D segments with a line index per segment (any values).
 * Two segments a < b of different lines form a junction iff neither is a point, the angle between them is at least the
 * one whose squared sine is min_sin2, their carriers come within max_distance of each other, and the point where they do
 * lies on both segments or at most max_extension beyond an end.  An end of a segment within max_extension of that point
 * is "at" the junction (L: both segments end there, T: one does, X: they cross).  Junctions that share an end of a
 * segment, or lie within max_distance of each other inside one, form one vertex; the ends that meet nothing are vertices
 * too, and every segment gives the edges between its consecutive vertices.  The model itself is not modified.  fp64, the
 * contract of DESIGN §24. */
typedef struct l3d_wireframe_params {   /* 32 bytes */
    double max_distance;         /* model units, finite, >= 0, no default: the gap between the two carriers where they come closest */
    double max_extension;        /* model units, finite, >= 0: how far beyond a segment's end the meeting point may lie, and
                                    the width of the end zone */
    double min_sin2;             /* in [0, 1]: sin^2 of the smallest angle between the two */
    uint32_t slice_chunks;       /* 0: the library chooses; else chunks of 256 references per slice.  No output depends on it */
    uint32_t reserved;           /* must be 0 */
} l3d_wireframe_params;
enum { L3D_WF_L = 1, L3D_WF_T = 2, L3D_WF_X = 4 };               /* kind of a junction; the bits of a vertex's kinds */
enum { L3D_WF_AT_P1 = 0, L3D_WF_AT_P2 = 1, L3D_WF_INTERIOR = 2 }; /* where on a segment a junction lies */
/* a junction (72 bytes), in ascending (a, b) order */
typedef struct l3d_wf_junction {
    uint32_t a, b;               /* the two segments, a < b */
    uint32_t kind;               /* L3D_WF_L, _T or _X */
    uint32_t class_a, class_b;   /* L3D_WF_AT_P1, _AT_P2 or _INTERIOR, on a and on b */
    uint32_t vertex;             /* the vertex it belongs to */
    double sa, sb;               /* the closest points of the carriers: P1 + s (P2 - P1) on a and on b */
    double gap;                  /* their distance */
    double J[3];                 /* their midpoint */
} l3d_wf_junction;
/* a vertex (48 bytes): the junction vertices, numbered by their smallest junction, then the free ends in (segment, end) order */
typedef struct l3d_wf_vertex {
    double P[3];                 /* the mean of its junctions' J; a free end: the end point itself */
    double spread;               /* the largest distance of a member's J from P.  Vertices form by chaining: this is how a
                                    caller sees one that went far */
    uint32_t n_junctions;        /* 0: a free end */
    uint32_t kinds;              /* the kinds of its junctions, or-ed */
    uint32_t degree;             /* incident edges */
    uint32_t component;          /* connected component of the graph, numbered by their smallest vertex */
} l3d_wf_vertex;
/* an edge (16 bytes): a piece of `segment` between two consecutive vertices on it, in ascending segment order */
typedef struct l3d_wf_edge { uint32_t v0, v1, segment, line; } l3d_wf_edge;
/* (120 bytes); length_total is added sequentially in ascending index order */
typedef struct l3d_wireframe_summary {
    uint64_t n_segments, n_point_segments, n_junctions;
    uint64_t n_L, n_T, n_X;
    uint64_t n_vertices, n_junction_vertices, n_free_ends;
    uint64_t n_edges, n_components;
    uint64_t largest_component;  /* in edges */
    double length_total;         /* of the segments */
    double max_gap, max_spread;
} l3d_wireframe_summary;
typedef struct l3d_wireframe l3d_wireframe;
/* Stateless, host pointers.  segs6 [n x 6], line [n].  The result is not bounded by n, so it lives in a handle: *out, to be
 * closed by l3d_wireframe_close.  Checked before any device work, *out untouched: L3D_ERR_LIMIT for 2^30 or more segments;
 * L3D_ERR_ARG for a null pointer, a coordinate that is not finite or beyond 2^100 (the message names the segment),
 * max_distance or max_extension negative or not finite, min_sin2 outside [0, 1] or NaN, reserved != 0.  More than 2^28
 * junctions: L3D_ERR_LIMIT, found after the count pass, *out untouched.  n = 0: L3D_OK, an empty graph, a summary of zeros. */
int l3d_wireframe_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_wireframe_params* params,
                           l3d_wireframe** out);
/* The same on the context's lines (flattened as for l3d_compare_lines), on the context's stream.  The context is NOT
 * modified.  L3D_ERR_STATE without reconstructed lines or while a split call is open. */
int l3d_wireframe_lines(l3d_ctx*, const l3d_wireframe_params* params, l3d_wireframe** out);
/* the sizes of the three arrays; any pointer may be NULL */
int l3d_wireframe_counts(const l3d_wireframe*, uint64_t* n_junctions, uint64_t* n_vertices, uint64_t* n_edges);
/* the arrays, of the sizes l3d_wireframe_counts states, and the summary; any pointer may be NULL */
int l3d_wireframe_get(const l3d_wireframe*, l3d_wf_junction* junctions, l3d_wf_vertex* vertices, l3d_wf_edge* edges,
                      l3d_wireframe_summary* summary);
/* "v x y z" (%.17g) per vertex in vertex order, then "l i j" (1-based) per edge in edge order.  L3D_ERR_IO where the file
 * cannot be written. */
int l3d_wireframe_save_obj(const l3d_wireframe*, const char* path);
void l3d_wireframe_close(l3d_wireframe*);

/* ---- the planes the 3D lines lie in (GPU: k_planes.hip, selection: l3d_planes.h) ------------------------------
 * No reference counterpart.  One model as above.  Every junction of §24 -- a pair of non-parallel segments that touch,
 * found with junction_distance, junction_extension and min_sin2 -- spans a plane hypothesis; every hypothesis is scored on
 * the device against every segment (a segment is an inlier iff both its end points lie within max_distance of the plane;
 * the score is the number of inliers and their length as an integer weight), and a sequential selection on the host keeps
 * the best-supported planes that are neither spanned again by two members of an accepted plane nor share more than half
 * their weight with one.  A segment may lie in several planes.  The model itself is not modified.  fp64, the contract of
 * DESIGN §25. */
typedef struct l3d_planes_params {   /* 64 bytes */
    double max_distance;         /* model units, finite, >= 0, no default: largest distance of a member's end points from the plane */
    double junction_distance;    /* §24's max_distance, for the hypotheses */
    double junction_extension;   /* §24's max_extension */
    double min_sin2;             /* in [0, 1], as in §24 */
    double min_length;           /* model units, finite, >= 0: least support (summed member length) of a plane */
    uint32_t min_segments;       /* >= 1: least number of member segments */
    uint32_t max_planes;         /* >= 1 */
    uint32_t max_tests;          /* >= 1: candidates tested against the accepted planes before the selection gives up */
    uint32_t slice_chunks;       /* 0: the library chooses; else chunks of 256 segments per slice.  No output depends on it */
    uint32_t reserved[2];        /* must be 0 */
} l3d_planes_params;
/* an accepted plane (264 bytes), in order of acceptance */
typedef struct l3d_pl_plane {
    uint32_t hypothesis;         /* its index in the junction list */
    uint32_t a, b;               /* the two segments that span it, a < b */
    uint32_t n_segments;         /* members */
    uint32_t n_lines;            /* distinct line indices among them */
    uint32_t reserved;           /* 0 */
    uint64_t weight;             /* the members' integer weights, summed: length * 2^scale_exponent, each floored */
    double N[3], J[3], d;        /* unit normal, the junction's point, d = N.J */
    double length;               /* of the members, added sequentially */
    double rms;                  /* of the members' 2 n end-point distances from (N, J) */
    double centroid[3];          /* of the members' end points */
    double N_fit[3], d_fit;      /* least-squares plane through them (N_fit.N >= 0), d_fit = N_fit.centroid */
    double rms_fit;              /* of the end-point distances from it */
    double corners[4][3];        /* a patch for display in the plane (N, J): the bounding rectangle of the members' end
                                    points along U = the direction of segment a and V = N x U */
} l3d_pl_plane;
/* a membership (8 bytes), in (plane, segment) order */
typedef struct l3d_pl_member { uint32_t plane, segment; } l3d_pl_member;
/* the score of a hypothesis (16 bytes), as the device yields it */
typedef struct l3d_pl_score { uint64_t weight; uint32_t count, reserved; } l3d_pl_score;
/* (136 bytes) */
typedef struct l3d_planes_summary {
    uint64_t n_segments, n_point_segments;
    uint64_t n_hypotheses, n_dead;          /* junctions; those whose normal has no finite, positive squared length */
    uint64_t n_candidates;                  /* live hypotheses with min_segments and min_length */
    uint64_t n_tested, n_dropped, n_rejected;
    uint64_t n_planes, n_memberships;
    uint64_t n_segments_in_planes, n_segments_in_several;
    uint64_t truncated;                     /* 1: max_tests was reached before the candidates or max_planes ran out */
    int64_t scale_exponent;                 /* weight = floor(length * 2^scale_exponent) */
    double length_total;                    /* of the segments, added sequentially */
    double length_in_planes;                /* of the segments in at least one plane, each once */
    double max_rms;
} l3d_planes_summary;
typedef struct l3d_planes l3d_planes;
/* Stateless, host pointers.  segs6 [n x 6], line [n].  The result lives in a handle: *out, to be closed by
 * l3d_planes_close.  Checked before any device work, *out untouched: L3D_ERR_LIMIT for 2^30 or more segments; L3D_ERR_ARG
 * for a null pointer, a coordinate that is not finite or beyond 2^100 (the message names the segment), max_distance,
 * junction_distance, junction_extension or min_length negative or not finite, min_sin2 outside [0, 1] or NaN,
 * min_segments, max_planes or max_tests 0, reserved != 0.  More than 2^24 hypotheses: L3D_ERR_LIMIT, found after the
 * junctions' count pass ("lower junction_distance"), *out untouched.  n = 0: L3D_OK, no plane, a summary of zeros. */
int l3d_plane_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_planes_params* params,
                       l3d_planes** out);
/* The same on the context's lines (flattened as for l3d_compare_lines), on the context's stream.  The context is NOT
 * modified.  L3D_ERR_STATE without reconstructed lines or while a split call is open. */
int l3d_plane_lines(l3d_ctx*, const l3d_planes_params* params, l3d_planes** out);
/* the sizes of planes, members and scores; any pointer may be NULL */
int l3d_planes_counts(const l3d_planes*, uint64_t* n_planes, uint64_t* n_memberships, uint64_t* n_hypotheses);
/* planes [n_planes], members [n_memberships], seg_planes [n_segments]: the number of planes of every segment, scores
 * [n_hypotheses]: the device's score of every hypothesis; the summary.  Any pointer may be NULL */
int l3d_planes_get(const l3d_planes*, l3d_pl_plane* planes, l3d_pl_member* members, uint32_t* seg_planes, l3d_pl_score* scores,
                   l3d_planes_summary* summary);
/* four "v x y z" (%.17g), the corners, and one "f i j k l" (1-based) per plane, in plane order.  L3D_ERR_IO where the
 * file cannot be written. */
int l3d_planes_save_obj(const l3d_planes*, const char* path);
void l3d_planes_close(l3d_planes*);

/* ---- the directions the 3D lines run in (GPU: k_directions.hip, selection: l3d_directions.h) ------------------
 * No reference counterpart.  One model as above.  The direction of every segment is a hypothesis; every hypothesis is scored
 * on the device against every segment (a segment is an inlier iff the squared sine of its angle to the direction is at most
 * max_sin2, either way round; the score is the number of inliers and their length as an integer weight), and a sequential
 * selection on the host keeps the best-supported directions whose own segment is not yet a member of an accepted one and
 * that do not share more than half their weight with one.  A segment may belong to several directions.  The frame is the
 * rotation that turns the heaviest pairwise orthogonal directions into the coordinate axes.  The model itself is not
 * modified.  fp64, the contract of DESIGN §26. */
typedef struct l3d_directions_params {   /* 64 bytes */
    double max_sin2;             /* in [0, 1], no default: largest squared sine between a member and the direction */
    double min_length;           /* model units, finite, >= 0: least support (summed member length) of a direction */
    double max_frame_cos2;       /* in [0, 1]: two directions are orthogonal iff the squared cosine of their angle is <= this */
    uint32_t min_segments;       /* >= 1: least number of member segments */
    uint32_t max_directions;     /* >= 1 */
    uint32_t max_tests;          /* >= 1: candidates tested against the accepted directions before the selection gives up */
    uint32_t slice_chunks;       /* 0: the library chooses; else chunks of 256 segments per slice.  No output depends on it */
    uint32_t frame_search;       /* 1 .. 64: the frame is sought among so many of the first directions */
    uint32_t reserved[5];        /* must be 0 */
} l3d_directions_params;
/* an accepted direction (136 bytes), in order of acceptance */
typedef struct l3d_dir_direction {
    uint32_t hypothesis;         /* the segment whose direction it is */
    uint32_t n_segments;         /* members */
    uint32_t n_lines;            /* distinct line indices among them */
    uint32_t reserved;           /* 0 */
    uint64_t weight;             /* the members' integer weights, summed: length * 2^scale_exponent, each floored */
    double D[3];                 /* the unit direction of the hypothesis */
    double length;               /* of the members, added sequentially */
    double rms_sin;              /* root mean square of the members' sines against D */
    double D_fit[3];             /* the largest eigenvector of the members' length-weighted scatter, D_fit.D >= 0 */
    double rms_sin_fit;          /* ... against D_fit */
    double centroid[3];          /* of the members' end points */
    double t_min, t_max;         /* the extremes of (p - centroid).D_fit over them */
} l3d_dir_direction;
/* a membership (8 bytes), in (direction, segment) order */
typedef struct l3d_dir_member { uint32_t direction, segment; } l3d_dir_member;
/* the score of a hypothesis (16 bytes), as the device yields it */
typedef struct l3d_dir_score { uint64_t weight; uint32_t count, reserved; } l3d_dir_score;
/* (200 bytes) */
typedef struct l3d_directions_summary {
    uint64_t n_segments, n_point_segments;
    uint64_t n_candidates;                  /* live hypotheses with min_segments and min_length */
    uint64_t n_tested, n_dropped, n_rejected;
    uint64_t n_directions, n_memberships;
    uint64_t n_segments_in_directions, n_segments_in_several;
    uint64_t truncated;                     /* 1: max_tests was reached before the candidates or max_directions ran out */
    int64_t scale_exponent;                 /* weight = floor(length * 2^scale_exponent) */
    double length_total;                    /* of the segments, added sequentially */
    double length_in_directions;            /* of the segments in at least one direction, each once */
    uint32_t frame_axes;                    /* 0 .. 3: directions the frame rests on */
    uint32_t frame[3];                      /* their indices; an unused slot holds 0xFFFFFFFF */
    double R[9];                            /* row-major, p' = R p: the rotation into the frame; the identity without a direction */
} l3d_directions_summary;
typedef struct l3d_directions l3d_directions;
/* Stateless, host pointers.  segs6 [n x 6], line [n].  The result lives in a handle: *out, to be closed by
 * l3d_directions_close.  Checked before any device work, *out untouched: L3D_ERR_LIMIT for 2^30 or more segments;
 * L3D_ERR_ARG for a null pointer, a coordinate that is not finite or beyond 2^100 (the message names the segment), max_sin2
 * or max_frame_cos2 outside [0, 1] or NaN, min_length negative or not finite, min_segments, max_directions or max_tests 0,
 * frame_search outside 1 .. 64, reserved != 0.  n = 0: L3D_OK, no direction, a summary of zeros with the identity and an
 * unused frame, no launch. */
int l3d_direction_segments(int device, uint32_t n, const double* segs6, const uint32_t* line, const l3d_directions_params* params,
                           l3d_directions** out);
/* The same on the context's lines (flattened as for l3d_compare_lines), on the context's stream.  The context is NOT
 * modified.  L3D_ERR_STATE without reconstructed lines or while a split call is open. */
int l3d_direction_lines(l3d_ctx*, const l3d_directions_params* params, l3d_directions** out);
/* the sizes of directions, members and scores (n_hypotheses = the segments); any pointer may be NULL */
int l3d_directions_counts(const l3d_directions*, uint64_t* n_directions, uint64_t* n_memberships, uint64_t* n_hypotheses);
/* directions [n_directions], members [n_memberships], seg_directions [n_segments]: the number of directions of every
 * segment, scores [n_hypotheses]: the device's score of every hypothesis; the summary.  Any pointer may be NULL */
int l3d_directions_get(const l3d_directions*, l3d_dir_direction* directions, l3d_dir_member* members, uint32_t* seg_directions,
                       l3d_dir_score* scores, l3d_directions_summary* summary);
/* two "v x y z" (%.17g), centroid + t_min D_fit and centroid + t_max D_fit, and one "l i j" (1-based) per direction, in
 * direction order.  L3D_ERR_IO where the file cannot be written. */
int l3d_directions_save_obj(const l3d_directions*, const char* path);
void l3d_directions_close(l3d_directions*);

/* ---- the 3D lines refit against cameras and their 2D segments (GPU: k_refit.hip, and unchanged k_project.hip's
 * stage 1, k_scan.hip, k_associate.hip, k_lineopt.hip) ---------------------------------------------------------------------
 * No reference counterpart as a stage; it restates the reference's project2DsegmentOnto3Dline and the sweep of its final
 * segments.  Given a model as above, cameras (l3d_camera: K upper triangular with K22 = 1, K00, K11 != 0 and K01 = 0) and each
 * camera's 2D segments, every line of the model -- the segments that share a line index -- is re-estimated from the 2D
 * segments associated with it (l3d_project_segments + l3d_associate_segments' kernels at max_distance, on the device) by the
 * solver of the line bundling from the line's own carrier, and its segments are cut anew: the stretches of the new carrier
 * that at least `visibility` cameras see.  fp64, the contract of DESIGN §28. */
typedef struct l3d_refit_params {   /* 64 bytes */
    double max_distance;         /* as in l3d_associate_params */
    double min_cos2;
    double min_overlap;
    double near_plane;           /* finite, > 0: of the projection */
    double min_length;           /* finite, >= 0, world units: a shorter piece is not kept */
    uint32_t visibility;         /* >= 1: cameras that must see a piece; a line needs max(2, visibility) cameras to be refit */
    uint32_t max_iterations;     /* 0 .. 1000 of the solver; 0 cuts the extents anew about the unchanged carrier */
    uint32_t use_ambiguous;      /* 0: a 2D segment that accepted more than one record is left out; 1: it is used */
    uint32_t reserved[3];        /* must be 0 */
} l3d_refit_params;
enum { L3D_REFIT_REFIT = 0, L3D_REFIT_TOO_FEW_VIEWS = 1, L3D_REFIT_CONSTANT = 2, L3D_REFIT_FAILED = 3, L3D_REFIT_NO_EXTENT = 4,
       L3D_REFIT_EMPTY = 5 };
/* one per line index 0 .. max(line) (152 bytes) */
typedef struct l3d_refit_line {
    uint32_t status;             /* L3D_REFIT_* */
    uint32_t n_observations;     /* 2D segments that observe the line */
    uint32_t n_views;            /* distinct cameras among them */
    uint32_t solver_status;      /* the stopping rule of the line bundling's solver (1 gradient, 2 function, 3 parameter, 4
                                  * iterations, 5 other); 0 where the line was not solved */
    uint32_t iterations;
    uint32_t n_pieces;           /* segments of the line in the output model */
    double cost0, cost1;         /* the robust cost before and after the solve */
    double x0[4], x[4];          /* the Cayley parameters of the carrier about the model's centre: the start, the result */
    double P1[3], P2[3];         /* the carrier in the model's frame: written back where the line was solved, else as given */
} l3d_refit_line;
/* one per observation (32 bytes), line after line in ascending line index, a line's in ascending (camera, segment) order */
typedef struct l3d_refit_observation {
    uint32_t camera, segment;    /* the camera's index in the call, the 2D segment's index in its camera */
    uint32_t line;
    uint32_t valid;              /* 1: the span below entered the sweep */
    double s_lo, s_hi;           /* the span of the 2D segment along the new carrier, M + s u (0 where the line was not solved) */
} l3d_refit_observation;
/* (104 bytes) */
typedef struct l3d_refit_summary {
    uint64_t n_lines;
    uint64_t n_status[6];        /* lines per L3D_REFIT_* */
    uint64_t n_observations;
    uint64_t n_ambiguous_left_out;   /* associated 2D segments with n_accepted > 1 that use_ambiguous = 0 left out */
    uint64_t n_segments_before, n_segments_after;
    double cost0, cost1;         /* of the REFIT lines, added in ascending line index */
} l3d_refit_summary;
typedef struct l3d_refit l3d_refit;
/* Stateless, host pointers.  segs6 / line: the model, n x (P1, P2) with a line index each (a line's segments need not be
 * neighbours); cams [n_cams]; n_segments_per_cam[c] 2D segments (x1, y1, x2, y2) of camera c in segs4, camera after camera.
 * The result lives in a handle: *out, to be closed by l3d_refit_close.  Every line that is not REFIT keeps its segments bit
 * for bit in input order; the output model is grouped by ascending line index, a REFIT line's pieces in ascending s.
 * Checked before any device work, *out untouched: L3D_ERR_LIMIT for 2^30 or more model segments, a line index of 2^31 or
 * more, 2^32 or more 2D segments or a camera side beyond 65535; L3D_ERR_ARG for a null pointer where one is needed, a
 * coordinate not finite or beyond 2^100, a 2D segment or a camera with a non-finite entry or a side of zero pixels, a K that
 * is not upper triangular with K22 = 1, K00, K11 != 0 and K01 = 0, a threshold outside its range, a near plane not finite
 * or not > 0, min_length negative or not finite, visibility 0, max_iterations above 1000, use_ambiguous above 1,
 * reserved != 0, and the model's bounding box a point.  An empty model, zero cameras or no 2D segment at all: L3D_OK, every
 * line as given (TOO_FEW_VIEWS or EMPTY), no launch. */
int l3d_refit_segments(int device, uint32_t n_segments, const double* segs6, const uint32_t* line, uint32_t n_cams,
                       const l3d_camera* cams, const uint32_t* n_segments_per_cam, const float* segs4,
                       const l3d_refit_params* params, l3d_refit** out);
/* The same on the context's lines (flattened as for l3d_compare_lines) with the added views camIDs (each once) and their own
 * segments, on the context's stream; cams [n_views] or NULL: the views' own (l3d_view_camera).  The refit model TAKES THE
 * PLACE of the context's lines, as l3d_merge_lines' does: a REFIT line's segments are the new pieces, its cluster segment the
 * written-back carrier, its residuals its observations as (camID, segID); its reference view is kept, every other line is
 * untouched, the records of l3d_project_lines are cleared and l3d_output_filename carries "REFIT_<max_distance>__" until the
 * next reconstruct3Dlines; a call in which no line becomes REFIT leaves the records and the name alone, as it leaves the
 * model.  summary and out may be NULL.  L3D_ERR_STATE without reconstructed lines or while a split call is
 * open; an unknown camID or one named twice: L3D_ERR_ARG. */
int l3d_refit_view_lines(l3d_ctx*, uint32_t n_views, const uint32_t* camIDs, const l3d_camera* cams,
                         const l3d_refit_params* params, l3d_refit_summary* summary, l3d_refit** out);
/* the sizes of the output model, the lines, the observations and the associations (= the 2D segments); any may be NULL */
int l3d_refit_counts(const l3d_refit*, uint64_t* n_segments, uint64_t* n_lines, uint64_t* n_observations, uint64_t* n_associations);
/* segs6 [n_segments x 6] and seg_line [n_segments]: the output model; lines [n_lines]; observations [n_observations];
 * associations [n_associations]: what l3d_project_segments + l3d_associate_segments return for the call's inputs, camera
 * after camera; the summary.  Any pointer may be NULL */
int l3d_refit_get(const l3d_refit*, double* segs6, uint32_t* seg_line, l3d_refit_line* lines, l3d_refit_observation* observations,
                  l3d_association* associations, l3d_refit_summary* summary);
void l3d_refit_close(l3d_refit*);
/* Host only: the span stage's arithmetic for one camera (K, R are read) and one 2D segment (x1, y1, x2, y2), by the function
 * the device runs: the parameters s of the segment's two end points along M + s u as seen from the centre Q (all three about
 * the model's centre), ordered.  Returns 1: valid, 0: not (s_lo = s_hi = 0), -1: a null pointer. */
int l3d_refit_span(const l3d_camera* cam, const float seg4[4], const double M[3], const double u[3], const double Q[3],
                   double* s_lo, double* s_hi);
/* Host only: the sweep of stage 9 over n spans [s_lo, s_hi] with their cameras: pieces [2 x n at most] receives (s_start,
 * s_end) of the kept pieces in ascending s, *n_pieces their number; u_norm = |u| turns parameters into lengths.
 * L3D_ERR_ARG for a null pointer, visibility 0, or min_length / u_norm negative or not finite. */
int l3d_refit_sweep(uint32_t n, const double* s_lo, const double* s_hi, const uint32_t* camera, uint32_t visibility,
                    double min_length, double u_norm, double* pieces, uint32_t* n_pieces);

/* ---- cameras and 3D lines bundled jointly (GPU: k_bundle.hip, and unchanged k_project.hip's stage 1, k_scan.hip,
 * k_associate.hip, k_refit.hip) --------------------------------------------------------------------------------------------
 * No reference counterpart.  Given a model, cameras and each camera's 2D segments as l3d_refit_segments takes them, ONE
 * association at max_distance, then Levenberg-Marquardt jointly over 6 pose parameters of every free camera and 4
 * parameters of every eligible line on that fixed observation set, Huber(2) on every observation: the lines are eliminated
 * by a Schur complement on the device, the reduced camera system is solved on the host (dense: at most 512 free cameras).
 * Then the lines' segments are cut anew as l3d_refit_segments cuts them.  A line is ELIGIBLE iff it has a segment, its
 * carrier is not a point and at least max(2, visibility) cameras observe it; every other observed line is HELD: constant, but
 * its observations constrain their cameras.  A camera is FREE iff its byte of `fixed` is 0 and it observes a line.  fp64,
 * the contract of DESIGN §29.  Re-association between calls is the caller's (the Python driver bundle_model). */
typedef struct l3d_bundle_params {   /* 104 bytes */
    double max_distance;         /* as in l3d_associate_params */
    double min_cos2;
    double min_overlap;
    double near_plane;           /* finite, > 0: of the projection */
    double min_length;           /* finite, >= 0, world units: a shorter piece is not kept */
    double initial_damping;      /* mu of the first iteration, in [min_damping, max_damping]; 1e-4 */
    double min_damping;          /* finite, > 0: the floor of mu; 1e-9 */
    double max_damping;          /* finite, >= min_damping: a rejected step that takes mu past it ends the call STALLED; 1e8 */
    double function_tolerance;   /* finite, >= 0: an accepted step that gains no more than this share of the cost: CONVERGED; 1e-6 */
    uint32_t visibility;         /* >= 1: cameras that must see a piece; a line needs max(2, visibility) cameras to be eligible */
    uint32_t max_iterations;     /* 0 .. 256; 0 cuts the extents anew about the unchanged carriers */
    uint32_t use_ambiguous;      /* 0: a 2D segment that accepted more than one record is left out; 1: it is used */
    uint32_t capture_iteration;  /* test item: 0 none, k: the handle keeps the reduced system of the k-th iteration */
    uint32_t reserved[4];        /* must be 0 */
} l3d_bundle_params;
enum { L3D_BUNDLE_BUNDLED = 0, L3D_BUNDLE_HELD = 1, L3D_BUNDLE_NO_EXTENT = 2, L3D_BUNDLE_EMPTY = 3 };
enum { L3D_BUNDLE_CONVERGED = 0, L3D_BUNDLE_MAX_ITERATIONS = 1, L3D_BUNDLE_STALLED = 2, L3D_BUNDLE_NO_VARIABLES = 3 };
/* one per line index 0 .. max(line) (64 bytes) */
typedef struct l3d_bundle_line {
    uint32_t status;             /* L3D_BUNDLE_*: HELD too few views, a point for a carrier; NO_EXTENT took part, but the sweep
                                  * kept no piece; EMPTY no segment */
    uint32_t n_observations;     /* 2D segments that observe the line */
    uint32_t n_views;            /* its cells: distinct cameras among them */
    uint32_t n_pieces;           /* segments of the line in the output model */
    double P1[3], P2[3];         /* the carrier in the model's frame: as given, or, for an eligible line of a call that
                                  * accepted a step, the new one */
} l3d_bundle_line;
/* one per iteration run (56 bytes) */
typedef struct l3d_bundle_iteration {
    double damping;              /* mu of the iteration */
    double cost, cost_trial;     /* the robust cost in force and at the trial step (0 where the system was not solved) */
    double step_cameras;         /* |delta_c|inf over the free cameras */
    double step_lines;           /* |delta_l|inf over the eligible lines */
    uint32_t solved;             /* 0: a pivot of the reduced system failed (a rejected step) */
    uint32_t accepted;
    uint32_t n_held_for_step;    /* eligible lines whose own 4 x 4 pivot failed at this mu */
    uint32_t pad;
} l3d_bundle_iteration;
/* (144 bytes) */
typedef struct l3d_bundle_summary {
    uint32_t status;             /* L3D_BUNDLE_CONVERGED .. ; NO_VARIABLES: no eligible line and no free camera */
    uint32_t iterations, accepted_steps, rejected_steps;
    double cost0, cost1;         /* sum of rho over the observations before and after */
    double damping;              /* mu as the call left it */
    uint64_t n_observations, n_cells, n_eligible_lines, n_free_cameras, n_lines;
    uint64_t n_status[4];        /* lines per L3D_BUNDLE_* line status */
    uint64_t n_ambiguous_left_out, n_segments_before, n_segments_after;
    uint32_t captured;           /* 1: the system of capture_iteration is in the handle */
    uint32_t reserved;
} l3d_bundle_summary;
typedef struct l3d_bundle l3d_bundle;
/* Stateless, host pointers; the model, the cameras and the 2D segments as for l3d_refit_segments (K01 = 0 as there: the
 * spans are §28's); fixed [n_cams] bytes 0 / 1 or NULL: none is fixed.  The result lives in a handle: *out, to be closed by
 * l3d_bundle_close.  Every line that is not BUNDLED keeps its segments bit for bit; a camera that no accepted step moved
 * comes back bit for bit.  Checked before any device work, *out untouched: what l3d_refit_segments checks, with
 * max_iterations above 256, a damping or a tolerance outside its range, capture_iteration above 256 and a byte of `fixed`
 * above 1 as L3D_ERR_ARG; more than 512 cameras that are not fixed, or lines x cameras of 2^28 or more, as L3D_ERR_LIMIT.
 * An empty model, zero cameras or no 2D segment at all: L3D_OK, everything as given, no launch. */
int l3d_bundle_segments(int device, uint32_t n_segments, const double* segs6, const uint32_t* line, uint32_t n_cams,
                        const l3d_camera* cams, const uint8_t* fixed, const uint32_t* n_segments_per_cam, const float* segs4,
                        const l3d_bundle_params* params, l3d_bundle** out);
/* The same on the context's lines with the added views camIDs (each once) and their own segments, on the context's stream;
 * cams [n_views] or NULL: the views' own.  The bundled model TAKES THE PLACE of the context's lines as l3d_refit_view_lines'
 * does (l3d_output_filename carries "BUNDLE_<max_distance>__"); the cameras come back through the handle and the views'
 * cameras are NOT changed.  summary and out may be NULL.  L3D_ERR_STATE / L3D_ERR_ARG as l3d_refit_view_lines. */
int l3d_bundle_view_lines(l3d_ctx*, uint32_t n_views, const uint32_t* camIDs, const l3d_camera* cams, const uint8_t* fixed,
                          const l3d_bundle_params* params, l3d_bundle_summary* summary, l3d_bundle** out);
/* the sizes of the output model, the lines, the observations, the associations (= the 2D segments), the cameras, the trace
 * and the captured system's side n (0: none); any may be NULL */
int l3d_bundle_counts(const l3d_bundle*, uint64_t* n_segments, uint64_t* n_lines, uint64_t* n_observations, uint64_t* n_associations,
                      uint64_t* n_cameras, uint64_t* n_iterations, uint64_t* n_system);
/* segs6 / seg_line: the output model; lines; observations (l3d_refit_observation: the spans along the new carriers);
 * associations; cams [n_cameras]; trace [n_iterations]; system [n x n] (the upper triangle is set, the free cameras in
 * ascending index, 6 rows each) and rhs [n] (g: the step solves S delta = -g).  Any pointer may be NULL */
int l3d_bundle_get(const l3d_bundle*, double* segs6, uint32_t* seg_line, l3d_bundle_line* lines, l3d_refit_observation* observations,
                   l3d_association* associations, l3d_camera* cams, l3d_bundle_iteration* trace, double* system, double* rhs,
                   l3d_bundle_summary* summary);
void l3d_bundle_close(l3d_bundle*);
/* Host only: the stage's dense Cholesky solve of S delta = -g, S [n x n] symmetric of which the upper triangle is read.
 * Returns 1: solved, 0: a pivot that is not finite and > 0 (delta untouched), -1: a null pointer or no memory. */
int l3d_bundle_solve(uint32_t n, const double* S, const double* g, double* delta);

#ifdef __cplusplus
}
#endif
#endif /* L3DPP_HIP_H_ */
