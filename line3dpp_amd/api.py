"""Host-side mirror of the reference's public interface for the hot path.

`Line3D` follows class L3DPP::Line3D (line3D.h:61-424): `addImage`, `matchImages`,
and the affinity part of `reconstruct3Dlines`, with the reference's argument names, defaults
(commons.h:40-70) and error behaviour: errors are printed with the `[L3D++] ERROR:` prefix and the
call returns without raising (line3D.cc:119-126, 385-391); `last_status` holds the l3d_status
code.  All compute runs in libl3dpp_hip.so (HIP, gfx950) through the C-ABI in
include/l3dpp_hip.h.  The reference is C++; this Python front-end exists for the tests, the
bench and torch.distributed plumbing -- the C++ facade over the same C-ABI is
include/line3dpp/line3D.h.
"""
import ctypes as C
import math
import threading

import numpy as np

from . import _lib, lsd
from ._lib import (ALIGN_ITERATION_DTYPE, ALIGN_STATUS, ASSOCIATION_DTYPE, CLEDGE_DTYPE, EMPTY, FLOAT4_DTYPE, LINE_MATCH_DTYPE, MATCH_DTYPE, MERGE_LINE_INFO_DTYPE,
                   BUNDLE_ITERATION_DTYPE, BUNDLE_LINE_DTYPE, BUNDLE_LINE_STATUS, BUNDLE_STATUS,
                   POSE_ITERATION_DTYPE, POSE_STATUS, POSE_SUMMARY_DTYPE, PROJECTED_SEGMENT_DTYPE, REFIT_LINE_DTYPE,
                   REFIT_OBSERVATION_DTYPE, REFIT_STATUS, SEGMENT2D_DTYPE,
                   SEGMENT3D_DTYPE, SLOT_DTYPE, MatchParams, Timings, ptr)

# commons.h:40-70
L3D_DEF_MATCHING_NEIGHBORS = 10
L3D_DEF_EPIPOLAR_OVERLAP = 0.25
L3D_DEF_KNN = 10
L3D_DEF_SCORING_POS_REGULARIZER = 2.5
L3D_DEF_SCORING_ANG_REGULARIZER = 10.0
L3D_DEF_MIN_VISIBILITY_T = 3


class Line3D:
    PREFIX = "[L3D++] "

    def __init__(self, output_folder="", load_segments=False, max_img_width=-1, max_line_segments=3000,
                 neighbors_by_worldpoints=False, use_GPU=True, device=0, stream=0, verbose=False):
        # neighbors_by_worldpoints (line3D.cc:6-69): addImage's list is a WORLDPOINT list and the visual neighbours are found
        # from the worldpoint overlap at every matchImages (Line3D::findVisualNeighborsFromWPs, line3D.cc:578-699)
        self.neighbors_by_worldpoints = bool(neighbors_by_worldpoints)
        # what addImage's detection reads (line3D.cc:6-12): the cache folder <output_folder>/L3D++_data/, whether the
        # segment cache is used, the max-width downscale and the cap on segments per image
        self.output_folder = str(output_folder)
        self.load_segments = bool(load_segments)
        self.max_img_width = int(max_img_width)
        self.max_line_segments = int(max_line_segments)
        self._detect_lock = threading.Lock()
        self.L = _lib.load()
        self.verbose = verbose
        self.last_status = 0
        self._M = {}
        self.device = int(device)
        self.stream = int(stream)          # the hipStream_t every launch of this context goes to (dist.py: ordering of collectives)
        self.h = self.L.l3d_create(int(device), C.c_void_p(stream))
        if not self.h:
            raise RuntimeError("l3d_create failed: " + _lib.last_error())
        self.h = C.c_void_p(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.l3d_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- error behaviour of the reference: print and return ---------------------------------
    def _check(self, rc, what):
        self.last_status = rc
        if rc != 0:
            print(f"{self.PREFIX}ERROR: {what}: {_lib.last_error()} [{rc}]")
        return rc == 0

    # Line3D::addImage(camID, image, K, R, t, median_depth, wps_or_neighbors, line_segments), line3D.h:104-108
    def addImage(self, camID, image, K, R, t, median_depth, wps_or_neighbors, line_segments=()):
        """image = a (cols, rows) tuple, which stands in for the cv::Mat when `line_segments` are given (the image then
        only contributes its size, line3D.cc:119,198), or a uint8 HxW / HxWx3 ndarray (undistorted, e.g. by undistortImage;
        first channel = R).
        An ndarray with no segments is detected on the GPU, or loaded from the segment cache (line3D.cc:168-173)."""
        segs = np.ascontiguousarray(line_segments, np.float32).reshape(-1, 4)
        K = np.ascontiguousarray(K, np.float64).reshape(3, 3)
        R = np.ascontiguousarray(R, np.float64).reshape(3, 3)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        nb = np.ascontiguousarray(list(wps_or_neighbors), np.uint32)
        if isinstance(image, np.ndarray):
            img, keep = lsd.as_image(image)
            if len(segs) == 0:
                add = self.L.l3d_add_view_image_worldpoints if self.neighbors_by_worldpoints else self.L.l3d_add_view_image
                opts = self._detect_options()
                n_segs = C.c_uint32(0)          # this view's own count, set by the call that added it
                with self._detect_lock:         # keeps addImages' detection and the fetch of its segments together
                    rc = add(self.h, int(camID), C.byref(img), C.byref(opts), ptr(K), ptr(R), ptr(t), float(median_depth),
                             ptr(nb), len(nb), C.byref(n_segs))
                if rc == _lib.L3D_ERR_NO_SEGMENTS and len(nb) and max(img.cols, img.rows) >= 800:
                    self.last_status = rc
                    print(f"{self.PREFIX}WARNING: no line segments found in image [{camID}]!")
                    return
                if self._check(rc, f"addImage [{camID}]"):
                    self._M[int(camID)] = int(n_segs.value)
                return
            image_size = (img.cols, img.rows)
        else:
            image_size = image
        add = self.L.l3d_add_view_worldpoints if self.neighbors_by_worldpoints else self.L.l3d_add_view
        rc = add(self.h, int(camID), ptr(segs), len(segs), ptr(K), ptr(R), ptr(t),
                 int(image_size[0]), int(image_size[1]), float(median_depth), ptr(nb), len(nb))
        if self._check(rc, f"addImage [{camID}]"):
            self._M[int(camID)] = len(segs)

    # static void Line3D::undistortImage(inImg, outImg, radial_coeffs, tangential_coeffs, K), line3D.h:110-122: returns the
    # undistorted image (None after an error, which is printed); k_undistort.hip, DESIGN §12
    @staticmethod
    def undistortImage(img, radial, tangential, K):
        try:
            return lsd.undistort_images([img], [K], [radial], [tangential])[0]
        except (RuntimeError, TypeError) as e:
            print(f"{Line3D.PREFIX}ERROR: undistortImage: {e}")
            return None

    # undistortImage for COLMAP's camera models beyond five coefficients: model = COLMAP's name, params in
    # its order; K_new = the camera matrix of the returned image (None: K).  None after an error, which is printed
    @staticmethod
    def undistortImageModel(img, model, K, params, K_new=None):
        try:
            return lsd.undistort_images_model([img], [model], [K], [params], [K_new])[0]
        except (RuntimeError, TypeError, ValueError) as e:
            print(f"{Line3D.PREFIX}ERROR: undistortImage: {e}")
            return None

    # static members of the reference's Line3D (line3D.cc:2714-2754, :2784-2853), through the C-ABI (host code)
    @staticmethod
    def rotationFromRPY(roll, pitch, yaw):
        R = np.zeros((3, 3))
        _lib.load().l3d_rotation_from_rpy(float(roll), float(pitch), float(yaw), ptr(R))
        return R

    @staticmethod
    def rotationFromQ(Qw, Qx, Qy, Qz):
        R = np.zeros((3, 3))
        _lib.load().l3d_rotation_from_q(float(Qw), float(Qx), float(Qy), float(Qz), ptr(R))
        return R

    @staticmethod
    def decomposeProjectionMatrix(P_in):
        """-> (K, R, t) of P = K [R | t]; a P that is not 3x4 is reported and gives None, as the reference leaves its
        outputs alone"""
        P = np.ascontiguousarray(P_in, np.float64)
        if P.shape != (3, 4):
            print(f"P is not a 3x4 matrix! ({'x'.join(str(n) for n in P.shape)})")
            return None
        K, R, t = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
        _lib.load().l3d_decompose_projection_matrix(ptr(P), ptr(K), ptr(R), ptr(t))
        return K, R, t

    def _detect_options(self):
        folder = self.output_folder.encode()
        opts = _lib.DetectOptions(folder, int(self.load_segments), self.max_img_width, self.max_line_segments)
        opts._keep = folder             # the bytes behind output_folder live as long as the options
        return opts

    def addImages(self, camIDs, images, Ks, Rs, ts, median_depths, wps_or_neighbors):
        """addImage for many images with no segments, with ONE detection batch for all of them (a front end that reads
        every image first).  Views are added in the order given, each exactly as addImage would add it."""
        camIDs = [int(c) for c in camIDs]
        images = list(images)
        lists = [list(x) for x in wps_or_neighbors]
        # addImage's checks before detection (line3D.cc:119-158): such views are handed on without detecting them
        go = [i for i in range(len(images)) if max(images[i].shape[:2]) >= 800 and len(lists[i]) and camIDs[i] not in self._M
              and camIDs[i] not in camIDs[:i]]
        found = {}
        if go:
            arr, keep = lsd.image_array([images[i] for i in go])
            cams = np.array([camIDs[i] for i in go], np.uint32)
            counts = np.zeros(len(go), np.uint32)
            opts = self._detect_options()
            with self._detect_lock:         # the detection and the fetch of its segments, with no other detection between
                rc = self.L.l3d_detect_view_segments(self.h, len(go), ptr(cams), arr, C.byref(opts), ptr(counts))
                if not self._check(rc, "addImages"):
                    return
                found = dict(zip(go, lsd.fetch(self.L, self.h, counts)))
        for i in range(len(images)):
            im = np.asarray(images[i])
            if i in found and len(found[i]) == 0:
                self.last_status = _lib.L3D_ERR_NO_SEGMENTS
                print(f"{self.PREFIX}WARNING: no line segments found in image [{camIDs[i]}]!")
                continue
            self.addImage(camIDs[i], (im.shape[1], im.shape[0]), Ks[i], Rs[i], ts[i], median_depths[i], lists[i],
                          found.get(i, np.zeros((0, 4), np.float32)))

    def add_scene(self, scene):
        for v in scene.views:
            lst = v.worldpoints if self.neighbors_by_worldpoints else v.neighbors
            self.addImage(v.cam, (v.width, v.height), v.K, v.R, v.t, v.median_depth, lst, v.segs)

    def visualNeighbors(self, camID):
        """visual_neighbors_[camID] (line3D.h:352) as the last matchImages left it, ascending"""
        n = C.c_uint32(0)
        if not self._check(self.L.l3d_get_visual_neighbors(self.h, int(camID), None, 0, C.byref(n)), "visualNeighbors"):
            return None
        out = np.zeros(max(n.value, 1), np.uint32)
        self._check(self.L.l3d_get_visual_neighbors(self.h, int(camID), ptr(out), n.value, C.byref(n)), "visualNeighbors")
        return out[:n.value].copy()

    def _params(self, sigma_position, sigma_angle, num_neighbors, epipolar_overlap, kNN, const_regularization_depth):
        return MatchParams(float(sigma_position), float(sigma_angle), int(num_neighbors), float(epipolar_overlap),
                           int(kNN), float(const_regularization_depth))

    # Line3D::matchImages, line3D.h:143-148
    def matchImages(self, sigma_position=L3D_DEF_SCORING_POS_REGULARIZER, sigma_angle=L3D_DEF_SCORING_ANG_REGULARIZER,
                    num_neighbors=L3D_DEF_MATCHING_NEIGHBORS, epipolar_overlap=L3D_DEF_EPIPOLAR_OVERLAP,
                    kNN=L3D_DEF_KNN, const_regularization_depth=-1.0):
        p = self._params(sigma_position, sigma_angle, num_neighbors, epipolar_overlap, kNN, const_regularization_depth)
        return self._check(self.L.l3d_match_images(self.h, C.byref(p)), "matchImages")

    # split form for pair-sharded runs (see line3dpp_amd/dist.py)
    def matchBegin(self, sigma_position=L3D_DEF_SCORING_POS_REGULARIZER, sigma_angle=L3D_DEF_SCORING_ANG_REGULARIZER,
                   num_neighbors=L3D_DEF_MATCHING_NEIGHBORS, epipolar_overlap=L3D_DEF_EPIPOLAR_OVERLAP,
                   kNN=L3D_DEF_KNN, const_regularization_depth=-1.0):
        p = self._params(sigma_position, sigma_angle, num_neighbors, epipolar_overlap, kNN, const_regularization_depth)
        return self._check(self.L.l3d_match_begin(self.h, C.byref(p)), "matchBegin")

    def matchPairs(self, first, count):
        return self._check(self.L.l3d_match_pairs(self.h, int(first), int(count)), "matchPairs")

    def matchFinish(self):
        return self._check(self.L.l3d_match_finish(self.h), "matchFinish")

    def listsShard(self, rank, world):
        """phase B's list pass for this rank's share of the views (l3d_lists_shard): returns [(slab pointer, slab
        bytes, full-array pointer)] x 4 (edges, headers, segment headers, pool counters) or None"""
        sp = (C.c_void_p * 4)(); sb = (C.c_uint64 * 4)(); fp = (C.c_void_p * 4)()
        if not self._check(self.L.l3d_lists_shard(self.h, int(rank), int(world), sp, sb, fp), "listsShard"):
            return None
        return [(sp[k], int(sb[k]), fp[k]) for k in range(4)]

    def listsShardViews(self, rank, world, view0, view1):
        """the same for an explicit view range (l3d_lists_shard_views: the halo form, only the pairs that touch the
        range have to be present)"""
        sp = (C.c_void_p * 4)(); sb = (C.c_uint64 * 4)(); fp = (C.c_void_p * 4)()
        if not self._check(self.L.l3d_lists_shard_views(self.h, int(rank), int(world), int(view0), int(view1), sp, sb, fp),
                           "listsShardViews"):
            return None
        return [(sp[k], int(sb[k]), fp[k]) for k in range(4)]

    # the tail of phase B sharded by views (see line3dpp_amd/dist.py: match_images_halo)
    def tailShardCount(self):
        """l3d_tail_shard_count -> (status, surviving matches, best hypotheses of this rank's views)"""
        c = (C.c_uint32 * 2)()
        rc = self.L.l3d_tail_shard_count(self.h, c)
        self.last_status = rc
        return rc, int(c[0]), int(c[1])

    def shardOptions(self, first_needed_rank=0, exchanges_stream_ordered=False):
        """l3d_shard_options: the lowest rank whose records this rank's chain depends on; whether the caller's exchanges order
        themselves behind the context's stream (then the sharded entries return without waiting for the device)"""
        return self._check(self.L.l3d_shard_options(self.h, int(first_needed_rank), 1 if exchanges_stream_ordered else 0), "shardOptions")

    def tailShardLayout(self, world, counts_all, view_bounds):
        """l3d_tail_shard_layout -> [(device pointer of the full array, element bytes, [(first, count) per rank])] x 9, or None"""
        ca = (C.c_uint32 * (2 * world))(*[int(x) for pair in counts_all for x in pair])
        vb = (C.c_uint32 * (world + 1))(*[int(x) for x in view_bounds])
        bp = (C.c_void_p * 9)(); eb = (C.c_uint64 * 9)()
        first = (C.c_uint64 * (9 * world))(); count = (C.c_uint64 * (9 * world))()
        if not self._check(self.L.l3d_tail_shard_layout(self.h, int(world), ca, vb, bp, eb, first, count), "tailShardLayout"):
            return None
        return [(bp[k], int(eb[k]), [(int(first[9 * r + k]), int(count[9 * r + k])) for r in range(world)]) for k in range(9)]

    def tailShardCommit(self):
        rc = self.L.l3d_tail_shard_commit(self.h)
        self.last_status = rc
        return rc

    def matchAbort(self):
        """closes an open matchBegin without results (views untranslated, context idle); no-op otherwise"""
        return self.L.l3d_match_abort(self.h) == 0

    # the affinity part of Line3D::reconstruct3Dlines, line3D.h:162-166 / line3D.cc:1749-1778
    def computeAffinity(self):
        return self._check(self.L.l3d_compute_affinity(self.h), "computeAffinity")

    def affinityShardBegin(self, rank, world):
        """l3d_affinity_shard_begin -> (device pointer of the similarity array, 4, [(first, count) per rank]) in the form
        dist.exchange_parts takes, or None (not after a sharded tail / collinearity links asked for / an error)"""
        p = C.c_void_p(); first = (C.c_uint64 * world)(); count = (C.c_uint64 * world)()
        rc = self.L.l3d_affinity_shard_begin(self.h, int(rank), int(world), C.byref(p), first, count)
        self.last_status = rc
        if rc != 0:
            return None
        return (p.value, 4, [(int(first[r]), int(count[r])) for r in range(world)])

    def affinityShardFinish(self):
        return self._check(self.L.l3d_affinity_shard_finish(self.h), "affinityShardFinish")

    def affinityShardAbort(self):
        """l3d_affinity_shard_abort: close an open sharded fill without its bookkeeping pass (a peer could not shard)"""
        return self._check(self.L.l3d_affinity_shard_abort(self.h), "affinityShardAbort")

    # Line3D::reconstruct3Dlines, line3D.h:162-166 (defaults commons.h:63-70)
    def reconstruct3Dlines(self, visibility_t=L3D_DEF_MIN_VISIBILITY_T, perform_diffusion=False, collinearity_t=-1.0,
                           use_CERES=False, max_iter_CERES=250):
        """use_CERES bundles the 3D lines (optimizeClusters, line3D.cc:1800-1805) on the GPU: a per-line
        Levenberg-Marquardt solve of the reference's robust reprojection cost (include/l3dpp_hip.h).  The default stays
        False, as in a reference build without Ceres; a reference build with Ceres defaults to True (commons.h:84)."""
        ok = self._check(self.L.l3d_reconstruct_3d_lines(self.h, int(visibility_t), int(perform_diffusion),
                                                         float(collinearity_t), int(use_CERES), int(max_iter_CERES)),
                         "reconstruct3Dlines")
        if ok and use_CERES:    # optimization.cc:190
            print(f"{self.PREFIX}#unoptimizable_lines = {self.lineOptStats()['lines_constant']}")
        return ok

    def lineOptStats(self):
        """l3d_line_opt_stats: what the line bundling of the last reconstruct3Dlines did (dict)"""
        st = _lib.LineOptStats()
        self._check(self.L.l3d_line_opt_stats(self.h, C.byref(st)), "lineOptStats")
        return {name: getattr(st, name) for name, _ in st._fields_ if name != "reserved"}

    # Line3D::createOutputFilename (private in the reference; line3D.cc:2853-2893)
    def outputFilename(self, max_image_width=-1):
        buf = C.create_string_buffer(512)
        if not self._check(self.L.l3d_output_filename(self.h, int(max_image_width), buf, 512), "outputFilename"):
            return None
        return buf.value.decode()

    # Line3D::save3DLinesAsTXT, line3D.h:176 -- <output_folder>/<outputFilename()>.txt
    def save3DLinesAsTXT(self, output_folder, max_image_width=-1):
        return self._check(self.L.l3d_save_3d_lines_txt(self.h, str(output_folder).encode(), int(max_image_width)),
                           "save3DLinesAsTXT")

    # Line3D::save3DLinesAsBIN, line3D.h:177 -- <output_folder>/<outputFilename()>.bin (boost binary archive layout)
    def save3DLinesAsBIN(self, output_folder, max_image_width=-1):
        return self._check(self.L.l3d_save_3d_lines_bin(self.h, str(output_folder).encode(), int(max_image_width)),
                           "save3DLinesAsBIN")

    # Line3D::getSegmentCoords2D, line3D.h:195-197
    def getSegmentCoords2D(self, camID, segID):
        out = np.zeros(4, np.float32)
        self._check(self.L.l3d_get_segment_coords2d(self.h, int(camID), int(segID), ptr(out)), "getSegmentCoords2D")
        return out

    # Line3D::saveResultAsSTL / saveResultAsOBJ, line3D.h:174-175
    def saveResultAsSTL(self, output_folder, max_image_width=-1):
        return self._check(self.L.l3d_save_result_stl(self.h, str(output_folder).encode(), int(max_image_width)),
                           "saveResultAsSTL")

    def saveResultAsOBJ(self, output_folder, max_image_width=-1):
        return self._check(self.L.l3d_save_result_obj(self.h, str(output_folder).encode(), int(max_image_width)),
                           "saveResultAsOBJ")

    # Line3D::get3Dlines, line3D.h:173: list of FinalLine3D as dicts
    def get3Dlines(self):
        nl = C.c_uint32(); ns = C.c_uint32(); nr = C.c_uint32()
        if not self._check(self.L.l3d_num_3d_lines(self.h, C.byref(nl), C.byref(ns), C.byref(nr)), "get3Dlines"):
            return []
        so = np.zeros(nl.value + 1, np.uint32); ro = np.zeros(nl.value + 1, np.uint32)
        segs = np.zeros(max(ns.value, 1), SEGMENT3D_DTYPE); res = np.zeros(max(nr.value, 1), SEGMENT2D_DTYPE)
        cl = np.zeros(max(nl.value, 1), SEGMENT3D_DTYPE); rv = np.zeros(max(nl.value, 1), np.uint32)
        self.L.l3d_get_3d_lines(self.h, ptr(so), ptr(segs), ptr(ro), ptr(res), ptr(cl), ptr(rv))
        return [dict(collinear3Dsegments=segs[so[i]:so[i + 1]], residuals=res[ro[i]:ro[i + 1]],
                     cluster_line=cl[i], reference_view=int(rv[i])) for i in range(nl.value)]

    # ---- the 3D lines projected into cameras (no reference counterpart) -----------------------------------
    def viewCamera(self, camID):
        """l3d_view_camera: K, R, t and the image size of an added view as a dict (None after an error)"""
        cam = _lib.Camera()
        if not self._check(self.L.l3d_view_camera(self.h, int(camID), C.byref(cam)), f"viewCamera [{camID}]"):
            return None
        return camera_dict(cam)

    def _cameras(self, cams_or_camIDs):
        """a list of camera IDs of added views and / or cameras (dicts as viewCamera returns them) -> l3d_camera array"""
        cams = []
        for c in cams_or_camIDs:
            if isinstance(c, (int, np.integer)):
                c = self.viewCamera(c)
                if c is None:
                    return None
            cams.append(c)
        return camera_array(cams)

    def projectLines(self, cams_or_camIDs, near=1e-6):
        """the 3D lines of the last reconstruct3Dlines as every camera sees them: one PROJECTED_SEGMENT_DTYPE array per
        camera, ascending segment index (None after an error)"""
        arr = self._cameras(cams_or_camIDs)
        if arr is None:
            return None
        counts = np.zeros(max(len(arr), 1), np.uint32)
        if not self._check(self.L.l3d_project_lines(self.h, len(cams_or_camIDs), arr, float(near), ptr(counts)), "projectLines"):
            return None
        n = C.c_uint64(0)
        self.L.l3d_get_projected_lines(self.h, None, 0, C.byref(n))
        rec = np.zeros(max(n.value, 1), PROJECTED_SEGMENT_DTYPE)
        self._check(self.L.l3d_get_projected_lines(self.h, ptr(rec), n.value, C.byref(n)), "projectLines")
        return split_records(rec, counts[:len(cams_or_camIDs)])

    def renderLines(self, cams_or_camIDs, thickness=1, near=1e-6):
        """-> [(line_id int32 [h, w], inv_depth float32 [h, w])] per camera: the index of the 3D line drawn at a pixel
        (-1: none; the nearest where lines cross) and its 1 / depth there (None after an error)"""
        arr = self._cameras(cams_or_camIDs)
        if arr is None:
            return None
        n = len(cams_or_camIDs)
        ids = [np.empty((arr[i].height, arr[i].width), np.int32) for i in range(n)]
        izs = [np.empty((arr[i].height, arr[i].width), np.float32) for i in range(n)]
        if not self._check(self.L.l3d_render_lines(self.h, n, arr, float(near), int(thickness), pointer_array(ids),
                                                   pointer_array(izs)), "renderLines"):
            return None
        return list(zip(ids, izs))

    def drawLines(self, cams_or_camIDs, images, thickness=1, alpha=255, colors=None, near=1e-6):
        """the 3D lines drawn over `images` (uint8 HxW or HxWx3, one per camera, of the camera's size) -> list of uint8
        HxWx3.  colors: one RGB triple per 3D line, None: a fixed palette (None after an error)"""
        arr = self._cameras(cams_or_camIDs)
        if arr is None:
            return None
        n = len(cams_or_camIDs)
        try:
            imgs, keep = lsd.image_array(list(images))
        except TypeError as e:
            print(f"{self.PREFIX}ERROR: drawLines: {e}")
            return None
        if len(keep) != n:
            print(f"{self.PREFIX}ERROR: drawLines: one image per camera")
            return None
        outs = [np.empty((imgs[i].rows, imgs[i].cols, 3), np.uint8) for i in range(n)]
        col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        nl = C.c_uint32(); ns = C.c_uint32(); nr = C.c_uint32()
        # l3d_draw_lines reads one triple per 3D line and is not told the table's length: it is checked here
        if col is not None and not self._check(self.L.l3d_num_3d_lines(self.h, C.byref(nl), C.byref(ns), C.byref(nr)), "drawLines"):
            return None
        if col is not None and len(col) < nl.value:
            print(f"{self.PREFIX}ERROR: drawLines: fewer colors than 3D lines")
            return None
        if not self._check(self.L.l3d_draw_lines(self.h, n, arr, imgs, float(near), int(thickness), int(alpha), ptr(col),
                                                 pointer_array(outs)), "drawLines"):
            return None
        return outs

    # ---- the 2D segments that support each 3D line (no reference counterpart) ------------------------------
    def associateSegments(self, camIDs=None, max_distance=L3D_DEF_SCORING_POS_REGULARIZER,
                          max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, near=1e-6):
        """every segment of the views camIDs (None: all, ascending) assigned the 3D line of the last reconstruct3Dlines
        it observes -> (dict camID -> ASSOCIATION_DTYPE array with one entry per segment of the view, support_segments,
        support_views: per 3D line the assigned (view, segment) pairs and the distinct views among them); None after an
        error.  max_distance in pixels, max_angle in degrees [0, 90], min_overlap = share of the 2D segment."""
        ids = np.ascontiguousarray(sorted(self._M) if camIDs is None else list(camIDs), np.uint32).reshape(-1)
        try:
            par = associate_params(max_distance, max_angle, min_overlap)
        except ValueError as e:
            print(f"{self.PREFIX}ERROR: associateSegments: {e}")
            self.last_status = -1
            return None
        off = np.zeros(len(ids) + 1, np.uint64)
        args = (self.h, len(ids), ptr(ids), C.byref(par), float(near), ptr(off))
        nl = C.c_uint32(); ns = C.c_uint32(); nr = C.c_uint32()
        if not (self._check(self.L.l3d_associate_view_segments(*args, None, None, None), "associateSegments") and
                self._check(self.L.l3d_num_3d_lines(self.h, C.byref(nl), C.byref(ns), C.byref(nr)), "associateSegments")):
            return None
        out = np.zeros(max(int(off[-1]), 1), ASSOCIATION_DTYPE)
        sup_s = np.zeros(max(nl.value, 1), np.uint32); sup_v = np.zeros(max(nl.value, 1), np.uint32)
        if not self._check(self.L.l3d_associate_view_segments(*args, ptr(out), ptr(sup_s), ptr(sup_v)), "associateSegments"):
            return None
        res = {int(c): out[int(off[k]):int(off[k + 1])].copy() for k, c in enumerate(ids)}
        return res, sup_s[:nl.value], sup_v[:nl.value]

    # ---- this model compared with another one (no reference counterpart) ---------------------------------
    def compareLines(self, other, max_distance, max_angle=10.0, min_overlap=0.5, exclude_same_line=False, slice_chunks=0):
        """the 3D lines of the last reconstruct3Dlines compared with `other` -- a list of lines as get3Dlines or
        io.read_3d_lines_txt / read_3d_lines_bin return it, or another Line3D -- in both directions -> (matches_mine,
        matches_other, summary_mine, summary_other): a LINE_MATCH_DTYPE array with one entry per flat segment of each
        side (flatten_lines' order) and the summaries as dicts; None after an error.  max_distance in model units,
        max_angle in degrees [0, 90], min_overlap = the share of a segment inside its counterpart's extent."""
        if isinstance(other, Line3D):
            other = other.get3Dlines()
        try:
            par = compare_params(max_distance, max_angle, min_overlap, exclude_same_line, slice_chunks)
            segs, line = flatten_lines(other)
        except (ValueError, KeyError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: compareLines: {e}")
            self.last_status = -1
            return None
        nl = C.c_uint32(); ns = C.c_uint32(); nr = C.c_uint32()
        if not self._check(self.L.l3d_num_3d_lines(self.h, C.byref(nl), C.byref(ns), C.byref(nr)), "compareLines"):
            return None
        mine = np.zeros(max(ns.value, 1), LINE_MATCH_DTYPE); theirs = np.zeros(max(len(line), 1), LINE_MATCH_DTYPE)
        s_mine = _lib.CompareSummary(); s_other = _lib.CompareSummary()
        if not self._check(self.L.l3d_compare_lines(self.h, len(line), ptr(segs), ptr(line), C.byref(par), ptr(mine), ptr(theirs),
                                                    C.byref(s_mine), C.byref(s_other)), "compareLines"):
            return None
        return mine[:ns.value], theirs[:len(line)], summary_dict(s_mine), summary_dict(s_other)

    # ---- near-duplicate lines merged (no reference counterpart) -------------------------------------------
    def mergeLines(self, max_distance, max_angle=10.0, min_overlap=0.5, slice_chunks=0):
        """the 3D lines of the last reconstruct3Dlines replaced by the merged model: lines joined by accepted pairs of
        segments (the pair test of compareLines, between different lines) become one line -> the summary as a dict; None
        after an error.  get3Dlines, the writers, projectLines, associateSegments and compareLines see the merged model;
        outputFilename carries MERGED_<max_distance>__ until the next reconstruct3Dlines."""
        try:
            par = merge_params(max_distance, max_angle, min_overlap, slice_chunks)
        except (ValueError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: mergeLines: {e}")
            self.last_status = -1
            return None
        s = _lib.MergeSummary()
        if not self._check(self.L.l3d_merge_lines(self.h, C.byref(par), C.byref(s)), "mergeLines"):
            return None
        return merge_summary_dict(s)

    # ---- where the lines meet (no reference counterpart) ---------------------------------------------------
    def wireframe(self, max_distance, max_extension=None, min_angle=10.0, slice_chunks=0, obj_path=None):
        """the junctions of the 3D lines of the last reconstruct3Dlines and the graph they form -> the dict of
        build_wireframe (its segments are flatten_lines' of get3Dlines); None after an error.  The lines themselves are
        NOT modified."""
        try:
            par = wireframe_params(max_distance, max_extension, min_angle, slice_chunks)
        except (ValueError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: wireframe: {e}")
            self.last_status = -1
            return None
        h = C.c_void_p()
        if not self._check(self.L.l3d_wireframe_lines(self.h, C.byref(par), C.byref(h)), "wireframe"):
            return None
        return take_wireframe(h, obj_path)

    # ---- the planes the lines lie in (no reference counterpart) ---------------------------------------------
    def detectPlanes(self, max_distance, junction_distance=None, junction_extension=None, min_angle=10.0, min_length=0.0,
                     min_segments=4, max_planes=64, max_tests=4096, slice_chunks=0, obj_path=None):
        """the planes that the 3D lines of the last reconstruct3Dlines lie in -> the dict of detect_planes (its segments are
        flatten_lines' of get3Dlines); None after an error.  The lines themselves are NOT modified."""
        try:
            par = planes_params(max_distance, junction_distance, junction_extension, min_angle, min_length, min_segments,
                                max_planes, max_tests, slice_chunks)
        except (ValueError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: detectPlanes: {e}")
            self.last_status = -1
            return None
        h = C.c_void_p()
        if not self._check(self.L.l3d_plane_lines(self.h, C.byref(par), C.byref(h)), "detectPlanes"):
            return None
        return take_planes(h, obj_path)

    # ---- the directions the lines run in (no reference counterpart) -----------------------------------------
    def detectDirections(self, max_angle, min_length=0.0, min_segments=4, max_directions=16, max_tests=4096, frame_angle=5.0,
                         frame_search=16, slice_chunks=0, obj_path=None):
        """the directions that the 3D lines of the last reconstruct3Dlines run in, and the frame that stands the model
        upright -> the dict of detect_directions (its segments are flatten_lines' of get3Dlines); None after an error.  The
        lines themselves are NOT modified."""
        try:
            par = directions_params(max_angle, min_length, min_segments, max_directions, max_tests, frame_angle, frame_search,
                                    slice_chunks)
        except (ValueError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: detectDirections: {e}")
            self.last_status = -1
            return None
        h = C.c_void_p()
        if not self._check(self.L.l3d_direction_lines(self.h, C.byref(par), C.byref(h)), "detectDirections"):
            return None
        return take_directions(h, obj_path)

    # ---- this model aligned to another one (no reference counterpart) -------------------------------------
    def alignLines(self, other, max_distance, start_distance=0.0, initial=None, estimate_scale=True, max_angle=10.0,
                   min_overlap=0.5, step_tolerance=1e-9, max_iterations=50, min_matches=8, slice_chunks=0):
        """the similarity transform that moves the 3D lines of the last reconstruct3Dlines onto `other` (as in
        compareLines), by iterated closest lines from `initial` (a similarity dict, a 3x4 / 4x4 matrix, or None =
        identity) -> the dict of align_segments: the similarity, its matrix, the summary, the moved copy of this model's
        flat segments, the matches of both sides after alignment and the trace; None after an error.  The context's
        lines are NOT modified."""
        if isinstance(other, Line3D):
            other = other.get3Dlines()
        try:
            par = align_params(max_distance, start_distance, max_angle, min_overlap, step_tolerance, max_iterations, min_matches,
                               estimate_scale, slice_chunks)
            init = _similarity_struct(initial)
            segs, line = flatten_lines(other)
        except (ValueError, KeyError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: alignLines: {e}")
            self.last_status = -1
            return None
        nl = C.c_uint32(); ns = C.c_uint32(); nr = C.c_uint32()
        if not self._check(self.L.l3d_num_3d_lines(self.h, C.byref(nl), C.byref(ns), C.byref(nr)), "alignLines"):
            return None
        out = _AlignOutputs(ns.value, len(line), par.max_iterations)
        if not self._check(self.L.l3d_align_lines(self.h, len(line), ptr(segs), ptr(line), C.byref(par), init, *out.pointers()), "alignLines"):
            return None
        return out.result()

    # ---- the views' cameras refined against this model (no reference counterpart) -------------------------
    def refineCameras(self, camIDs=None, max_distance=L3D_DEF_SCORING_POS_REGULARIZER, start_distance=0.0,
                      max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, stall_tolerance=1e-4, step_tolerance=1e-9,
                      max_iterations=50, min_matches=8, near=1e-6):
        """the poses of the views camIDs (None: all, ascending) refined against the 3D lines of the last
        reconstruct3Dlines from each view's own segments -> the dict of refine_cameras, with `camIDs` beside it: cameras,
        summaries, associations and trace hold one entry per view in that order; None after an error.  The context --
        its views and its lines -- is NOT modified."""
        ids = np.ascontiguousarray(sorted(self._M) if camIDs is None else list(camIDs), np.uint32).reshape(-1)
        try:
            par = pose_params(max_distance, start_distance, max_angle, min_overlap, stall_tolerance, step_tolerance, max_iterations,
                              min_matches, near)
        except ValueError as e:
            print(f"{self.PREFIX}ERROR: refineCameras: {e}")
            self.last_status = -1
            return None
        # room for the segments the views were given (the context keeps at most that many; an unknown ID is the library's
        # to refuse); the offsets that come back say where each view's associations lie
        out = _PoseOutputs(len(ids), [self._M.get(int(c), 0) for c in ids], par.max_iterations)
        off = np.zeros(len(ids) + 1, np.uint64)
        if not self._check(self.L.l3d_refine_view_cameras(self.h, len(ids), ptr(ids), C.byref(par), out.cams, ptr(out.summaries),
                                                          ptr(off), ptr(out.assoc), ptr(out.trace)), "refineCameras"):
            return None
        out.n_seg = [int(off[k + 1] - off[k]) for k in range(len(ids))]
        res = out.result()
        res["camIDs"] = [int(c) for c in ids]
        return res

    # ---- this model refit against the views (no reference counterpart) --------------------------------------
    def refitLines(self, camIDs=None, cameras=None, max_distance=L3D_DEF_SCORING_POS_REGULARIZER,
                   max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, near=1e-6, min_length=0.0,
                   visibility=L3D_DEF_MIN_VISIBILITY_T, max_iterations=50, use_ambiguous=False):
        """the 3D lines of the last reconstruct3Dlines re-estimated from the segments of the views camIDs (None: all,
        ascending) that observe them, in `cameras` (camera dicts in that order; None: the views' own), and cut anew ->
        the dict of refit_segments with `camIDs` beside it; None after an error.  The refit model TAKES THE PLACE of the
        context's lines, as mergeLines' does; outputFilename carries REFIT_<max_distance>__ until the next
        reconstruct3Dlines."""
        ids = np.ascontiguousarray(sorted(self._M) if camIDs is None else list(camIDs), np.uint32).reshape(-1)
        try:
            par = refit_params(max_distance, max_angle, min_overlap, near, min_length, visibility, max_iterations, use_ambiguous)
            if cameras is not None and len(cameras) != len(ids):
                raise ValueError("one camera per view")
            arr = camera_array(list(cameras)) if cameras is not None else None
        except (ValueError, KeyError, TypeError) as e:
            print(f"{self.PREFIX}ERROR: refitLines: {e}")
            self.last_status = -1
            return None
        h = C.c_void_p(); s = _lib.RefitSummary()
        if not self._check(self.L.l3d_refit_view_lines(self.h, len(ids), ptr(ids), arr, C.byref(par), C.byref(s), C.byref(h)), "refitLines"):
            return None
        res = take_refit(h, None)
        res["camIDs"] = [int(c) for c in ids]
        return res

    def refineModel(self, rounds=3, camIDs=None, max_distance=L3D_DEF_SCORING_POS_REGULARIZER, start_distance=0.0, **kw):
        """refine_model on the 3D lines of the last reconstruct3Dlines and the views camIDs (None: all, ascending) with
        their own cameras and segments (kw: refine_model's) -> its dict, with `camIDs` beside it; None after an error.
        Every round refines the cameras against the context's lines as they stand and then refits those lines in the
        cameras just returned (refitLines), so the context holds the model of the last round that ran; the views keep
        their cameras.  After an error in round k (None is returned) the context is left with the model of round k - 1,
        its file names tagged REFIT_ if a round before refit a line; an error in round 0 leaves it as it was."""
        ids = [int(c) for c in (sorted(self._M) if camIDs is None else camIDs)]
        pose_kw = {k: kw[k] for k in ("max_angle", "min_overlap", "stall_tolerance", "step_tolerance", "min_matches", "near") if k in kw}
        refit_kw = {k: kw[k] for k in ("max_angle", "min_overlap", "near", "min_length", "visibility", "use_ambiguous") if k in kw}
        try:
            unknown = set(kw) - set(pose_kw) - set(refit_kw) - {"pose_iterations", "refit_iterations"}
            if unknown:
                raise TypeError(f"unknown arguments {sorted(unknown)}")
            cams = [self.viewCamera(c) for c in ids]
            if any(c is None for c in cams):
                raise ValueError("unknown camera ID")
            obs = [np.array([self.getSegmentCoords2D(c, s) for s in range(self._M[c])], np.float32).reshape(-1, 4) for c in ids]
            per_round, fit = [], None
            for r in range(int(rounds)):
                segs, line = flatten_lines(self.get3Dlines())
                pose = refine_cameras(segs, line, cams, obs, max_distance=max_distance, start_distance=start_distance if r == 0 else 0.0,
                                      max_iterations=kw.get("pose_iterations", 50), device=self.device, **pose_kw)
                cams = pose["cameras"]
                fit = self.refitLines(ids, cams, max_distance=max_distance, max_iterations=kw.get("refit_iterations", 50), **refit_kw)
                if fit is None:
                    return None
                per_round.append((pose["summaries"], fit["summary"]))
        except (ValueError, KeyError, TypeError, RuntimeError) as e:
            print(f"{self.PREFIX}ERROR: refineModel: {e}")
            self.last_status = -1
            return None
        segs, line = flatten_lines(self.get3Dlines())
        return dict(cameras=cams, segments=segs, line=line, rounds=per_round, refit=fit, camIDs=ids)

    # ---- this model and the views' cameras bundled jointly (no reference counterpart) ------------------------
    def bundleModel(self, camIDs=None, cameras=None, fixed=None, rounds=1, max_distance=L3D_DEF_SCORING_POS_REGULARIZER, **kw):
        """the 3D lines of the last reconstruct3Dlines and the cameras of the views camIDs (None: all, ascending; `cameras`:
        camera dicts in that order, None: the views' own) bundled jointly from the views' segments, `rounds` times, each
        round on the cameras the round before returned (kw: bundle_params') -> the dict of bundle_segments of the last
        round with `camIDs` and `rounds` (one summary per round) beside it; None after an error.  The bundled model TAKES
        THE PLACE of the context's lines; outputFilename carries BUNDLE_<max_distance>__ until the next
        reconstruct3Dlines.  The cameras come back in the dict: the views keep theirs."""
        ids = np.ascontiguousarray(sorted(self._M) if camIDs is None else list(camIDs), np.uint32).reshape(-1)
        res, per_round = None, []
        for _ in range(int(rounds)):
            try:
                par = bundle_params(max_distance, **kw)
                if cameras is not None and len(cameras) != len(ids):
                    raise ValueError("one camera per view")
                arr = camera_array(list(cameras)) if cameras is not None else None
                fx = _fixed_bytes(fixed, len(ids))
            except (ValueError, KeyError, TypeError) as e:
                print(f"{self.PREFIX}ERROR: bundleModel: {e}")
                self.last_status = -1
                return None
            h = C.c_void_p(); s = _lib.BundleSummary()
            if not self._check(self.L.l3d_bundle_view_lines(self.h, len(ids), ptr(ids), arr, ptr(fx) if fx is not None else None,
                                                            C.byref(par), C.byref(s), C.byref(h)), "bundleModel"):
                return None
            res = take_bundle(h, None)
            cameras = res["cameras"]
            per_round.append(res["summary"])
        if res is not None:
            res["camIDs"] = [int(c) for c in ids]
            res["rounds"] = per_round
        return res

    def set_projection_budget(self, n_bytes):
        """test hook: device-memory budget of a group of cameras in the four calls above (0: the default)"""
        self.L.l3d_set_projection_budget(self.h, int(n_bytes))

    def set_brute_force(self, on):
        self.L.l3d_set_brute_force(self.h, int(on))

    # ---- accessors ----------------------------------------------------------------------------
    def numImages(self):
        return len(self._M)

    def pairs(self):
        n = C.c_uint32()
        self.L.l3d_num_pairs(self.h, C.byref(n))
        s = np.zeros(n.value, np.uint32); t = np.zeros(n.value, np.uint32); off = np.zeros(n.value, np.uint64)
        self.L.l3d_get_pairs(self.h, ptr(s), ptr(t), ptr(off))
        return np.stack([s, t], 1), off

    def slot_buffer(self):
        p = C.c_void_p(); n = C.c_uint64()
        self.L.l3d_slot_buffer(self.h, C.byref(p), C.byref(n))
        return p.value, n.value

    def fresh_hyp(self):
        """test hook: the (depth_p1, depth_p2) stream of the slot buffer the list pass reads -- NaN for a slot that is not
        alive -- as float32 [n_slots, 2]"""
        _, n = self.slot_buffer()
        out = np.zeros((n, 2), np.float32)
        if not self._check(self.L.l3d_get_fresh_hyp(self.h, ptr(out), n), "fresh_hyp"):
            return None
        return out

    def slot_index_buffer(self):
        """device pointer of the compact exchange buffer (uint32 target index per slot) and its length"""
        p = C.c_void_p(); n = C.c_uint64()
        if not self._check(self.L.l3d_slot_index_buffer(self.h, C.byref(p), C.byref(n)), "slot_index_buffer"):
            return None, 0
        return p.value, n.value

    def packSlotIndices(self, first, count):
        return self._check(self.L.l3d_pack_slot_indices(self.h, int(first), int(count)), "packSlotIndices")

    def expandSlotIndices(self, first, count):
        return self._check(self.L.l3d_expand_slot_indices(self.h, int(first), int(count)), "expandSlotIndices")

    def pair_tests(self):
        n = C.c_uint64()
        self.L.l3d_pair_tests(self.h, C.byref(n))
        return n.value

    def pair_slots(self, pair_index):
        Ms = C.c_uint32(); K = C.c_uint32()
        if not self._check(self.L.l3d_get_pair_slots(self.h, pair_index, None, 0, C.byref(Ms), C.byref(K)), "pair_slots"):
            return None
        out = np.zeros((Ms.value, K.value), SLOT_DTYPE)
        self._check(self.L.l3d_get_pair_slots(self.h, pair_index, ptr(out), out.size, C.byref(Ms), C.byref(K)),
                    "pair_slots")
        return out

    def matches(self, camID):
        """matches_[camID] as (Match records, CSR offsets over the view's segments)"""
        M = self._M[camID]
        n = C.c_uint64()
        off = np.zeros(M + 1, np.uint32)
        if not self._check(self.L.l3d_get_matches(self.h, camID, None, 0, ptr(off), C.byref(n)), "matches"):
            return None, None
        out = np.zeros(max(n.value, 1), MATCH_DTYPE)
        self._check(self.L.l3d_get_matches(self.h, camID, ptr(out), n.value, ptr(off), C.byref(n)), "matches")
        return out[:n.value], off

    def best(self):
        """estimated_position3D_: (Segment2D keys, Segment3D, best Match), ordered by (camID, segID)"""
        n = C.c_uint32()
        self.L.l3d_num_best(self.h, C.byref(n))
        s2 = np.zeros(n.value, SEGMENT2D_DTYPE); s3 = np.zeros(n.value, SEGMENT3D_DTYPE); m = np.zeros(n.value, MATCH_DTYPE)
        if n.value:
            self._check(self.L.l3d_get_best(self.h, ptr(s2), ptr(s3), ptr(m)), "best")
        return s2, s3, m

    def view_info(self, camID):
        k = C.c_float(); md = C.c_float()
        self.L.l3d_view_info(self.h, camID, C.byref(k), C.byref(md))
        return dict(k=np.float32(k.value), median_depth=np.float32(md.value))

    def translation(self):
        t = np.zeros(3)
        self.L.l3d_translation(self.h, ptr(t))
        return t

    def affinity(self):
        """A_ (CLEdge array), local2global_ (Segment2D per matrix row), med_scene_depth_lines_"""
        ne = C.c_uint32(); nr = C.c_uint32()
        if not self._check(self.L.l3d_num_affinity(self.h, C.byref(ne), C.byref(nr)), "affinity"):
            return None, None, None
        e = np.zeros(max(ne.value, 1), CLEDGE_DTYPE); l2g = np.zeros(max(nr.value, 1), SEGMENT2D_DTYPE)
        msdl = C.c_float()
        self.L.l3d_get_affinity(self.h, ptr(e), ptr(l2g), C.byref(msdl))
        return e[:ne.value], l2g[:nr.value], np.float32(msdl.value)

    def sparse_matrix(self, sort_by_row=False):
        """L3DPP::SparseMatrix(A_, n_rows, 1.0f, sort_by_row): (float4 entries, int start_indices)"""
        ne = C.c_uint32(); nr = C.c_uint32()
        self.L.l3d_num_affinity(self.h, C.byref(ne), C.byref(nr))
        ent = np.zeros(max(ne.value, 1), FLOAT4_DTYPE); start = np.zeros(max(nr.value, 1), np.int32)
        self._check(self.L.l3d_get_sparse_matrix(self.h, int(sort_by_row), ptr(ent), ptr(start)), "sparse_matrix")
        return ent[:ne.value], start[:nr.value]

    def tail_records(self):
        """l3d_debug_tail_records (test hook): the records the converged list pass of the last matchImages left behind and
        what every kernel of phase B's tail made of them -> dict: the sizes (G, V, pools, ecap, hcap, scap, n_surv,
        n_hyps, n_slots), headers (HYP_HDR_DTYPE) with hdr_pool / hdr_index / hdr_positive, edges (EDGE_REC_DTYPE) with
        edge_index (pool * ecap + k, what HypHdr.edge_begin counts in) / edge_positive, segs (SEG_HDR_DTYPE), seg_base,
        max_score_bits [V, 16], kept_cnt, best_pack, off64s, surv_off, hyp_off, hyp_of_seg, surv_sg, surv_tg,
        depths [n_hyps, 2], medians.  None (and last_status) when the context holds no matches."""
        from ._lib import EDGE_REC_DTYPE, HYP_HDR_DTYPE, SEG_HDR_DTYPE, TailRecords
        t = TailRecords()
        if not self._check(self.L.l3d_debug_tail_records(self.h, 1, C.byref(t)), "tail_records"):
            return None
        out = {k: int(getattr(t, k)) for k in TailRecords.SIZES if k != "reserved"}
        out["n_slots"] = int(t.n_slots)
        G, V, nh, ne = t.G, t.V, t.n_headers, t.n_edges
        bufs = dict(seg_base=np.zeros(V + 1, np.uint32), hdr_words=np.zeros(nh, HYP_HDR_DTYPE), hdr_pool=np.zeros(nh, np.uint32),
                    hdr_index=np.zeros(nh, np.uint32), hdr_positive=np.zeros(nh, np.uint8), edge_words=np.zeros(ne, EDGE_REC_DTYPE),
                    edge_index=np.zeros(ne, np.uint32), edge_positive=np.zeros(ne, np.uint8),
                    seg_words=np.zeros(t.n_segs, SEG_HDR_DTYPE), max_score_bits=np.zeros((V, 16), np.uint32),
                    kept_cnt=np.zeros(G, np.uint32), best_pack=np.zeros(G, np.uint64), off64s=np.zeros(G + 1, np.uint64),
                    surv_off=np.zeros(G + 1, np.uint32), hyp_off=np.zeros(G + 1, np.uint32), hyp_of_seg=np.zeros(G, np.int32),
                    surv_sg=np.zeros(t.n_surv, np.uint32), surv_tg=np.zeros(t.n_surv, np.uint32),
                    depths=np.zeros((t.n_hyps, 2), np.float32), medians=np.zeros(V, np.float32))
        for k, a in bufs.items():
            setattr(t, k, a.ctypes.data if a.size else None)
        if not self._check(self.L.l3d_debug_tail_records(self.h, 0, C.byref(t)), "tail_records"):
            return None
        out.update(bufs)
        out["headers"] = out.pop("hdr_words"); out["edges"] = out.pop("edge_words"); out["segs"] = out.pop("seg_words")
        return out

    def affinity_records(self):
        """l3d_debug_affinity_records (test hook): what every stage of the affinity fill left behind -> dict: the sizes (N, H,
        G, V, n_cand, n_edges, n_rows, epos_total, touch_total, n_coll, n_child, n_own), mode (0 parallel path, 1 collinear
        path, 2 similarities only: between affinityShardBegin and affinityShardFinish), diffused, two_sigA_sqr,
        med_scene_depth_lines, and the arrays: view_k, msdl_dev, medians, hyps (HYP_REC_DTYPE), surv_off, surv_sg, surv_tg,
        hyp_of_seg, simv, cand_a, cand_b; mode 0: flag, epos, first_touch, touch_flag, touch_rank, edges, l2g; mode 1:
        coll_off, coll_idx, child_off / child_seg / child_sim, own_off / own_seg / own_sim, edges, l2g.  `edges` is None when
        the device holds the diffused matrix instead.  None (and last_status) when no affinity step has run on the
        current matches."""
        from ._lib import HYP_REC_DTYPE, AffinityRecords
        t = AffinityRecords()
        if not self._check(self.L.l3d_debug_affinity_records(self.h, 1, C.byref(t)), "affinity_records"):
            return None
        N, H, G, V, n, mode = t.N, t.H, t.G, t.V, t.n_cand, t.mode
        u32, i32, f32 = np.uint32, np.int32, np.float32
        bufs = dict(view_k=np.zeros(V, f32), msdl_dev=np.zeros(1, f32), medians=np.zeros(V, f32),
                    hyps=np.zeros(H, HYP_REC_DTYPE), surv_off=np.zeros(G + 1, u32), surv_sg=np.zeros(N, u32),
                    surv_tg=np.zeros(N, u32), hyp_of_seg=np.zeros(G, i32), simv=np.zeros(n, f32), cand_a=np.zeros(n, i32),
                    cand_b=np.zeros(n, i32))
        if mode == 0:
            bufs.update(flag=np.zeros(n, u32), epos=np.zeros(n, u32), first_touch=np.zeros(H if n else 0, u32),
                        touch_flag=np.zeros(2 * n + 1 if n else 0, u32), touch_rank=np.zeros(2 * n, u32))
        if mode == 1:
            bufs.update(coll_off=np.zeros(G + 1, u32), coll_idx=np.zeros(t.n_coll, u32),
                        child_off=np.zeros(N + 1, u32), child_seg=np.zeros(t.n_child, u32), child_sim=np.zeros(t.n_child, f32),
                        own_off=np.zeros(H + 1, u32), own_seg=np.zeros(t.n_own, u32), own_sim=np.zeros(t.n_own, f32))
        if mode in (0, 1):
            bufs.update(edges=np.zeros(t.n_edges, CLEDGE_DTYPE), l2g=np.zeros(t.n_rows, SEGMENT2D_DTYPE))
        for k, a in bufs.items():
            setattr(t, k, a.ctypes.data if a.size else None)
        if not self._check(self.L.l3d_debug_affinity_records(self.h, 0, C.byref(t)), "affinity_records"):
            return None
        out = {k: int(getattr(t, k)) for k in AffinityRecords.SIZES}
        out["two_sigA_sqr"] = np.float32(t.two_sigA_sqr); out["med_scene_depth_lines"] = np.float32(t.med_scene_depth_lines)
        out.update(bufs)
        if t.diffused and "edges" in out:
            out["edges"] = None
        return out

    def keep_rows(self):
        """l3d_debug_keep_rows (test hook): the layout of a keep-all call's ragged slot buffer as it lies on the device ->
        dict: the sizes (n_rows, n_pairs, n_blocks, keep_cap, tgt16, n_slots) and the arrays row_start [n_rows + 1], row_pair,
        blk_row [n_blocks], pair_info [n_pairs, 4] = {first slot, longest row, slots lo, slots hi}, slot_row and inv_tgt
        [n_slots].  None (and last_status) unless the context's current matches are ragged."""
        from ._lib import KeepRows
        t = KeepRows()
        if not self._check(self.L.l3d_debug_keep_rows(self.h, 1, C.byref(t)), "keep_rows"):
            return None
        u32 = np.uint32
        bufs = dict(row_start=np.zeros(t.n_rows + 1, u32), row_pair=np.zeros(t.n_rows, u32), blk_row=np.zeros(t.n_blocks, u32),
                    pair_info=np.zeros((t.n_pairs, 4), u32), slot_row=np.zeros(t.n_slots, u32), inv_tgt=np.zeros(t.n_slots, u32))
        for k, a in bufs.items():
            setattr(t, k, a.ctypes.data if a.size else None)
        if not self._check(self.L.l3d_debug_keep_rows(self.h, 0, C.byref(t)), "keep_rows"):
            return None
        out = {k: int(getattr(t, k)) for k in KeepRows.SIZES if k != "reserved"}
        out["n_slots"] = int(t.n_slots)
        out.update(bufs)
        return out

    def cull_state(self, pair_index):
        """l3d_debug_cull (test hook): the epipolar-band tables k_cull_prepare left for one pair of the last matchPairs launch,
        as they lie on the device -> dict: enabled, layout_rows (16 / 64: the padded class layout, 0: unpadded), Ms, Mt,
        src_len, n_chunks, the forms As / Bs / At / Bt, and src_perm [src_len], src_band [src_len, 2], tgt_perm [Mt],
        tgt_band [Mt, 2], chunk_band [n_chunks, 2] (all empty for a refused pair).  None (and last_status) outside the
        window between that launch and matchFinish / matchAbort."""
        from ._lib import CullState
        t = CullState()
        if not self._check(self.L.l3d_debug_cull(self.h, int(pair_index), 1, C.byref(t)), "cull_state"):
            return None
        u32, f32 = np.uint32, np.float32
        bufs = dict(src_perm=np.zeros(t.src_len, u32), src_band=np.zeros((t.src_len, 2), f32),
                    tgt_perm=np.zeros(t.Mt if t.enabled else 0, u32), tgt_band=np.zeros((t.Mt if t.enabled else 0, 2), f32),
                    chunk_band=np.zeros((t.n_chunks, 2), f32))
        for k, a in bufs.items():
            setattr(t, k, a.ctypes.data if a.size else None)
        if not self._check(self.L.l3d_debug_cull(self.h, int(pair_index), 0, C.byref(t)), "cull_state"):
            return None
        out = {k: int(getattr(t, k)) for k in CullState.SIZES}
        out.update({k: np.array(getattr(t, k)[:]) for k in CullState.FORMS})
        out.update(bufs)
        return out

    def setTimingLevel(self, level):
        """l3d_set_timing_level: 1 = the match kernel only (default), 2 = every phase timed with HIP events (profiling), 0 = none"""
        return self._check(self.L.l3d_set_timing_level(self.h, int(level)), "setTimingLevel")

    def timings(self):
        t = Timings()
        self.L.l3d_get_timings(self.h, C.byref(t))
        return {f: getattr(t, f) for f, _ in Timings._fields_}


def cull_forms(F, ws, hs, wt, ht):
    """l3d_cull_forms (test hook, host only): the culling set-up of a directed pair as matchBegin computes it, from the
    fundamental matrix (3 x 3) and the two image sizes -> (As, Bs, At, Bt), or None where the pair is refused"""
    info = _lib.CullFormsInfo()
    Fm = np.ascontiguousarray(F, np.float64).reshape(9)
    rc = _lib.load().l3d_cull_forms(ptr(Fm), float(ws), float(hs), float(wt), float(ht), C.byref(info))
    if rc != 0:
        raise RuntimeError(f"l3d_cull_forms: {rc}")
    return tuple(np.array(getattr(info, k)[:]) for k in ("As", "Bs", "At", "Bt")) if info.enabled else None


def camera_dict(cam):
    return dict(K=np.array(cam.K[:]).reshape(3, 3), R=np.array(cam.R[:]).reshape(3, 3), t=np.array(cam.t[:]),
                width=int(cam.width), height=int(cam.height))


def camera_array(cams):
    """cameras as dicts (K, R, t, width, height) or l3d_camera -> ctypes array of l3d_camera"""
    arr = (_lib.Camera * max(len(cams), 1))()
    for i, c in enumerate(cams):
        if isinstance(c, _lib.Camera):
            arr[i] = c
            continue
        arr[i].K[:] = [float(v) for v in np.asarray(c["K"], np.float64).reshape(9)]
        arr[i].R[:] = [float(v) for v in np.asarray(c["R"], np.float64).reshape(9)]
        arr[i].t[:] = [float(v) for v in np.asarray(c["t"], np.float64).reshape(3)]
        arr[i].width, arr[i].height = int(c["width"]), int(c["height"])
    return arr


def pointer_array(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def split_records(rec, counts):
    out, o = [], 0
    for c in counts:
        out.append(rec[o:o + int(c)].copy())
        o += int(c)
    return out


def project_segments(cams, P1, P2, line_of_segment, near=1e-6, device=0):
    """l3d_project_segments (stage 1): 3D segments P1, P2 [n, 3] of the lines line_of_segment [n] as the
    cameras (dicts K, R, t, width, height) see them -> one PROJECTED_SEGMENT_DTYPE array per camera: clipped at the near
    plane and at the image, ascending segment index"""
    L = _lib.load()
    P1 = np.ascontiguousarray(P1, np.float64).reshape(-1, 3); P2 = np.ascontiguousarray(P2, np.float64).reshape(-1, 3)
    line = np.ascontiguousarray(line_of_segment, np.uint32).reshape(-1)
    if not len(P1) == len(P2) == len(line):
        raise ValueError("one P1, P2 and line index per segment")
    segs = np.zeros(max(len(P1), 1), SEGMENT3D_DTYPE)
    segs["P1"][:len(P1)] = P1; segs["P2"][:len(P1)] = P2
    arr = camera_array(list(cams))
    counts = np.zeros(max(len(cams), 1), np.uint32)
    n = C.c_uint64(0)
    args = (int(device), len(cams), arr, len(P1), ptr(segs), ptr(line), float(near), ptr(counts))
    # one call with room for every (camera, segment) while that is small (64 MiB); beyond it a call for the number first
    cap = len(cams) * len(P1) if 32 * len(cams) * len(P1) <= (64 << 20) else 0
    rec = np.zeros(max(cap, 1), PROJECTED_SEGMENT_DTYPE)
    rc = L.l3d_project_segments(*args, ptr(rec) if cap else None, cap, C.byref(n))
    if rc == 0 and n.value > cap:
        rec = np.zeros(n.value, PROJECTED_SEGMENT_DTYPE)
        rc = L.l3d_project_segments(*args, ptr(rec), n.value, C.byref(n))
    if rc != 0:
        raise RuntimeError(f"l3d_project_segments failed [{rc}]: {_lib.last_error()}")
    return split_records(rec, counts[:len(cams)])


def associate_params(max_distance, max_angle, min_overlap):
    """l3d_associate_params from the wrappers' arguments: min_cos2 = cos(radians(max_angle))^2, max_angle in [0, 90]"""
    if not 0.0 <= float(max_angle) <= 90.0:
        raise ValueError("max_angle must lie in [0, 90] degrees")
    cos = float(np.cos(np.radians(np.float64(max_angle))))
    return _lib.AssociateParams(float(max_distance), cos * cos, float(min_overlap))


def associate_segments(records_per_cam, segs_per_cam, max_distance=L3D_DEF_SCORING_POS_REGULARIZER,
                       max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, device=0):
    """l3d_associate_segments: records_per_cam = one PROJECTED_SEGMENT_DTYPE array per camera (as
    project_segments returns them), segs_per_cam = one float32 [M, 4] array of 2D segments (x1, y1, x2, y2) per camera
    -> one ASSOCIATION_DTYPE array per camera, one entry per 2D segment: the record it observes, or none"""
    L = _lib.load()
    if len(records_per_cam) != len(segs_per_cam):
        raise ValueError("one array of records and one of segments per camera")
    recs = [np.ascontiguousarray(r, PROJECTED_SEGMENT_DTYPE).reshape(-1) for r in records_per_cam]
    segs = [np.ascontiguousarray(s, np.float32).reshape(-1, 4) for s in segs_per_cam]
    n = len(recs)
    n_rec = np.array([len(r) for r in recs] + [0], np.uint32); n_seg = np.array([len(s) for s in segs] + [0], np.uint32)
    rec = np.concatenate(recs + [np.zeros(1, PROJECTED_SEGMENT_DTYPE)])
    seg = np.concatenate(segs + [np.zeros((1, 4), np.float32)])
    out = np.zeros(len(seg), ASSOCIATION_DTYPE)
    par = associate_params(max_distance, max_angle, min_overlap)
    rc = L.l3d_associate_segments(int(device), n, ptr(n_rec), ptr(rec), ptr(n_seg), ptr(seg), C.byref(par), ptr(out))
    if rc != 0:
        raise RuntimeError(f"l3d_associate_segments failed [{rc}]: {_lib.last_error()}")
    return split_records(out, n_seg[:n])


def compare_params(max_distance, max_angle=10.0, min_overlap=0.5, exclude_same_line=False, slice_chunks=0):
    """l3d_compare_params from the wrappers' arguments: min_cos2 = cos(radians(max_angle))^2, max_angle in [0, 90]"""
    if not 0.0 <= float(max_angle) <= 90.0:
        raise ValueError("max_angle must lie in [0, 90] degrees")
    cos = float(np.cos(np.radians(np.float64(max_angle))))
    return _lib.CompareParams(float(max_distance), cos * cos, float(min_overlap), int(bool(exclude_same_line)), int(slice_chunks))


def flatten_lines(lines):
    """a list of 3D lines -> (segs [n, 6] float64 (P1, P2), line [n] uint32: the index of each segment's line in the
    list).  Both list forms: the dicts of Line3D.get3Dlines (collinear3Dsegments with P1, P2) and those of
    io.read_3d_lines_txt / read_3d_lines_bin (segments [n, 6] or [n, 9]: P1, P2 first)."""
    segs, line = [], []
    for i, L in enumerate(lines):
        c = L["collinear3Dsegments"] if "collinear3Dsegments" in L else L["segments"]
        if getattr(c, "dtype", None) is not None and c.dtype.names:
            s = np.concatenate([np.asarray(c["P1"], np.float64).reshape(-1, 3), np.asarray(c["P2"], np.float64).reshape(-1, 3)], 1)
        else:
            s = np.asarray(c, np.float64)
            s = s.reshape(len(s), -1)[:, :6] if len(s) else np.zeros((0, 6))
        if s.shape[1] != 6:
            raise ValueError(f"line {i}: segments need P1 and P2, six coordinates each")
        segs.append(s)
        line.append(np.full(len(s), i, np.uint32))
    if not segs:
        return np.zeros((0, 6), np.float64), np.zeros(0, np.uint32)
    return np.ascontiguousarray(np.concatenate(segs), np.float64), np.concatenate(line)


def summary_dict(s):
    return {f: getattr(s, f) for f, _ in _lib.CompareSummary._fields_}


def compare_segments(q_segs, q_line, r_segs, r_line, max_distance, max_angle=10.0, min_overlap=0.5, exclude_same_line=False,
                     slice_chunks=0, device=0):
    """l3d_compare_segments: two models of 3D segments, segs [n, 6] float64 (P1, P2) with a line index each,
    compared in both directions -> (matches_q, matches_r, summary_q, summary_r): one LINE_MATCH_DTYPE entry per segment
    of Q (its counterpart in R) and of R (its counterpart in Q); the summaries are dicts"""
    L = _lib.load()
    q = np.ascontiguousarray(q_segs, np.float64).reshape(-1, 6); r = np.ascontiguousarray(r_segs, np.float64).reshape(-1, 6)
    ql = np.ascontiguousarray(q_line, np.uint32).reshape(-1); rl = np.ascontiguousarray(r_line, np.uint32).reshape(-1)
    if len(ql) != len(q) or len(rl) != len(r):
        raise ValueError("one line index per segment")
    par = compare_params(max_distance, max_angle, min_overlap, exclude_same_line, slice_chunks)
    mq = np.zeros(max(len(q), 1), LINE_MATCH_DTYPE); mr = np.zeros(max(len(r), 1), LINE_MATCH_DTYPE)
    sq = _lib.CompareSummary(); sr = _lib.CompareSummary()
    rc = L.l3d_compare_segments(int(device), len(q), ptr(q), ptr(ql), len(r), ptr(r), ptr(rl), C.byref(par), ptr(mq), ptr(mr),
                                C.byref(sq), C.byref(sr))
    if rc != 0:
        raise RuntimeError(f"l3d_compare_segments failed [{rc}]: {_lib.last_error()}")
    return mq[:len(q)], mr[:len(r)], summary_dict(sq), summary_dict(sr)


def merge_params(max_distance, max_angle=10.0, min_overlap=0.5, slice_chunks=0):
    """l3d_merge_params from the wrappers' arguments, by compare_params' degree rule"""
    p = compare_params(max_distance, max_angle, min_overlap, False, slice_chunks)
    return _lib.MergeParams(p.max_distance, p.min_cos2, p.min_overlap, p.slice_chunks, 0)


def merge_summary_dict(s):
    return {f: getattr(s, f) for f, _ in _lib.MergeSummary._fields_}


def merge_segments(segs, line, max_distance, max_angle=10.0, min_overlap=0.5, slice_chunks=0, device=0):
    """l3d_merge_segments: one model of 3D segments, segs [n, 6] float64 (P1, P2) with a line index each ->
    (segs_out [m, 6], line_out [m] uint32: the output line of each output segment, line_map [n] uint32: the output line
    of each input segment, line_info: one MERGE_LINE_INFO_DTYPE entry per output line, summary: a dict)"""
    L = _lib.load()
    s = np.ascontiguousarray(segs, np.float64).reshape(-1, 6)
    ln = np.ascontiguousarray(line, np.uint32).reshape(-1)
    if len(ln) != len(s):
        raise ValueError("one line index per segment")
    par = merge_params(max_distance, max_angle, min_overlap, slice_chunks)
    n = len(s); cap = max(n, 1)
    line_map = np.zeros(cap, np.uint32); out = np.zeros((cap, 6), np.float64); out_line = np.zeros(cap, np.uint32)
    info = np.zeros(cap, MERGE_LINE_INFO_DTYPE)
    n_segs = C.c_uint32(); n_lines = C.c_uint32(); summary = _lib.MergeSummary()
    rc = L.l3d_merge_segments(int(device), n, ptr(s), ptr(ln), C.byref(par), ptr(line_map), cap, ptr(out), ptr(out_line),
                              C.byref(n_segs), cap, ptr(info), C.byref(n_lines), C.byref(summary))
    if rc != 0:
        raise RuntimeError(f"l3d_merge_segments failed [{rc}]: {_lib.last_error()}")
    return out[:n_segs.value], out_line[:n_segs.value], line_map[:n], info[:n_lines.value], merge_summary_dict(summary)


def wireframe_params(max_distance, max_extension=None, min_angle=10.0, slice_chunks=0):
    """l3d_wireframe_params from the wrappers' arguments: max_extension None = max_distance; min_sin2 =
    sin(radians(min_angle))^2, min_angle in [0, 90] (compare_params' degree rule)"""
    if not 0.0 <= float(min_angle) <= 90.0:
        raise ValueError("min_angle must lie in [0, 90] degrees")
    sin = float(np.sin(np.radians(np.float64(min_angle))))
    return _lib.WireframeParams(float(max_distance), float(max_distance if max_extension is None else max_extension), sin * sin,
                                int(slice_chunks), 0)


def wireframe_summary_dict(s):
    return {f: getattr(s, f) for f, _ in _lib.WireframeSummary._fields_}


def take_wireframe(handle, obj_path=None):
    """the arrays and the summary out of an l3d_wireframe handle, which is closed -> dict(junctions: WF_JUNCTION_DTYPE,
    vertices: WF_VERTEX_DTYPE, edges: WF_EDGE_DTYPE, summary: dict).  obj_path: l3d_wireframe_save_obj writes it first"""
    L = _lib.load()
    try:
        if obj_path is not None and L.l3d_wireframe_save_obj(handle, str(obj_path).encode()) != 0:
            raise RuntimeError(f"l3d_wireframe_save_obj failed: {_lib.last_error()}")
        nj = C.c_uint64(); nv = C.c_uint64(); ne = C.c_uint64(); s = _lib.WireframeSummary()
        L.l3d_wireframe_counts(handle, C.byref(nj), C.byref(nv), C.byref(ne))
        j = np.zeros(max(nj.value, 1), _lib.WF_JUNCTION_DTYPE); v = np.zeros(max(nv.value, 1), _lib.WF_VERTEX_DTYPE)
        e = np.zeros(max(ne.value, 1), _lib.WF_EDGE_DTYPE)
        L.l3d_wireframe_get(handle, ptr(j), ptr(v), ptr(e), C.byref(s))
    finally:
        L.l3d_wireframe_close(handle)
    return dict(junctions=j[:nj.value], vertices=v[:nv.value], edges=e[:ne.value], summary=wireframe_summary_dict(s))


def build_wireframe(segs, line, max_distance, max_extension=None, min_angle=10.0, slice_chunks=0, device=0, obj_path=None):
    """l3d_wireframe_segments: one model of 3D segments, segs [n, 6] float64 (P1, P2) with a line index each ->
    dict(junctions, vertices, edges: structured arrays, summary: a dict): where the lines meet, the vertices these
    junctions and the free ends form, and every segment cut into the edges between its vertices.  max_distance and
    max_extension (None: max_distance) in model units, min_angle in degrees [0, 90]."""
    L = _lib.load()
    s = np.ascontiguousarray(segs, np.float64).reshape(-1, 6)
    ln = np.ascontiguousarray(line, np.uint32).reshape(-1)
    if len(ln) != len(s):
        raise ValueError("one line index per segment")
    par = wireframe_params(max_distance, max_extension, min_angle, slice_chunks)
    h = C.c_void_p()
    rc = L.l3d_wireframe_segments(int(device), len(s), ptr(s), ptr(ln), C.byref(par), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"l3d_wireframe_segments failed [{rc}]: {_lib.last_error()}")
    return take_wireframe(h, obj_path)


def write_wireframe_obj(wireframe, path):
    """a wireframe as build_wireframe returns it -> an OBJ file, the bytes of l3d_wireframe_save_obj: "v x y z" at %.17g per
    vertex, then "l i j" (1-based) per edge"""
    with open(path, "w") as f:
        for v in wireframe["vertices"]:
            f.write("v %.17g %.17g %.17g\n" % (float(v["P"][0]), float(v["P"][1]), float(v["P"][2])))
        for e in wireframe["edges"]:
            f.write("l %d %d\n" % (int(e["v0"]) + 1, int(e["v1"]) + 1))


def planes_params(max_distance, junction_distance=None, junction_extension=None, min_angle=10.0, min_length=0.0, min_segments=4,
                  max_planes=64, max_tests=4096, slice_chunks=0):
    """l3d_planes_params from the wrappers' arguments: junction_distance and junction_extension None = max_distance;
    min_sin2 by wireframe_params' degree rule"""
    w = wireframe_params(max_distance if junction_distance is None else junction_distance,
                         max_distance if junction_extension is None else junction_extension, min_angle, slice_chunks)
    return _lib.PlanesParams(float(max_distance), w.max_distance, w.max_extension, w.min_sin2, float(min_length), int(min_segments),
                             int(max_planes), int(max_tests), w.slice_chunks, (0, 0))


def planes_summary_dict(s):
    return {f: getattr(s, f) for f, _ in _lib.PlanesSummary._fields_}


def take_planes(handle, obj_path=None):
    """the arrays and the summary out of an l3d_planes handle, which is closed -> dict(planes: PL_PLANE_DTYPE, members:
    PL_MEMBER_DTYPE, seg_planes: uint32 per segment, scores: PL_SCORE_DTYPE per hypothesis, summary: dict).  obj_path:
    l3d_planes_save_obj writes it first"""
    L = _lib.load()
    try:
        if obj_path is not None and L.l3d_planes_save_obj(handle, str(obj_path).encode()) != 0:
            raise RuntimeError(f"l3d_planes_save_obj failed: {_lib.last_error()}")
        n_p = C.c_uint64(); n_m = C.c_uint64(); n_h = C.c_uint64(); s = _lib.PlanesSummary()
        L.l3d_planes_counts(handle, C.byref(n_p), C.byref(n_m), C.byref(n_h))
        L.l3d_planes_get(handle, None, None, None, None, C.byref(s))
        planes = np.zeros(max(n_p.value, 1), _lib.PL_PLANE_DTYPE); members = np.zeros(max(n_m.value, 1), _lib.PL_MEMBER_DTYPE)
        seg_planes = np.zeros(max(s.n_segments, 1), np.uint32); scores = np.zeros(max(n_h.value, 1), _lib.PL_SCORE_DTYPE)
        L.l3d_planes_get(handle, ptr(planes), ptr(members), ptr(seg_planes), ptr(scores), None)
    finally:
        L.l3d_planes_close(handle)
    return dict(planes=planes[:n_p.value], members=members[:n_m.value], seg_planes=seg_planes[:s.n_segments], scores=scores[:n_h.value],
                summary=planes_summary_dict(s))


def detect_planes(segs, line, max_distance, junction_distance=None, junction_extension=None, min_angle=10.0, min_length=0.0,
                  min_segments=4, max_planes=64, max_tests=4096, slice_chunks=0, device=0, obj_path=None):
    """l3d_plane_segments: one model of 3D segments, segs [n, 6] float64 (P1, P2) with a line index each ->
    dict(planes, members, seg_planes, scores: arrays, summary: a dict): the planes that at least min_segments segments of
    at least min_length in all lie in, both end points within max_distance, each spanned by two lines that meet (§24 with
    junction_distance, junction_extension -- None: max_distance -- and min_angle in degrees [0, 90])."""
    L = _lib.load()
    s = np.ascontiguousarray(segs, np.float64).reshape(-1, 6)
    ln = np.ascontiguousarray(line, np.uint32).reshape(-1)
    if len(ln) != len(s):
        raise ValueError("one line index per segment")
    par = planes_params(max_distance, junction_distance, junction_extension, min_angle, min_length, min_segments, max_planes,
                        max_tests, slice_chunks)
    h = C.c_void_p()
    rc = L.l3d_plane_segments(int(device), len(s), ptr(s), ptr(ln), C.byref(par), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"l3d_plane_segments failed [{rc}]: {_lib.last_error()}")
    return take_planes(h, obj_path)


def write_planes_obj(planes, path):
    """planes as detect_planes returns them -> an OBJ file, the bytes of l3d_planes_save_obj: per plane four "v x y z" at
    %.17g, its corners, and one "f i j k l" (1-based)"""
    with open(path, "w") as f:
        for k, p in enumerate(planes["planes"]):
            for c in p["corners"]:
                f.write("v %.17g %.17g %.17g\n" % (float(c[0]), float(c[1]), float(c[2])))
            f.write("f %d %d %d %d\n" % (4 * k + 1, 4 * k + 2, 4 * k + 3, 4 * k + 4))


def _sin2_of_degrees(angle, name):
    """sin(radians(angle))^2 for an angle in [0, 90] degrees (wireframe_params' degree rule)"""
    if not 0.0 <= float(angle) <= 90.0:
        raise ValueError(f"{name} must lie in [0, 90] degrees")
    sin = float(np.sin(np.radians(np.float64(angle))))
    return sin * sin


def directions_params(max_angle, min_length=0.0, min_segments=4, max_directions=16, max_tests=4096, frame_angle=5.0, frame_search=16,
                      slice_chunks=0):
    """l3d_directions_params from the wrappers' arguments: max_sin2 = sin^2(max_angle), max_frame_cos2 = sin^2(frame_angle)
    -- two directions are orthogonal when their angle is within frame_angle of 90 degrees --, both in degrees [0, 90]"""
    return _lib.DirectionsParams(_sin2_of_degrees(max_angle, "max_angle"), float(min_length), _sin2_of_degrees(frame_angle, "frame_angle"),
                                 int(min_segments), int(max_directions), int(max_tests), int(slice_chunks), int(frame_search), (0,) * 5)


def directions_summary_dict(s):
    """the summary as a dict; frame as a list of three, R as a list of nine (row-major)"""
    return {f: (list(getattr(s, f)) if f in ("frame", "R") else getattr(s, f)) for f, _ in _lib.DirectionsSummary._fields_}


def take_directions(handle, obj_path=None):
    """the arrays and the summary out of an l3d_directions handle, which is closed -> dict(directions: DIR_DIRECTION_DTYPE,
    members: DIR_MEMBER_DTYPE, seg_directions: uint32 per segment, scores: DIR_SCORE_DTYPE per hypothesis (= segment),
    summary: dict, R: [3, 3] float64 with p' = R p).  obj_path: l3d_directions_save_obj writes it first"""
    L = _lib.load()
    try:
        if obj_path is not None and L.l3d_directions_save_obj(handle, str(obj_path).encode()) != 0:
            raise RuntimeError(f"l3d_directions_save_obj failed: {_lib.last_error()}")
        n_d = C.c_uint64(); n_m = C.c_uint64(); n_h = C.c_uint64(); s = _lib.DirectionsSummary()
        L.l3d_directions_counts(handle, C.byref(n_d), C.byref(n_m), C.byref(n_h))
        L.l3d_directions_get(handle, None, None, None, None, C.byref(s))
        directions = np.zeros(max(n_d.value, 1), _lib.DIR_DIRECTION_DTYPE); members = np.zeros(max(n_m.value, 1), _lib.DIR_MEMBER_DTYPE)
        seg_directions = np.zeros(max(s.n_segments, 1), np.uint32); scores = np.zeros(max(n_h.value, 1), _lib.DIR_SCORE_DTYPE)
        L.l3d_directions_get(handle, ptr(directions), ptr(members), ptr(seg_directions), ptr(scores), None)
    finally:
        L.l3d_directions_close(handle)
    summary = directions_summary_dict(s)
    return dict(directions=directions[:n_d.value], members=members[:n_m.value], seg_directions=seg_directions[:s.n_segments],
                scores=scores[:n_h.value], summary=summary, R=np.array(summary["R"], np.float64).reshape(3, 3))


def detect_directions(segs, line, max_angle, min_length=0.0, min_segments=4, max_directions=16, max_tests=4096, frame_angle=5.0,
                      frame_search=16, slice_chunks=0, device=0, obj_path=None):
    """l3d_direction_segments: one model of 3D segments, segs [n, 6] float64 (P1, P2) with a line index each ->
    dict(directions, members, seg_directions, scores: arrays, summary: a dict, R: [3, 3]): the directions that at least
    min_segments segments of at least min_length in all run in, each within max_angle degrees of it, best-supported first,
    and the rotation R that turns the heaviest directions that are orthogonal within frame_angle degrees into the axes."""
    L = _lib.load()
    s = np.ascontiguousarray(segs, np.float64).reshape(-1, 6)
    ln = np.ascontiguousarray(line, np.uint32).reshape(-1)
    if len(ln) != len(s):
        raise ValueError("one line index per segment")
    par = directions_params(max_angle, min_length, min_segments, max_directions, max_tests, frame_angle, frame_search, slice_chunks)
    h = C.c_void_p()
    rc = L.l3d_direction_segments(int(device), len(s), ptr(s), ptr(ln), C.byref(par), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"l3d_direction_segments failed [{rc}]: {_lib.last_error()}")
    return take_directions(h, obj_path)


def write_directions_obj(directions, path):
    """directions as detect_directions returns them -> an OBJ file, the bytes of l3d_directions_save_obj: per direction two
    "v x y z" at %.17g, centroid + t_min D_fit and centroid + t_max D_fit, and one "l i j" (1-based)"""
    with open(path, "w") as f:
        for k, p in enumerate(directions["directions"]):
            c = [float(x) for x in p["centroid"]]; d = [float(x) for x in p["D_fit"]]
            for t in (float(p["t_min"]), float(p["t_max"])):
                f.write("v %.17g %.17g %.17g\n" % (c[0] + t * d[0], c[1] + t * d[1], c[2] + t * d[2]))
            f.write("l %d %d\n" % (2 * k + 1, 2 * k + 2))


def align_params(max_distance, start_distance=0.0, max_angle=10.0, min_overlap=0.5, step_tolerance=1e-9, max_iterations=50,
                 min_matches=8, estimate_scale=True, slice_chunks=0):
    """l3d_align_params from the wrappers' arguments, by compare_params' degree rule"""
    p = compare_params(max_distance, max_angle, min_overlap, False, slice_chunks)
    return _lib.AlignParams(p.max_distance, p.min_cos2, p.min_overlap, float(start_distance), float(step_tolerance),
                            int(max_iterations), int(min_matches), int(bool(estimate_scale)), p.slice_chunks, (0, 0))


def rotation_from_quaternion(q):
    """R(q) of a quaternion (w, x, y, z), divided by its norm first: the nine expressions of DESIGN §23"""
    q = np.asarray(q, np.float64).reshape(4)
    w, x, y, z = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def similarity_matrix(similarity):
    """a similarity dict (scale, q = (w, x, y, z), t) -> the 4x4 matrix [[scale R(q), t], [0, 0, 0, 1]]"""
    M = np.eye(4)
    M[:3, :3] = float(similarity["scale"]) * rotation_from_quaternion(similarity["q"])
    M[:3, 3] = np.asarray(similarity["t"], np.float64).reshape(3)
    return M


def similarity_from_matrix(M):
    """a 3x4 or 4x4 matrix [scale R, t] -> the similarity dict; ValueError where the left block is no scaled rotation"""
    M = np.asarray(M, np.float64)
    if M.shape not in ((3, 4), (4, 4)) or not np.isfinite(M).all():
        raise ValueError("a similarity is a finite 3x4 or 4x4 matrix")
    A = M[:3, :3]
    det = float(np.linalg.det(A))
    if not det > 0.0:
        raise ValueError("the matrix holds no rotation: its determinant is not positive")
    scale = det ** (1.0 / 3.0)
    R = A / scale
    if not np.allclose(R @ R.T, np.eye(3), atol=1e-6):
        raise ValueError("the matrix's left block is not a scaled rotation")
    # the largest of the four diagonal forms keeps the division away from zero
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cand = [tr, R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]]
    k = int(np.argmax(cand))
    r = np.sqrt(1.0 + cand[k])
    if k == 0:
        q = [0.5 * r, (R[2, 1] - R[1, 2]) / (2 * r), (R[0, 2] - R[2, 0]) / (2 * r), (R[1, 0] - R[0, 1]) / (2 * r)]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / (2 * r), 0.5 * r, (R[0, 1] + R[1, 0]) / (2 * r), (R[0, 2] + R[2, 0]) / (2 * r)]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / (2 * r), (R[0, 1] + R[1, 0]) / (2 * r), 0.5 * r, (R[1, 2] + R[2, 1]) / (2 * r)]
    else:
        q = [(R[1, 0] - R[0, 1]) / (2 * r), (R[0, 2] + R[2, 0]) / (2 * r), (R[1, 2] + R[2, 1]) / (2 * r), 0.5 * r]
    q = np.array(q)
    if q[0] < 0:
        q = -q
    return dict(scale=float(scale), q=q / np.linalg.norm(q), t=M[:3, 3].copy())


def similarity_from_points(src, dst, with_scale=True):
    """the similarity that maps the points src [n, 3] onto dst [n, 3] in the least-squares sense (Umeyama's closed form,
    numpy on the host): how a caller gets `initial` from corresponding camera centres or tie points -> similarity dict"""
    src = np.asarray(src, np.float64).reshape(-1, 3); dst = np.asarray(dst, np.float64).reshape(-1, 3)
    if len(src) != len(dst) or len(src) < 3:
        raise ValueError("three or more corresponding points on either side")
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2] = -1.0
    R = U @ np.diag(D) @ Vt
    var = (a * a).sum() / len(src)
    if not var > 0.0:
        raise ValueError("the source points coincide")
    scale = float((S * D).sum() / var) if with_scale else 1.0
    M = np.zeros((3, 4))
    M[:, :3] = scale * R
    M[:, 3] = md - scale * (R @ ms)
    out = similarity_from_matrix(M)
    out["scale"] = scale
    return out


def _similarity_struct(similarity):
    """None, a similarity dict or a 3x4 / 4x4 matrix -> a pointer argument for the C-ABI (None: identity)"""
    if similarity is None:
        return None
    if not isinstance(similarity, dict):
        similarity = similarity_from_matrix(similarity)
    q = np.asarray(similarity["q"], np.float64).reshape(4); t = np.asarray(similarity["t"], np.float64).reshape(3)
    return C.pointer(_lib.Similarity(float(similarity["scale"]), (C.c_double * 4)(*q), (C.c_double * 3)(*t)))


def similarity_dict(s):
    return dict(scale=float(s.scale), q=np.array(s.q[:], np.float64), t=np.array(s.t[:], np.float64))


def align_summary_dict(s):
    d = dict(status=ALIGN_STATUS[s.status], iterations=int(s.iterations), n_matched=int(s.n_matched), rms=float(s.rms),
             last_step=float(s.last_step), diag=float(s.diag), center=np.array(s.center[:], np.float64))
    return d


class _AlignOutputs:
    """the output arguments of l3d_align_segments / l3d_align_lines, and the dict the wrappers return from them"""

    def __init__(self, n_q, n_r, max_iterations):
        self.n_q, self.n_r = n_q, n_r
        self.similarity = _lib.Similarity(); self.summary = _lib.AlignSummary()
        self.segs = np.zeros((max(n_q, 1), 6), np.float64)
        self.mq = np.zeros(max(n_q, 1), LINE_MATCH_DTYPE); self.mr = np.zeros(max(n_r, 1), LINE_MATCH_DTYPE)
        self.trace = np.zeros(max(int(max_iterations), 1), ALIGN_ITERATION_DTYPE)

    def pointers(self):
        return (C.byref(self.similarity), C.byref(self.summary), ptr(self.segs), ptr(self.mq), ptr(self.mr), ptr(self.trace))

    def result(self):
        sim = similarity_dict(self.similarity)
        summary = align_summary_dict(self.summary)
        return dict(similarity=sim, matrix=similarity_matrix(sim), summary=summary, segments=self.segs[:self.n_q],
                    matches_q=self.mq[:self.n_q], matches_r=self.mr[:self.n_r], trace=self.trace[:summary["iterations"]])


def align_segments(q_segs, q_line, r_segs, r_line, max_distance, start_distance=0.0, initial=None, estimate_scale=True,
                   max_angle=10.0, min_overlap=0.5, step_tolerance=1e-9, max_iterations=50, min_matches=8, slice_chunks=0,
                   device=0):
    """l3d_align_segments: the similarity transform that moves the model Q onto the model R (segs [n, 6]
    float64 with a line index each), by iterated closest lines from `initial` (a similarity dict, a 3x4 / 4x4 matrix,
    None = identity) with the gate halving from start_distance down to max_distance -> a dict: similarity (scale, q, t),
    matrix (4x4), summary (status as a name, iterations, n_matched, rms, last_step, diag, center), segments (Q moved),
    matches_q / matches_r (LINE_MATCH_DTYPE, the aligned models compared at max_distance) and trace (one
    ALIGN_ITERATION_DTYPE entry per iteration)"""
    L = _lib.load()
    q = np.ascontiguousarray(q_segs, np.float64).reshape(-1, 6); r = np.ascontiguousarray(r_segs, np.float64).reshape(-1, 6)
    ql = np.ascontiguousarray(q_line, np.uint32).reshape(-1); rl = np.ascontiguousarray(r_line, np.uint32).reshape(-1)
    if len(ql) != len(q) or len(rl) != len(r):
        raise ValueError("one line index per segment")
    par = align_params(max_distance, start_distance, max_angle, min_overlap, step_tolerance, max_iterations, min_matches,
                       estimate_scale, slice_chunks)
    out = _AlignOutputs(len(q), len(r), par.max_iterations)
    rc = L.l3d_align_segments(int(device), len(q), ptr(q), ptr(ql), len(r), ptr(r), ptr(rl), C.byref(par), _similarity_struct(initial),
                              *out.pointers())
    if rc != 0:
        raise RuntimeError(f"l3d_align_segments failed [{rc}]: {_lib.last_error()}")
    return out.result()


def pose_params(max_distance=L3D_DEF_SCORING_POS_REGULARIZER, start_distance=0.0, max_angle=L3D_DEF_SCORING_ANG_REGULARIZER,
                min_overlap=0.5, stall_tolerance=1e-4, step_tolerance=1e-9, max_iterations=50, min_matches=8, near=1e-6):
    """l3d_pose_params from the wrappers' arguments, by associate_params' degree rule; the distances in pixels"""
    p = associate_params(max_distance, max_angle, min_overlap)
    return _lib.PoseParams(p.max_distance, p.min_cos2, p.min_overlap, float(start_distance), float(stall_tolerance),
                           float(step_tolerance), float(near), int(max_iterations), int(min_matches), (0, 0))


class _PoseOutputs:
    """the output arguments of l3d_refine_cameras / l3d_refine_view_cameras, and the dict the wrappers return from them"""

    def __init__(self, n_cams, n_seg_per_cam, max_iterations):
        self.n, self.n_seg, self.max_it = n_cams, [int(v) for v in n_seg_per_cam], int(max_iterations)
        self.cams = (_lib.Camera * max(n_cams, 1))()
        self.summaries = np.zeros(max(n_cams, 1), POSE_SUMMARY_DTYPE)
        self.assoc = np.zeros(max(sum(self.n_seg), 1), ASSOCIATION_DTYPE)
        self.trace = np.zeros(max(n_cams * self.max_it, 1), POSE_ITERATION_DTYPE)

    def result(self):
        s = self.summaries[:self.n]
        summaries = [dict(status=POSE_STATUS[int(v["status"])], iterations=int(v["iterations"]), n_matched=int(v["n_matched"]),
                          rms=float(v["rms"]), last_step=float(v["last_step"]), q=v["q"].copy(), t=v["t"].copy()) for v in s]
        trace = [self.trace[k * self.max_it:k * self.max_it + int(s["iterations"][k])].copy() for k in range(self.n)]
        return dict(cameras=[camera_dict(self.cams[k]) for k in range(self.n)], summaries=summaries,
                    associations=split_records(self.assoc, self.n_seg), trace=trace)


def _model_and_cameras(segs, line, cams, segs_per_cam):
    """the arguments that refine_cameras, refit_segments and bundle_segments share, as the library takes them -> the model
    [n, 6] float64 and its line indices, the float32 [M, 4] arrays per camera, their counts and their concatenation (each
    with one entry to spare, so that neither is empty) and the camera array"""
    s = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); ln = np.ascontiguousarray(line, np.uint32).reshape(-1)
    if len(ln) != len(s):
        raise ValueError("one line index per segment")
    if len(cams) != len(segs_per_cam):
        raise ValueError("one array of segments per camera")
    seg = [np.ascontiguousarray(v, np.float32).reshape(-1, 4) for v in segs_per_cam]
    n_seg = np.array([len(v) for v in seg] + [0], np.uint32)
    seg4 = np.concatenate(seg + [np.zeros((1, 4), np.float32)])
    return s, ln, seg, n_seg, seg4, camera_array(list(cams))


def refine_cameras(segs, line, cams, segs_per_cam, max_distance=L3D_DEF_SCORING_POS_REGULARIZER, start_distance=0.0,
                   max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, stall_tolerance=1e-4, step_tolerance=1e-9,
                   max_iterations=50, min_matches=8, near=1e-6, device=0):
    """l3d_refine_cameras: the poses of `cams` (dicts K, R, t, width, height; K stays fixed) refined against
    the model (segs [n, 6] float64 with a line index each) from each camera's 2D segments (segs_per_cam: one float32
    [M, 4] array per camera), by iterated closest lines with the gate halving from start_distance down to max_distance
    (pixels) whenever the step stalls -> a dict: cameras (the refined dicts), summaries (status as a name, iterations,
    n_matched, rms in pixels, last_step, the delta q and t), associations (one ASSOCIATION_DTYPE array per camera, of the
    refined camera at max_distance) and trace (one POSE_ITERATION_DTYPE array per camera)"""
    L = _lib.load()
    s, ln, seg, n_seg, seg4, arr = _model_and_cameras(segs, line, cams, segs_per_cam)
    par = pose_params(max_distance, start_distance, max_angle, min_overlap, stall_tolerance, step_tolerance, max_iterations,
                      min_matches, near)
    out = _PoseOutputs(len(cams), n_seg[:len(cams)], par.max_iterations)
    rc = L.l3d_refine_cameras(int(device), len(s), ptr(s), ptr(ln), len(cams), arr, ptr(n_seg), ptr(seg4), C.byref(par), out.cams,
                              ptr(out.summaries), ptr(out.assoc), ptr(out.trace))
    if rc != 0:
        raise RuntimeError(f"l3d_refine_cameras failed [{rc}]: {_lib.last_error()}")
    return out.result()


def refit_params(max_distance=L3D_DEF_SCORING_POS_REGULARIZER, max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5,
                 near=1e-6, min_length=0.0, visibility=L3D_DEF_MIN_VISIBILITY_T, max_iterations=50, use_ambiguous=False):
    """l3d_refit_params from the wrappers' arguments, by associate_params' degree rule; max_distance in pixels, min_length
    in world units"""
    p = associate_params(max_distance, max_angle, min_overlap)
    return _lib.RefitParams(p.max_distance, p.min_cos2, p.min_overlap, float(near), float(min_length), int(visibility),
                            int(max_iterations), int(bool(use_ambiguous)), (0, 0, 0))


def refit_summary_dict(s):
    return dict(n_lines=int(s.n_lines), status={name: int(s.n_status[k]) for k, name in enumerate(REFIT_STATUS)},
                n_observations=int(s.n_observations), n_ambiguous_left_out=int(s.n_ambiguous_left_out),
                n_segments_before=int(s.n_segments_before), n_segments_after=int(s.n_segments_after), cost0=float(s.cost0),
                cost1=float(s.cost1))


def _handle_counts(counts, h, n):
    """the first n counts of a result handle (l3d_refit_counts, l3d_bundle_counts)"""
    v = [C.c_uint64() for _ in range(n)]
    counts(h, *[C.byref(x) for x in v])
    return [int(x.value) for x in v]


def _line_arrays(ns, nl, no, na, line_dtype):
    """the arrays that l3d_refit_get and l3d_bundle_get fill first, none of them empty: segments, line, lines, observations,
    associations"""
    return (np.zeros((max(ns, 1), 6), np.float64), np.zeros(max(ns, 1), np.uint32), np.zeros(max(nl, 1), line_dtype),
            np.zeros(max(no, 1), REFIT_OBSERVATION_DTYPE), np.zeros(max(na, 1), ASSOCIATION_DTYPE))


def _lines_dict(arrays, ns, nl, no, na, n_seg_per_cam):
    """... cut to their counts, as the dict that take_refit and take_bundle share"""
    segs, line, lines, obs, assoc = arrays
    assoc = assoc[:na]
    return dict(segments=segs[:ns], line=line[:ns], lines=lines[:nl], observations=obs[:no],
                associations=split_records(assoc, n_seg_per_cam) if n_seg_per_cam is not None else assoc)


def take_refit(h, n_seg_per_cam):
    """the contents of an l3d_refit handle as a dict, and the handle closed: segments [n, 6] and line [n] (the output
    model), lines (REFIT_LINE_DTYPE, one per line index; `status` an index into REFIT_STATUS), observations
    (REFIT_OBSERVATION_DTYPE, line after line), associations (ASSOCIATION_DTYPE; one array per camera where the counts are
    known) and the summary"""
    L = _lib.load()
    try:
        n = _handle_counts(L.l3d_refit_counts, h, 4)
        arrays = _line_arrays(*n, REFIT_LINE_DTYPE)
        s = _lib.RefitSummary()
        L.l3d_refit_get(h, *[ptr(a) for a in arrays], C.byref(s))
    finally:
        L.l3d_refit_close(h)
    return dict(_lines_dict(arrays, *n, n_seg_per_cam), summary=refit_summary_dict(s))


def refit_segments(segs, line, cams, segs_per_cam, max_distance=L3D_DEF_SCORING_POS_REGULARIZER,
                   max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, near=1e-6, min_length=0.0,
                   visibility=L3D_DEF_MIN_VISIBILITY_T, max_iterations=50, use_ambiguous=False, device=0):
    """l3d_refit_segments: every line of the model (segs [n, 6] float64 with a line index each) re-estimated
    from the 2D segments that observe it in `cams` (dicts K, R, t, width, height; segs_per_cam: one float32 [M, 4] array
    per camera) and cut anew -> the dict of take_refit.  A line that is not REFIT keeps its segments bit for bit."""
    L = _lib.load()
    s, ln, seg, n_seg, seg4, arr = _model_and_cameras(segs, line, cams, segs_per_cam)
    par = refit_params(max_distance, max_angle, min_overlap, near, min_length, visibility, max_iterations, use_ambiguous)
    h = C.c_void_p()
    rc = L.l3d_refit_segments(int(device), len(s), ptr(s), ptr(ln), len(cams), arr, ptr(n_seg), ptr(seg4), C.byref(par), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"l3d_refit_segments failed [{rc}]: {_lib.last_error()}")
    return take_refit(h, [int(v) for v in n_seg[:len(cams)]])


def refine_model(segs, line, cams, segs_per_cam, rounds=3, max_distance=L3D_DEF_SCORING_POS_REGULARIZER, start_distance=0.0,
                 max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, near=1e-6, min_length=0.0,
                 visibility=L3D_DEF_MIN_VISIBILITY_T, pose_iterations=50, refit_iterations=50, min_matches=8,
                 stall_tolerance=1e-4, step_tolerance=1e-9, use_ambiguous=False, device=0):
    """cameras and lines refined in turn, K fixed (bundle adjustment over lines): every round is refine_cameras against the
    model as it stands, then refit_segments in the cameras just returned; start_distance applies in the first round only
    -> a dict: cameras, segments and line (the model after the last round), rounds (one (pose summaries, refit summary)
    pair per round) and the last round's refit dict as `refit`"""
    model, ml = np.ascontiguousarray(segs, np.float64).reshape(-1, 6), np.ascontiguousarray(line, np.uint32).reshape(-1)
    cams = list(cams)
    per_round, fit = [], None
    for r in range(int(rounds)):
        pose = refine_cameras(model, ml, cams, segs_per_cam, max_distance, start_distance if r == 0 else 0.0, max_angle, min_overlap,
                              stall_tolerance, step_tolerance, pose_iterations, min_matches, near, device)
        cams = pose["cameras"]
        fit = refit_segments(model, ml, cams, segs_per_cam, max_distance, max_angle, min_overlap, near, min_length, visibility,
                             refit_iterations, use_ambiguous, device)
        model, ml = fit["segments"], fit["line"]
        per_round.append((pose["summaries"], fit["summary"]))
    return dict(cameras=cams, segments=model, line=ml, rounds=per_round, refit=fit)


def bundle_params(max_distance=L3D_DEF_SCORING_POS_REGULARIZER, max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5,
                  near=1e-6, min_length=0.0, visibility=L3D_DEF_MIN_VISIBILITY_T, max_iterations=10, use_ambiguous=False,
                  initial_damping=1e-4, min_damping=1e-9, max_damping=1e8, function_tolerance=1e-6, capture_iteration=0):
    """l3d_bundle_params from the wrappers' arguments, by associate_params' degree rule; max_distance in pixels, min_length
    in world units"""
    p = associate_params(max_distance, max_angle, min_overlap)
    return _lib.BundleParams(p.max_distance, p.min_cos2, p.min_overlap, float(near), float(min_length), float(initial_damping),
                             float(min_damping), float(max_damping), float(function_tolerance), int(visibility),
                             int(max_iterations), int(bool(use_ambiguous)), int(capture_iteration), (0, 0, 0, 0))


def bundle_summary_dict(s):
    return dict(status=BUNDLE_STATUS[s.status], iterations=int(s.iterations), accepted_steps=int(s.accepted_steps),
                rejected_steps=int(s.rejected_steps), cost0=float(s.cost0), cost1=float(s.cost1), damping=float(s.damping),
                n_observations=int(s.n_observations), n_cells=int(s.n_cells), n_eligible_lines=int(s.n_eligible_lines),
                n_free_cameras=int(s.n_free_cameras), n_lines=int(s.n_lines),
                lines={name: int(s.n_status[k]) for k, name in enumerate(BUNDLE_LINE_STATUS)},
                n_ambiguous_left_out=int(s.n_ambiguous_left_out), n_segments_before=int(s.n_segments_before),
                n_segments_after=int(s.n_segments_after), captured=bool(s.captured))


def take_bundle(h, n_seg_per_cam):
    """the contents of an l3d_bundle handle as a dict, and the handle closed: segments [n, 6] and line [n] (the output
    model), lines (BUNDLE_LINE_DTYPE; `status` an index into BUNDLE_LINE_STATUS), observations (REFIT_OBSERVATION_DTYPE),
    associations, cameras (dicts), trace (BUNDLE_ITERATION_DTYPE), system [n, n] and rhs [n] of the captured iteration
    (None where none was kept) and the summary"""
    L = _lib.load()
    try:
        *n, nc, ni, nsys = _handle_counts(L.l3d_bundle_counts, h, 7)
        arrays = _line_arrays(*n, BUNDLE_LINE_DTYPE)
        cams = (_lib.Camera * max(nc, 1))(); trace = np.zeros(max(ni, 1), BUNDLE_ITERATION_DTYPE)
        system = np.zeros((max(nsys, 1), max(nsys, 1)), np.float64); rhs = np.zeros(max(nsys, 1), np.float64)
        s = _lib.BundleSummary()
        L.l3d_bundle_get(h, *[ptr(a) for a in arrays], cams, ptr(trace), ptr(system), ptr(rhs), C.byref(s))
    finally:
        L.l3d_bundle_close(h)
    return dict(_lines_dict(arrays, *n, n_seg_per_cam), cameras=[camera_dict(cams[k]) for k in range(nc)], trace=trace[:ni],
                system=system[:nsys, :nsys] if s.captured else None, rhs=rhs[:nsys] if s.captured else None,
                summary=bundle_summary_dict(s))


def _fixed_bytes(fixed, n):
    if fixed is None:
        return None
    f = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    if len(f) != n:
        raise ValueError("one byte of `fixed` per camera")
    return np.concatenate([f, np.zeros(1, np.uint8)])


def bundle_segments(segs, line, cams, segs_per_cam, fixed=None, max_distance=L3D_DEF_SCORING_POS_REGULARIZER,
                    max_angle=L3D_DEF_SCORING_ANG_REGULARIZER, min_overlap=0.5, near=1e-6, min_length=0.0,
                    visibility=L3D_DEF_MIN_VISIBILITY_T, max_iterations=10, use_ambiguous=False, initial_damping=1e-4,
                    min_damping=1e-9, max_damping=1e8, function_tolerance=1e-6, capture_iteration=0, device=0):
    """l3d_bundle_segments: one association of the model (segs [n, 6] float64 with a line index each) with the
    2D segments of `cams` (dicts K, R, t, width, height; segs_per_cam: one float32 [M, 4] array per camera), then
    Levenberg-Marquardt jointly over the poses of the cameras that are not `fixed` (one 0 / 1 per camera; None: none) and
    the lines that enough cameras see, and the lines' segments cut anew -> the dict of take_bundle"""
    L = _lib.load()
    s, ln, seg, n_seg, seg4, arr = _model_and_cameras(segs, line, cams, segs_per_cam)
    par = bundle_params(max_distance, max_angle, min_overlap, near, min_length, visibility, max_iterations, use_ambiguous,
                        initial_damping, min_damping, max_damping, function_tolerance, capture_iteration)
    fx = _fixed_bytes(fixed, len(cams))
    h = C.c_void_p()
    rc = L.l3d_bundle_segments(int(device), len(s), ptr(s), ptr(ln), len(cams), arr, ptr(fx) if fx is not None else None, ptr(n_seg),
                               ptr(seg4), C.byref(par), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"l3d_bundle_segments failed [{rc}]: {_lib.last_error()}")
    return take_bundle(h, [int(v) for v in n_seg[:len(cams)]])


def _rotation_of(q):
    """R(q) of a quaternion (w, x, y, z), normalised first"""
    w, x, y, z = (float(v) for v in np.asarray(q, np.float64) / np.linalg.norm(q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def transform_cameras(cams, similarity):
    """the cameras (dicts) that see a model moved by x' = s R_s x + t_s as they saw it before: R' = R R_s^T,
    t' = s t - R' t_s (K, width, height unchanged); numpy on the host -> a list of camera dicts"""
    if not isinstance(similarity, dict):
        similarity = similarity_from_matrix(similarity)
    Rs = _rotation_of(similarity["q"])
    ts = np.asarray(similarity["t"], np.float64).reshape(3); scale = float(similarity["scale"])
    out = []
    for c in cams:
        R = np.asarray(c["R"], np.float64).reshape(3, 3) @ Rs.T
        t = scale * np.asarray(c["t"], np.float64).reshape(3) - R @ ts
        out.append(dict(K=np.array(c["K"], np.float64).reshape(3, 3), R=R, t=t, width=int(c["width"]), height=int(c["height"])))
    return out


def camera_centres(cams):
    """[n, 3]: -R^T t of every camera dict"""
    return np.array([-(np.asarray(c["R"], np.float64).reshape(3, 3).T @ np.asarray(c["t"], np.float64).reshape(3)) for c in cams]).reshape(-1, 3)


def bundle_model(segs, line, cams, segs_per_cam, rounds=3, keep_gauge=True, fixed=None, **kw):
    """cameras and lines bundled jointly over `rounds` rounds: each round is one bundle_segments -- one
    association, then the joint solve on it -- on the previous round's cameras and model (kw: bundle_segments').  Nothing
    but the damping holds the 7-parameter gauge, so with keep_gauge and no fixed camera the driver finishes with the
    similarity that takes the new camera centres back onto the input's -- similarity_from_points' rotation, the scale and
    the translation that restore the centres' scatter and mean exactly --, applied to the model (transform_segments) and to
    the cameras (transform_cameras); with fewer than three cameras it skips that and says so
    -> a dict: cameras, segments, line, rounds (one summary per round), bundle (the last round's dict), gauge (the
    similarity applied, or None) and gauge_skipped (why not, or None)"""
    model, ml = np.ascontiguousarray(segs, np.float64).reshape(-1, 6), np.ascontiguousarray(line, np.uint32).reshape(-1)
    cams = list(cams)
    cams0 = cams
    per_round, fit = [], None
    for _ in range(int(rounds)):
        fit = bundle_segments(model, ml, cams, segs_per_cam, fixed, **kw)
        cams, model, ml = fit["cameras"], fit["segments"], fit["line"]
        per_round.append(fit["summary"])
    gauge, skipped = None, None
    if keep_gauge and fit is not None:
        if fixed is not None and np.any(np.asarray(fixed)):
            skipped = "a camera is fixed"
        elif len(cams) < 3:
            skipped = "fewer than three cameras"
        else:
            try:
                src, dst = camera_centres(cams), camera_centres(cams0)
                gauge = similarity_from_points(src, dst)
                # the rotation is the least-squares one; scale and translation are set so that the scatter and the mean of
                # the centres come back exactly (the least-squares scale falls short by the misfit)
                ms, md = src.mean(0), dst.mean(0)
                gauge["scale"] = math.sqrt(float(((dst - md) ** 2).sum()) / float(((src - ms) ** 2).sum()))
                gauge["t"] = md - gauge["scale"] * (_rotation_of(gauge["q"]) @ ms)
            except (ValueError, ZeroDivisionError, np.linalg.LinAlgError) as e:
                gauge, skipped = None, str(e)
        if gauge is not None:
            model = transform_segments(model, gauge)
            cams = transform_cameras(cams, gauge)
    return dict(cameras=cams, segments=model, line=ml, rounds=per_round, bundle=fit, gauge=gauge, gauge_skipped=skipped)


def transform_segments(segs, similarity):
    """l3d_transform_segments: segs [n, 6] under a similarity (dict or matrix), on the host by the function the device
    runs -> [n, 6] float64"""
    L = _lib.load()
    s = np.ascontiguousarray(segs, np.float64).reshape(-1, 6)
    out = np.zeros((max(len(s), 1), 6), np.float64)
    rc = L.l3d_transform_segments(len(s), ptr(s), _similarity_struct(similarity), ptr(out))
    if rc != 0:
        raise RuntimeError(f"l3d_transform_segments failed [{rc}]: {_lib.last_error()}")
    return out[:len(s)]


def render_line_maps(cams, records, thickness=1, device=0):
    """l3d_render_line_maps (stage 2): records = one PROJECTED_SEGMENT_DTYPE array per camera (of the cameras, width and
    height are read) -> [(line_id int32 [h, w], inv_depth float32 [h, w])]"""
    L = _lib.load()
    arr = camera_array(list(cams))
    n = len(cams)
    if len(records) != n:
        raise ValueError("one record array per camera")
    counts = np.array([len(r) for r in records] + [0], np.uint32)
    rec = np.ascontiguousarray(np.concatenate([np.asarray(r, PROJECTED_SEGMENT_DTYPE).reshape(-1) for r in records] +
                                              [np.zeros(1, PROJECTED_SEGMENT_DTYPE)]))
    ids = [np.empty((arr[i].height, arr[i].width), np.int32) for i in range(n)]
    izs = [np.empty((arr[i].height, arr[i].width), np.float32) for i in range(n)]
    rc = L.l3d_render_line_maps(int(device), n, arr, ptr(counts), ptr(rec), int(thickness), pointer_array(ids), pointer_array(izs))
    if rc != 0:
        raise RuntimeError(f"l3d_render_line_maps failed [{rc}]: {_lib.last_error()}")
    return list(zip(ids, izs))


def draw_line_maps(images, line_ids, alpha=255, colors=None, device=0):
    """l3d_draw_line_maps (stage 3): images uint8 HxW or HxWx3, line_ids int32 HxW per image -> list of uint8 HxWx3;
    colors: RGB triples by line index, None: the fixed palette"""
    L = _lib.load()
    imgs, keep = lsd.image_array(list(images))
    n = len(keep)
    if len(line_ids) != n:
        raise ValueError("one line-id plane per image")
    ids = [np.ascontiguousarray(p, np.int32) for p in line_ids]
    for i in range(n):
        if ids[i].shape != (imgs[i].rows, imgs[i].cols):
            raise ValueError(f"line-id plane {i} is not of its image's size")
    col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    outs = [np.empty((imgs[i].rows, imgs[i].cols, 3), np.uint8) for i in range(n)]
    rc = L.l3d_draw_line_maps(int(device), n, imgs, pointer_array(ids), 0 if col is None else len(col), ptr(col), int(alpha),
                              pointer_array(outs))
    if rc != 0:
        raise RuntimeError(f"l3d_draw_line_maps failed [{rc}]: {_lib.last_error()}")
    return outs


def match_lines(lines_src, lines_tgt, F, RtKinv_src, RtKinv_tgt, C_src, C_tgt, width, height, epi_overlap=0.25,
                kNN=10, device=0):
    """Seam-level call replacing match_lines_GPU (cudawrapper.h:54-63) with CPU-path semantics."""
    L = _lib.load()
    a = np.ascontiguousarray(lines_src, np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(lines_tgt, np.float32).reshape(-1, 4)
    arrs = [np.ascontiguousarray(x, np.float64) for x in (F, RtKinv_src, RtKinv_tgt, C_src, C_tgt)]
    out = np.zeros((len(a), kNN), SLOT_DTYPE)
    n = C.c_uint64()
    rc = L.l3d_match_lines(device, ptr(a), len(a), ptr(b), len(b), *[ptr(x) for x in arrs], width, height,
                           float(epi_overlap), int(kNN), ptr(out), C.byref(n))
    if rc != 0:
        raise RuntimeError(f"l3d_match_lines failed [{rc}]: {_lib.last_error()}")
    return out, n.value


def diffuse_affinity(edges, n_rows, iterations=10, device=0):
    """Seam-level call replacing the body of Line3D::performRDD (line3D.cc:2026-2076): replicator-dynamics
    diffusion of the affinity matrix + min-symmetrisation; returns the CLEdges in (i, j) order."""
    from ._lib import CLEDGE_DTYPE
    L = _lib.load()
    e = np.ascontiguousarray(edges, CLEDGE_DTYPE)
    out = np.zeros(len(e), CLEDGE_DTYPE)
    rc = L.l3d_diffuse_affinity(device, ptr(e), len(e), int(n_rows), int(iterations), ptr(out))
    if rc != 0:
        raise RuntimeError(f"l3d_diffuse_affinity failed [{rc}]: {_lib.last_error()}")
    return out


def triangulate_points(P, obs_offsets, obs_camera, obs_xy, device=0):
    """l3d_triangulate_points: main_pix4d.cpp's linear triangulation of tie points (linearHomTriangulation, :34-69) on
    the GPU.  P [n_cameras, 3, 4]; the observations of point i are obs_offsets[i] .. obs_offsets[i + 1] of obs_camera
    [n_obs] and obs_xy [n_obs, 2].  -> (X [n, 3] float64, valid [n] bool): valid = more than two observations and
    norm(X) > L3D_EPS; X is zero where not valid."""
    L = _lib.load()
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3, 4)
    off = np.ascontiguousarray(obs_offsets, np.uint64).reshape(-1)
    cam = np.ascontiguousarray(obs_camera, np.uint32).reshape(-1)
    xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    n = max(len(off) - 1, 0)
    if n and (int(off[-1]) > len(cam) or len(xy) != len(cam)):
        raise ValueError("obs_offsets, obs_camera and obs_xy do not describe the same observations")
    X = np.zeros((n, 3), np.float64)
    valid = np.zeros(n, np.uint8)
    rc = L.l3d_triangulate_points(int(device), len(P), ptr(P), n, ptr(off), ptr(cam), ptr(xy), ptr(X), ptr(valid))
    if rc != 0:
        raise RuntimeError(f"l3d_triangulate_points failed [{rc}]: {_lib.last_error()}")
    return X, valid.astype(bool)


def line_opt_solve(x0, res_off, obs, obs_cam, cams, max_iter=250, narrow_max=16, device=0):
    """l3d_line_opt_solve: the line bundling kernel's Levenberg-Marquardt solves on their own (k_lineopt.hip, through the
    function the pipeline's stage calls).  x0 [n, 4]; line i owns the residuals res_off[i] .. res_off[i + 1] of obs
    [n_res, 6] = (p1x, p1y, p2x, p2y, nx, ny) and obs_cam [n_res]; cams [n_cams, 16] = (R row-major, C, fx, fy, px, py).
    Lines with more than narrow_max (<= 16) residuals take a wave each, the others 16 lanes.
    -> (x [n, 4], cost0 [n], cost1 [n], iters [n], status [n]): 1 gradient, 2 function, 3 parameter, 4 max_iter, 5 other"""
    L = _lib.load()
    x0 = np.ascontiguousarray(x0, np.float64).reshape(-1, 4)
    off = np.ascontiguousarray(res_off, np.uint32).reshape(-1)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 6)
    cam = np.ascontiguousarray(obs_cam, np.uint32).reshape(-1)
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 16)
    n = len(x0)
    if len(off) != n + 1 or len(obs) != len(cam) or (n and int(off[-1]) > len(cam)):
        raise ValueError("x0, res_off, obs and obs_cam do not describe the same lines")
    x = np.zeros((n, 4), np.float64)
    cost = np.zeros((n, 2), np.float64)
    iters = np.zeros(n, np.uint32)
    status = np.zeros(n, np.uint32)
    rc = L.l3d_line_opt_solve(int(device), n, ptr(x0), ptr(off), ptr(obs), ptr(cam), len(cams), ptr(cams), int(max_iter),
                              int(narrow_max), ptr(x), ptr(cost), ptr(iters), ptr(status))
    if rc != 0:
        raise RuntimeError(f"l3d_line_opt_solve failed [{rc}]: {_lib.last_error()}")
    return x, cost[:, 0].copy(), cost[:, 1].copy(), iters, status


def find_collinear_segments(lines, dist_t, device=0):
    """Seam-level call replacing View::findCollinGPU / find_collinear_segments_GPU (view.cc:173-209) with the
    semantics of View::findCollinCPU: CSR (offsets[M+1], idx) of the collinear segments of every segment."""
    L = _lib.load()
    a = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
    off = np.zeros(len(a) + 1, np.uint32)
    n = C.c_uint64()
    rc = L.l3d_find_collinear_segments(device, ptr(a), len(a), float(dist_t), ptr(off), None, 0, C.byref(n))
    idx = np.zeros(max(n.value, 1), np.uint32)
    if rc == 0 and n.value:
        rc = L.l3d_find_collinear_segments(device, ptr(a), len(a), float(dist_t), ptr(off), ptr(idx), n.value, C.byref(n))
    if rc != 0:
        raise RuntimeError(f"l3d_find_collinear_segments failed [{rc}]: {_lib.last_error()}")
    return off, idx[:n.value]


def score_matches(lines, matches4, ranges2, reg_tgt2, RtKinv, C_, two_sigA_sqr, k, device=0):
    """Seam-level call replacing score_matches_GPU (cudawrapper.h:70-73) with the semantics of Line3D::scoringCPU;
    arrays as Line3D::scoringGPU marshals them (see include/l3dpp_hip.h)."""
    L = _lib.load()
    a = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
    m = np.ascontiguousarray(matches4, np.float32).reshape(-1, 4)
    r = np.ascontiguousarray(ranges2, np.int32).reshape(-1, 2)
    g = np.ascontiguousarray(reg_tgt2, np.float32).reshape(-1, 2)
    A = np.ascontiguousarray(RtKinv, np.float64); Cc = np.ascontiguousarray(C_, np.float64)
    out = np.zeros(len(m), np.float32)
    rc = L.l3d_score_matches(device, ptr(a), len(a), ptr(m), ptr(r), ptr(g), len(m), ptr(A), ptr(Cc),
                             float(two_sigA_sqr), float(k), ptr(out))
    if rc != 0:
        raise RuntimeError(f"l3d_score_matches failed [{rc}]: {_lib.last_error()}")
    return out


def neighbors_from_worldpoints(cams, K, R, t, worldpoints, num_neighbors=10):
    """Line3D::findVisualNeighborsFromWPs (line3D.cc:578-699) without a context or a GPU: cams = camera ids, K / R / t per
    camera as handed to addImage, worldpoints = one list of worldpoint ids per camera -> {cam: ascending neighbour ids}"""
    L = _lib.load()
    n = len(cams)
    ids = np.ascontiguousarray(cams, np.uint32)
    Ka = np.ascontiguousarray(K, np.float64).reshape(n, 9); Ra = np.ascontiguousarray(R, np.float64).reshape(n, 9)
    ta = np.ascontiguousarray(t, np.float64).reshape(n, 3)
    off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum([len(w) for w in worldpoints])
    wps = np.ascontiguousarray(np.concatenate([np.asarray(w, np.uint32) for w in worldpoints]) if off[-1] else np.zeros(1, np.uint32), np.uint32)
    nb_off = np.zeros(n + 1, np.uint64)
    rc = L.l3d_neighbors_from_worldpoints(n, ptr(ids), ptr(Ka), ptr(Ra), ptr(ta), ptr(off), ptr(wps), int(num_neighbors), ptr(nb_off), None, 0)
    if rc != 0:
        raise RuntimeError("l3d_neighbors_from_worldpoints: " + _lib.last_error())
    nb = np.zeros(max(int(nb_off[-1]), 1), np.uint32)
    rc = L.l3d_neighbors_from_worldpoints(n, ptr(ids), ptr(Ka), ptr(Ra), ptr(ta), ptr(off), ptr(wps), int(num_neighbors), ptr(nb_off), ptr(nb), len(nb))
    if rc != 0:
        raise RuntimeError("l3d_neighbors_from_worldpoints: " + _lib.last_error())
    return {int(c): nb[int(nb_off[i]):int(nb_off[i + 1])].copy() for i, c in enumerate(cams)}
