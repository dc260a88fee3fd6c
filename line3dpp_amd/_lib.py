"""ctypes binding of libl3dpp_hip.so (C-ABI: include/l3dpp_hip.h).

There is no CPU fallback: if the HIP library is missing this module raises, and every compute
entry point fails with L3D_ERR_HIP when no MI355X/HIP device is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "csrc", "libl3dpp_hip.so")
# L3D_LIB=<path>: load another build of the same library (diagnostic builds with -DL3D_STATS / -DL3D_CYCLES)
SO_PATH = os.environ.get("L3D_LIB", SO_PATH)

# reference PODs (include/l3dpp_hip.h)
MATCH_DTYPE = np.dtype([
    ("src_cam", "<u4"), ("src_seg", "<u4"), ("tgt_cam", "<u4"), ("tgt_seg", "<u4"),
    ("overlap", "<f4"), ("score3D", "<f4"),
    ("d_p1", "<f4"), ("d_p2", "<f4"), ("d_q1", "<f4"), ("d_q2", "<f4")])
SEGMENT2D_DTYPE = np.dtype([("cam", "<u4"), ("seg", "<u4")])
SEGMENT3D_DTYPE = np.dtype([("P1", "<f8", 3), ("P2", "<f8", 3), ("dir", "<f8", 3), ("length", "<f4"), ("valid", "<u4")])
CLEDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("w", "<f4")])
SLOT_DTYPE = np.dtype([
    ("tgt_seg", "<u4"), ("overlap", "<f4"), ("d_p1", "<f4"), ("d_p2", "<f4"), ("d_q1", "<f4"), ("d_q2", "<f4"),
    ("score3D", "<f4"), ("flags", "<u4")])
FLOAT4_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")])
# l3d_projected_segment: a 3D segment as a camera sees it; flag bits in `segment`
PROJECTED_SEGMENT_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("inv_depth1", "<f4"),
                                    ("inv_depth2", "<f4"), ("line", "<u4"), ("segment", "<u4")])
PROJ_CLIPPED_NEAR, PROJ_CLIPPED_RECT, PROJ_SEGMENT_MASK = 0x80000000, 0x40000000, 0x3FFFFFFF
assert MATCH_DTYPE.itemsize == 40 and SLOT_DTYPE.itemsize == 32 and SEGMENT3D_DTYPE.itemsize == 80
assert PROJECTED_SEGMENT_DTYPE.itemsize == 32
# l3d_association: the record a 2D segment was assigned; record = -1, line = segment = EMPTY: none
ASSOCIATION_DTYPE = np.dtype([("record", "<i4"), ("line", "<u4"), ("segment", "<u4"), ("distance", "<f4"),
                              ("overlap", "<f4"), ("n_accepted", "<u4")])
assert ASSOCIATION_DTYPE.itemsize == 24
# l3d_line_match: the reference segment a 3D query segment was assigned; segment = -1, line = EMPTY: none
LINE_MATCH_DTYPE = np.dtype([("segment", "<i4"), ("line", "<u4"), ("n_accepted", "<u4"), ("overlap", "<f4"),
                             ("distance", "<f8")])
assert LINE_MATCH_DTYPE.itemsize == 24
# l3d_similarity and l3d_align_iteration: one entry of an alignment's trace
SIMILARITY_DTYPE = np.dtype([("scale", "<f8"), ("q", "<f8", 4), ("t", "<f8", 3)])
ALIGN_ITERATION_DTYPE = np.dtype([("gate", "<f8"), ("sums", "<f8", 37), ("delta", "<f8", 7), ("similarity", SIMILARITY_DTYPE),
                                  ("n_matched", "<u8")])
assert SIMILARITY_DTYPE.itemsize == 64 and ALIGN_ITERATION_DTYPE.itemsize == 432
ALIGN_STATUS = ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW", "DEGENERATE")
# l3d_pose_summary and l3d_pose_iteration: a refined camera's summary, one entry of its trace
POSE_SUMMARY_DTYPE = np.dtype([("status", "<u4"), ("iterations", "<u4"), ("n_matched", "<u8"), ("rms", "<f8"), ("last_step", "<f8"),
                               ("q", "<f8", 4), ("t", "<f8", 3)])
POSE_ITERATION_DTYPE = np.dtype([("gate", "<f8"), ("sums", "<f8", 29), ("delta", "<f8", 6), ("R", "<f8", 9), ("t", "<f8", 3),
                                 ("n_matched", "<u8")])
assert POSE_SUMMARY_DTYPE.itemsize == 88 and POSE_ITERATION_DTYPE.itemsize == 392
POSE_STATUS = ALIGN_STATUS
# l3d_refit_line, l3d_refit_observation: a line of a refit model, a 2D segment that observes one
REFIT_LINE_DTYPE = np.dtype([("status", "<u4"), ("n_observations", "<u4"), ("n_views", "<u4"), ("solver_status", "<u4"),
                             ("iterations", "<u4"), ("n_pieces", "<u4"), ("cost0", "<f8"), ("cost1", "<f8"), ("x0", "<f8", 4),
                             ("x", "<f8", 4), ("P1", "<f8", 3), ("P2", "<f8", 3)])
REFIT_OBSERVATION_DTYPE = np.dtype([("camera", "<u4"), ("segment", "<u4"), ("line", "<u4"), ("valid", "<u4"), ("s_lo", "<f8"),
                                    ("s_hi", "<f8")])
assert REFIT_LINE_DTYPE.itemsize == 152 and REFIT_OBSERVATION_DTYPE.itemsize == 32
REFIT_STATUS = ("REFIT", "TOO_FEW_VIEWS", "CONSTANT", "FAILED", "NO_EXTENT", "EMPTY")
# l3d_bundle_line, l3d_bundle_iteration: a line of a bundled model, one iteration of a call's trace
BUNDLE_LINE_DTYPE = np.dtype([("status", "<u4"), ("n_observations", "<u4"), ("n_views", "<u4"), ("n_pieces", "<u4"),
                              ("P1", "<f8", 3), ("P2", "<f8", 3)])
BUNDLE_ITERATION_DTYPE = np.dtype([("damping", "<f8"), ("cost", "<f8"), ("cost_trial", "<f8"), ("step_cameras", "<f8"),
                                   ("step_lines", "<f8"), ("solved", "<u4"), ("accepted", "<u4"), ("n_held_for_step", "<u4"),
                                   ("pad", "<u4")])
assert BUNDLE_LINE_DTYPE.itemsize == 64 and BUNDLE_ITERATION_DTYPE.itemsize == 56
BUNDLE_LINE_STATUS = ("BUNDLED", "HELD", "NO_EXTENT", "EMPTY")
BUNDLE_STATUS = ("CONVERGED", "MAX_ITERATIONS", "STALLED", "NO_VARIABLES")
# l3d_merge_line_info: one line of a merged model
MERGE_LINE_INFO_DTYPE = np.dtype([("n_members", "<u4"), ("label", "<u4"), ("max_offset", "<f8")])
assert MERGE_LINE_INFO_DTYPE.itemsize == 16
# l3d_wf_junction, l3d_wf_vertex, l3d_wf_edge: the wireframe of a model
WF_JUNCTION_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("kind", "<u4"), ("class_a", "<u4"), ("class_b", "<u4"), ("vertex", "<u4"),
                              ("sa", "<f8"), ("sb", "<f8"), ("gap", "<f8"), ("J", "<f8", 3)])
WF_VERTEX_DTYPE = np.dtype([("P", "<f8", 3), ("spread", "<f8"), ("n_junctions", "<u4"), ("kinds", "<u4"), ("degree", "<u4"),
                            ("component", "<u4")])
WF_EDGE_DTYPE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("segment", "<u4"), ("line", "<u4")])
assert WF_JUNCTION_DTYPE.itemsize == 72 and WF_VERTEX_DTYPE.itemsize == 48 and WF_EDGE_DTYPE.itemsize == 16
# l3d_pl_plane, l3d_pl_member, l3d_pl_score: the planes of a model
PL_PLANE_DTYPE = np.dtype([("hypothesis", "<u4"), ("a", "<u4"), ("b", "<u4"), ("n_segments", "<u4"), ("n_lines", "<u4"), ("reserved", "<u4"),
                           ("weight", "<u8"), ("N", "<f8", 3), ("J", "<f8", 3), ("d", "<f8"), ("length", "<f8"), ("rms", "<f8"),
                           ("centroid", "<f8", 3), ("N_fit", "<f8", 3), ("d_fit", "<f8"), ("rms_fit", "<f8"), ("corners", "<f8", (4, 3))])
PL_MEMBER_DTYPE = np.dtype([("plane", "<u4"), ("segment", "<u4")])
PL_SCORE_DTYPE = np.dtype([("weight", "<u8"), ("count", "<u4"), ("reserved", "<u4")])
assert PL_PLANE_DTYPE.itemsize == 264 and PL_MEMBER_DTYPE.itemsize == 8 and PL_SCORE_DTYPE.itemsize == 16
# l3d_dir_direction, l3d_dir_member, l3d_dir_score: the directions of a model
DIR_DIRECTION_DTYPE = np.dtype([("hypothesis", "<u4"), ("n_segments", "<u4"), ("n_lines", "<u4"), ("reserved", "<u4"), ("weight", "<u8"),
                                ("D", "<f8", 3), ("length", "<f8"), ("rms_sin", "<f8"), ("D_fit", "<f8", 3), ("rms_sin_fit", "<f8"),
                                ("centroid", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
DIR_MEMBER_DTYPE = np.dtype([("direction", "<u4"), ("segment", "<u4")])
DIR_SCORE_DTYPE = np.dtype([("weight", "<u8"), ("count", "<u4"), ("reserved", "<u4")])
assert DIR_DIRECTION_DTYPE.itemsize == 136 and DIR_MEMBER_DTYPE.itemsize == 8 and DIR_SCORE_DTYPE.itemsize == 16
WF_L, WF_T, WF_X = 1, 2, 4                      # kind of a junction, the bits of a vertex's kinds
WF_AT_P1, WF_AT_P2, WF_INTERIOR = 0, 1, 2       # class_a, class_b
EMPTY = 0xFFFFFFFF
L3D_ERR_NO_SEGMENTS = -5
L3D_ERR_IO = -11


class MatchParams(C.Structure):
    _fields_ = [("sigma_position", C.c_float), ("sigma_angle", C.c_float), ("num_neighbors", C.c_uint32),
                ("epipolar_overlap", C.c_float), ("kNN", C.c_int32), ("const_regularization_depth", C.c_float)]


class NvmCamera(C.Structure):
    """l3d_nvm_camera (include/l3dpp_hip.h)"""
    _fields_ = [("filename", C.c_char_p), ("focal", C.c_float), ("distortion", C.c_float), ("median_depth", C.c_float),
                ("n_worldpoints", C.c_uint32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("C", C.c_double * 3)]


class SfmImage(C.Structure):
    """l3d_sfm_image (include/l3dpp_hip.h)"""
    _fields_ = [("id", C.c_uint32), ("camera", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("name", C.c_char_p), ("focal", C.c_float), ("median_depth", C.c_float), ("n_worldpoints", C.c_uint32),
                ("K", C.c_double * 9), ("R", C.c_double * 9), ("t", C.c_double * 3), ("C", C.c_double * 3),
                ("radial", C.c_double * 3), ("tangential", C.c_double * 2)]


class Timings(C.Structure):
    _fields_ = [("begin_ms", C.c_float), ("match_pairs_ms", C.c_float), ("finish_ms", C.c_float),
                ("affinity_ms", C.c_float), ("match_kernel_launches", C.c_uint32), ("match_kernel_ms", C.c_float),
                ("cull_prepare_ms", C.c_float), ("culled_pairs", C.c_uint32),
                ("list_entries", C.c_uint32), ("support_words", C.c_uint32), ("tied_rows", C.c_uint32), ("chain_sweeps", C.c_uint32),
                ("chain_extra_rounds", C.c_uint32), ("pool_retries", C.c_uint32),
                ("lists_ms", C.c_float), ("record_kbytes", C.c_uint32),
                ("list_inverse", C.c_uint32), ("list_candidates", C.c_uint32), ("list_headers", C.c_uint32),
                ("slots_lo", C.c_uint32), ("slots_hi", C.c_uint32)]


class MatchPlanInfo(C.Structure):
    """l3d_match_plan_info (include/l3dpp_hip.h)"""
    _fields_ = [("tier", C.c_uint32), ("waves", C.c_uint32), ("row_cache", C.c_uint32), ("ix16", C.c_uint32),
                ("lds_bytes", C.c_uint64), ("replay", C.c_uint32), ("launch_accepted", C.c_uint32)]


class LineOptStats(C.Structure):
    """l3d_line_opt_summary (include/l3dpp_hip.h)"""
    _fields_ = [("lines_bundled", C.c_uint32), ("lines_constant", C.c_uint32), ("lines_dropped", C.c_uint32),
                ("stop_gradient", C.c_uint32), ("stop_function", C.c_uint32), ("stop_parameter", C.c_uint32),
                ("stop_max_iter", C.c_uint32), ("stop_other", C.c_uint32), ("max_iterations", C.c_uint32),
                ("residuals", C.c_uint32), ("lines_wide", C.c_uint32), ("max_residuals", C.c_uint32),
                ("cost_before", C.c_double), ("cost_after", C.c_double), ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


class Image(C.Structure):
    """l3d_image (include/l3dpp_hip.h)"""
    _fields_ = [("data", C.c_void_p), ("cols", C.c_uint32), ("rows", C.c_uint32), ("channels", C.c_uint32),
                ("row_stride", C.c_uint32)]


class DetectOptions(C.Structure):
    """l3d_detect_options (include/l3dpp_hip.h)"""
    _fields_ = [("output_folder", C.c_char_p), ("load_segments", C.c_int32), ("max_image_width", C.c_int32),
                ("max_line_segments", C.c_uint32)]


class Distortion(C.Structure):
    """l3d_distortion (include/l3dpp_hip.h): the arguments of Line3D::undistortImage"""
    _fields_ = [("K", C.c_double * 9), ("radial", C.c_double * 3), ("tangential", C.c_double * 2)]


# L3D_CAM_* (include/l3dpp_hip.h) by COLMAP's model name, and the number of distortion parameters each takes
CAMERA_MODELS = {"FULL_OPENCV": 1, "OPENCV_FISHEYE": 2, "SIMPLE_RADIAL_FISHEYE": 3, "RADIAL_FISHEYE": 4, "FOV": 5}
CAMERA_MODEL_PARAMS = {"FULL_OPENCV": 8, "OPENCV_FISHEYE": 4, "SIMPLE_RADIAL_FISHEYE": 1, "RADIAL_FISHEYE": 2, "FOV": 1}


class CameraModel(C.Structure):
    """l3d_camera_model (include/l3dpp_hip.h): the arguments of undistortion by camera model"""
    _fields_ = [("model", C.c_uint32), ("reserved", C.c_uint32), ("K", C.c_double * 9), ("params", C.c_double * 8),
                ("K_new", C.c_double * 9)]


class Camera(C.Structure):
    """l3d_camera (include/l3dpp_hip.h): a pinhole camera of the projection stages, K and R row-major"""
    _fields_ = [("K", C.c_double * 9), ("R", C.c_double * 9), ("t", C.c_double * 3), ("width", C.c_uint32),
                ("height", C.c_uint32)]


class ProjectedSegment(C.Structure):
    """l3d_projected_segment (include/l3dpp_hip.h) = PROJECTED_SEGMENT_DTYPE"""
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float), ("inv_depth1", C.c_float),
                ("inv_depth2", C.c_float), ("line", C.c_uint32), ("segment", C.c_uint32)]


class AssociateParams(C.Structure):
    """l3d_associate_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double)]


class CompareParams(C.Structure):
    """l3d_compare_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double),
                ("exclude_same_line", C.c_uint32), ("slice_chunks", C.c_uint32)]


class CompareSummary(C.Structure):
    """l3d_compare_summary (include/l3dpp_hip.h)"""
    _fields_ = [("n_segments", C.c_uint64), ("n_matched", C.c_uint64), ("n_ambiguous", C.c_uint64), ("n_lines", C.c_uint64),
                ("n_lines_matched", C.c_uint64), ("length_total", C.c_double), ("length_matched", C.c_double)]


class MergeParams(C.Structure):
    """l3d_merge_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double),
                ("slice_chunks", C.c_uint32), ("reserved", C.c_uint32)]


class MergeSummary(C.Structure):
    """l3d_merge_summary (include/l3dpp_hip.h)"""
    _fields_ = [("n_segments_in", C.c_uint64), ("n_segments_out", C.c_uint64), ("n_lines_in", C.c_uint64),
                ("n_lines_out", C.c_uint64), ("n_pairs", C.c_uint64), ("n_merged_components", C.c_uint64),
                ("largest_component", C.c_uint64), ("length_in", C.c_double), ("length_out", C.c_double),
                ("max_offset", C.c_double)]


class WireframeParams(C.Structure):
    """l3d_wireframe_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("max_extension", C.c_double), ("min_sin2", C.c_double),
                ("slice_chunks", C.c_uint32), ("reserved", C.c_uint32)]


class WireframeSummary(C.Structure):
    """l3d_wireframe_summary (include/l3dpp_hip.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n_segments", "n_point_segments", "n_junctions", "n_L", "n_T", "n_X", "n_vertices",
                                          "n_junction_vertices", "n_free_ends", "n_edges", "n_components", "largest_component")] + \
        [(n, C.c_double) for n in ("length_total", "max_gap", "max_spread")]


class PlanesParams(C.Structure):
    """l3d_planes_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("junction_distance", C.c_double), ("junction_extension", C.c_double),
                ("min_sin2", C.c_double), ("min_length", C.c_double), ("min_segments", C.c_uint32), ("max_planes", C.c_uint32),
                ("max_tests", C.c_uint32), ("slice_chunks", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PlanesSummary(C.Structure):
    """l3d_planes_summary (include/l3dpp_hip.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n_segments", "n_point_segments", "n_hypotheses", "n_dead", "n_candidates", "n_tested",
                                          "n_dropped", "n_rejected", "n_planes", "n_memberships", "n_segments_in_planes",
                                          "n_segments_in_several", "truncated")] + [("scale_exponent", C.c_int64)] + \
        [(n, C.c_double) for n in ("length_total", "length_in_planes", "max_rms")]


class DirectionsParams(C.Structure):
    """l3d_directions_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_sin2", C.c_double), ("min_length", C.c_double), ("max_frame_cos2", C.c_double), ("min_segments", C.c_uint32),
                ("max_directions", C.c_uint32), ("max_tests", C.c_uint32), ("slice_chunks", C.c_uint32), ("frame_search", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]


class DirectionsSummary(C.Structure):
    """l3d_directions_summary (include/l3dpp_hip.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n_segments", "n_point_segments", "n_candidates", "n_tested", "n_dropped", "n_rejected",
                                          "n_directions", "n_memberships", "n_segments_in_directions", "n_segments_in_several",
                                          "truncated")] + [("scale_exponent", C.c_int64)] + \
        [(n, C.c_double) for n in ("length_total", "length_in_directions")] + \
        [("frame_axes", C.c_uint32), ("frame", C.c_uint32 * 3), ("R", C.c_double * 9)]


class Similarity(C.Structure):
    """l3d_similarity (include/l3dpp_hip.h): y = scale * R(q) x + t, q = (w, x, y, z)"""
    _fields_ = [("scale", C.c_double), ("q", C.c_double * 4), ("t", C.c_double * 3)]


class AlignParams(C.Structure):
    """l3d_align_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double),
                ("start_distance", C.c_double), ("step_tolerance", C.c_double), ("max_iterations", C.c_uint32),
                ("min_matches", C.c_uint32), ("estimate_scale", C.c_uint32), ("slice_chunks", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class PoseParams(C.Structure):
    """l3d_pose_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double),
                ("start_distance", C.c_double), ("stall_tolerance", C.c_double), ("step_tolerance", C.c_double),
                ("near_plane", C.c_double), ("max_iterations", C.c_uint32), ("min_matches", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class RefitParams(C.Structure):
    """l3d_refit_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double), ("near_plane", C.c_double),
                ("min_length", C.c_double), ("visibility", C.c_uint32), ("max_iterations", C.c_uint32),
                ("use_ambiguous", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class RefitSummary(C.Structure):
    """l3d_refit_summary (include/l3dpp_hip.h)"""
    _fields_ = [("n_lines", C.c_uint64), ("n_status", C.c_uint64 * 6), ("n_observations", C.c_uint64),
                ("n_ambiguous_left_out", C.c_uint64), ("n_segments_before", C.c_uint64), ("n_segments_after", C.c_uint64),
                ("cost0", C.c_double), ("cost1", C.c_double)]


class BundleParams(C.Structure):
    """l3d_bundle_params (include/l3dpp_hip.h)"""
    _fields_ = [("max_distance", C.c_double), ("min_cos2", C.c_double), ("min_overlap", C.c_double), ("near_plane", C.c_double),
                ("min_length", C.c_double), ("initial_damping", C.c_double), ("min_damping", C.c_double),
                ("max_damping", C.c_double), ("function_tolerance", C.c_double), ("visibility", C.c_uint32),
                ("max_iterations", C.c_uint32), ("use_ambiguous", C.c_uint32), ("capture_iteration", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class BundleSummary(C.Structure):
    """l3d_bundle_summary (include/l3dpp_hip.h)"""
    _fields_ = [("status", C.c_uint32), ("iterations", C.c_uint32), ("accepted_steps", C.c_uint32), ("rejected_steps", C.c_uint32),
                ("cost0", C.c_double), ("cost1", C.c_double), ("damping", C.c_double), ("n_observations", C.c_uint64),
                ("n_cells", C.c_uint64), ("n_eligible_lines", C.c_uint64), ("n_free_cameras", C.c_uint64), ("n_lines", C.c_uint64),
                ("n_status", C.c_uint64 * 4), ("n_ambiguous_left_out", C.c_uint64), ("n_segments_before", C.c_uint64),
                ("n_segments_after", C.c_uint64), ("captured", C.c_uint32), ("reserved", C.c_uint32)]


class AlignSummary(C.Structure):
    """l3d_align_summary (include/l3dpp_hip.h)"""
    _fields_ = [("status", C.c_uint32), ("iterations", C.c_uint32), ("n_matched", C.c_uint64), ("rms", C.c_double),
                ("last_step", C.c_double), ("diag", C.c_double), ("center", C.c_double * 3)]


class DetectStats(C.Structure):
    """l3d_detect_stats (include/l3dpp_hip.h)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("raw_segments", C.c_uint32), ("segments", C.c_uint32),
                ("from_cache", C.c_uint32), ("seeds", C.c_uint32), ("nfa_evals", C.c_uint32), ("reserved", C.c_uint32),
                ("max_grad", C.c_double)]


class LsdStages(C.Structure):
    """l3d_lsd_stages (include/l3dpp_hip.h): sizes out, host buffers in, the kernel's result record out"""
    _fields_ = [("gw", C.c_uint32), ("gh", C.c_uint32), ("sw", C.c_uint32), ("sh", C.c_uint32), ("down", C.c_uint32),
                ("raw_cap", C.c_uint32), ("gray", C.c_void_p), ("small_gray", C.c_void_p), ("blur", C.c_void_p),
                ("deg", C.c_void_p), ("mod", C.c_void_p), ("raw4", C.c_void_p), ("raw_segments", C.c_uint32),
                ("overflow", C.c_uint32), ("seeds", C.c_uint32), ("nfa_evals", C.c_uint32),
                ("max_grad_bits", C.c_ulonglong), ("stats", DetectStats)]


class TailRecords(C.Structure):
    """l3d_tail_records (include/l3dpp_hip.h): sizes out, host buffers in"""
    SIZES = ("G", "V", "pools", "ecap", "hcap", "scap", "n_headers", "n_edges", "n_segs", "n_surv", "n_hyps", "reserved")
    BUFFERS = ("seg_base", "hdr_words", "hdr_pool", "hdr_index", "hdr_positive", "edge_words", "edge_index", "edge_positive",
               "seg_words", "max_score_bits", "kept_cnt", "best_pack", "off64s", "surv_off", "hyp_off", "hyp_of_seg",
               "surv_sg", "surv_tg", "depths", "medians")
    _fields_ = [(n, C.c_uint32) for n in SIZES] + [("n_slots", C.c_uint64)] + [(n, C.c_void_p) for n in BUFFERS]


class AffinityRecords(C.Structure):
    """l3d_affinity_records (include/l3dpp_hip.h): sizes and scalars out, host buffers in"""
    SIZES = ("N", "H", "G", "V", "n_cand", "mode", "diffused", "n_edges", "n_rows", "epos_total", "touch_total", "n_coll",
             "n_child", "n_own")
    BUFFERS = ("view_k", "msdl_dev", "medians", "hyps", "surv_off", "surv_sg", "surv_tg", "hyp_of_seg", "simv", "cand_a",
               "cand_b", "flag", "epos", "first_touch", "touch_flag", "touch_rank", "edges", "l2g", "coll_off", "coll_idx",
               "child_off", "child_seg", "child_sim", "own_off", "own_seg", "own_sim")
    _fields_ = [(n, C.c_uint32) for n in SIZES] + [("two_sigA_sqr", C.c_float), ("med_scene_depth_lines", C.c_float)] + \
        [(n, C.c_void_p) for n in BUFFERS]


class KeepRows(C.Structure):
    """l3d_keep_rows (include/l3dpp_hip.h): sizes out, host buffers in"""
    SIZES = ("n_rows", "n_pairs", "n_blocks", "keep_cap", "tgt16", "reserved")
    BUFFERS = ("row_start", "row_pair", "blk_row", "pair_info", "slot_row", "inv_tgt")
    _fields_ = [(n, C.c_uint32) for n in SIZES] + [("n_slots", C.c_uint64)] + [(n, C.c_void_p) for n in BUFFERS]


class CullFormsInfo(C.Structure):
    """l3d_cull_forms_info (include/l3dpp_hip.h)"""
    _fields_ = [("enabled", C.c_uint32), ("reserved", C.c_uint32), ("As", C.c_double * 3), ("Bs", C.c_double * 3),
                ("At", C.c_double * 3), ("Bt", C.c_double * 3)]


class CullState(C.Structure):
    """l3d_cull_state (include/l3dpp_hip.h): sizes and forms out, host buffers in"""
    SIZES = ("enabled", "layout_rows", "Ms", "Mt", "src_len", "n_chunks")
    FORMS = ("As", "Bs", "At", "Bt")
    BUFFERS = ("src_perm", "src_band", "tgt_perm", "tgt_band", "chunk_band")
    _fields_ = [(n, C.c_uint32) for n in SIZES] + [(n, C.c_double * 3) for n in FORMS] + [(n, C.c_void_p) for n in BUFFERS]


# l3d_dev.h: HypRec (128 bytes) as l3d_debug_affinity_records hands it out
HYP_REC_DTYPE = np.dtype([("P1", "<f8", 3), ("P2", "<f8", 3), ("dir", "<f8", 3), ("length", "<f4"), ("valid", "<u4"),
                          ("m", MATCH_DTYPE), ("view", "<u4"), ("pad", "<u4")])
assert HYP_REC_DTYPE.itemsize == 128


# l3d_lists.h: HypHdr (64 bytes), EdgeRec (16), SegHdr (16) as the hook hands them out
HYP_HDR_DTYPE = np.dtype([("g", "<u4"), ("ref", "<u4"), ("pair_flags", "<u4"), ("canon", "<u4"), ("dp1", "<f4"), ("dp2", "<f4"),
                          ("edge_begin", "<u4"), ("edge_cnt", "<u4"), ("score3D", "<f4"), ("state", "<u4"), ("tgt_seg", "<u4"),
                          ("overlap", "<f4"), ("oq1", "<f4"), ("oq2", "<f4"), ("pad", "<u4", 2)])
EDGE_REC_DTYPE = np.dtype([("ref_j", "<u4"), ("sim", "<f4"), ("j_cam", "<u4"), ("tv_j", "<u4")])
SEG_HDR_DTYPE = np.dtype([("g", "<u4"), ("hyp_begin", "<u4"), ("hyp_cnt", "<u4"), ("pad", "<u4")])
assert HYP_HDR_DTYPE.itemsize == 64 and EDGE_REC_DTYPE.itemsize == 16 and SEG_HDR_DTYPE.itemsize == 16


EXPORTS = [
    "l3d_last_error", "l3d_build_info", "l3d_create", "l3d_destroy", "l3d_add_view", "l3d_match_images",
    "l3d_match_begin", "l3d_num_pairs", "l3d_get_pairs", "l3d_match_pairs", "l3d_slot_buffer", "l3d_match_finish",
    "l3d_compute_affinity", "l3d_synchronize", "l3d_pair_tests", "l3d_get_matches", "l3d_get_pair_slots",
    "l3d_num_best", "l3d_get_best", "l3d_view_info", "l3d_translation", "l3d_num_affinity", "l3d_get_affinity",
    "l3d_get_sparse_matrix", "l3d_get_timings", "l3d_match_lines", "l3d_set_brute_force", "l3d_slots_exchanged",
    "l3d_reconstruct_3d_lines", "l3d_num_3d_lines", "l3d_get_3d_lines", "l3d_diffuse_affinity",
    "l3d_output_filename", "l3d_save_3d_lines_txt", "l3d_save_result_stl", "l3d_save_result_obj",
    "l3d_get_segment_coords2d", "l3d_find_collinear_segments", "l3d_score_matches",
    "l3d_slot_index_buffer", "l3d_pack_slot_indices", "l3d_expand_slot_indices", "l3d_match_abort", "l3d_save_3d_lines_bin", "l3d_lists_shard",
    "l3d_principal_direction", "l3d_selftest_arith", "l3d_lists_shard_views", "l3d_plan_shards",
    "l3d_add_view_worldpoints", "l3d_get_visual_neighbors", "l3d_neighbors_from_worldpoints",
    "l3d_nvm_open", "l3d_nvm_num_cameras", "l3d_nvm_get_camera", "l3d_nvm_get_worldpoints", "l3d_nvm_close",
    "l3d_nvm_intrinsics", "l3d_segment_cache_name", "l3d_read_segment_cache", "l3d_write_segment_cache",
    "l3d_trim_cache", "l3d_set_timing_level", "l3d_tail_shard_count", "l3d_tail_shard_layout", "l3d_tail_shard_commit",
    "l3d_sfm_open_colmap", "l3d_sfm_open_bundler", "l3d_sfm_num_images", "l3d_sfm_get_image", "l3d_sfm_get_worldpoints",
    "l3d_sfm_close", "l3d_debug_counter", "l3d_affinity_shard_begin", "l3d_affinity_shard_finish", "l3d_affinity_shard_abort", "l3d_shard_options",
    "l3d_line_opt_stats", "l3d_line_to_cayley", "l3d_cayley_to_segment", "l3d_line_opt_eval", "l3d_line_opt_solve", "l3d_get_fresh_hyp",
    "l3d_detect_segments", "l3d_detect_view_segments", "l3d_get_detected_segments", "l3d_get_detect_stats",
    "l3d_add_view_image", "l3d_add_view_image_worldpoints", "l3d_undistort_images",
    "l3d_undistort_images_model", "l3d_sfm_get_camera_model", "l3d_sfm_get_camera_params",
    "l3d_triangulate_points", "l3d_rotation_from_rpy", "l3d_rotation_from_q", "l3d_decompose_projection_matrix",
    "l3d_project_segments", "l3d_render_line_maps", "l3d_draw_line_maps", "l3d_view_camera", "l3d_project_lines",
    "l3d_get_projected_lines", "l3d_render_lines", "l3d_draw_lines", "l3d_set_projection_budget", "l3d_selftest_scan",
    "l3d_debug_lsd_stages", "l3d_match_plan", "l3d_match_tile_rows", "l3d_debug_tail_records",
    "l3d_debug_affinity_records", "l3d_debug_keep_rows", "l3d_cull_forms", "l3d_debug_cull",
    "l3d_associate_segments", "l3d_associate_view_segments",
    "l3d_compare_segments", "l3d_compare_lines",
    "l3d_merge_segments", "l3d_merge_lines",
    "l3d_align_segments", "l3d_align_lines", "l3d_transform_segments",
    "l3d_refine_cameras", "l3d_refine_view_cameras",
    "l3d_wireframe_segments", "l3d_wireframe_lines", "l3d_wireframe_counts", "l3d_wireframe_get", "l3d_wireframe_save_obj",
    "l3d_wireframe_close",
    "l3d_plane_segments", "l3d_plane_lines", "l3d_planes_counts", "l3d_planes_get", "l3d_planes_save_obj", "l3d_planes_close",
    "l3d_direction_segments", "l3d_direction_lines", "l3d_directions_counts", "l3d_directions_get", "l3d_directions_save_obj",
    "l3d_directions_close",
    "l3d_refit_segments", "l3d_refit_view_lines", "l3d_refit_counts", "l3d_refit_get", "l3d_refit_close", "l3d_refit_span",
    "l3d_refit_sweep",
    "l3d_bundle_segments", "l3d_bundle_view_lines", "l3d_bundle_counts", "l3d_bundle_get", "l3d_bundle_close", "l3d_bundle_solve",
]

_lib = None


def load():
    """Load the HIP library; fail loudly if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: the HIP extension has not been built (run `make -C line3dpp_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    L = C.CDLL(SO_PATH)
    vp, u32, u64, i32, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
    L.l3d_last_error.restype = C.c_char_p
    L.l3d_build_info.restype = C.c_char_p
    L.l3d_trim_cache.argtypes = []; L.l3d_trim_cache.restype = u64
    L.l3d_create.argtypes = [i32, vp]; L.l3d_create.restype = vp
    L.l3d_destroy.argtypes = [vp]; L.l3d_destroy.restype = None
    L.l3d_add_view.argtypes = [vp, u32, vp, u32, vp, vp, vp, u32, u32, f32, vp, u32]
    L.l3d_add_view_worldpoints.argtypes = [vp, u32, vp, u32, vp, vp, vp, u32, u32, f32, vp, u32]
    L.l3d_get_visual_neighbors.argtypes = [vp, u32, vp, u32, vp]
    L.l3d_neighbors_from_worldpoints.argtypes = [u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, u64]
    L.l3d_sfm_open_colmap.argtypes = [C.c_char_p, vp]; L.l3d_sfm_open_bundler.argtypes = [C.c_char_p, vp]
    L.l3d_sfm_num_images.argtypes = [vp]; L.l3d_sfm_num_images.restype = u32
    L.l3d_sfm_get_image.argtypes = [vp, u32, vp]; L.l3d_sfm_get_worldpoints.argtypes = [vp, u32, vp, u32]
    L.l3d_sfm_close.argtypes = [vp]; L.l3d_sfm_close.restype = None
    L.l3d_nvm_open.argtypes = [C.c_char_p, vp]
    L.l3d_nvm_num_cameras.argtypes = [vp]; L.l3d_nvm_num_cameras.restype = u32
    L.l3d_nvm_get_camera.argtypes = [vp, u32, vp]
    L.l3d_nvm_get_worldpoints.argtypes = [vp, u32, vp, u32]
    L.l3d_nvm_close.argtypes = [vp]; L.l3d_nvm_close.restype = None
    L.l3d_nvm_intrinsics.argtypes = [f32, u32, u32, vp]; L.l3d_nvm_intrinsics.restype = None
    L.l3d_segment_cache_name.argtypes = [u32, u32, u32, u32, C.c_char_p, u32]
    L.l3d_read_segment_cache.argtypes = [C.c_char_p, vp, u32, vp]
    L.l3d_write_segment_cache.argtypes = [C.c_char_p, vp, u32]
    L.l3d_match_images.argtypes = [vp, C.POINTER(MatchParams)]
    L.l3d_match_begin.argtypes = [vp, C.POINTER(MatchParams)]
    L.l3d_num_pairs.argtypes = [vp, C.POINTER(u32)]
    L.l3d_get_pairs.argtypes = [vp, vp, vp, vp]
    L.l3d_match_pairs.argtypes = [vp, u32, u32]
    L.l3d_slot_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.l3d_get_fresh_hyp.argtypes = [vp, vp, u64]
    L.l3d_match_finish.argtypes = [vp]
    L.l3d_match_abort.argtypes = [vp]
    L.l3d_lists_shard.argtypes = [vp, u32, u32, vp, vp, vp]
    L.l3d_lists_shard_views.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp]
    L.l3d_plan_shards.argtypes = [u32, u32, vp, vp, u32, vp, vp]
    L.l3d_compute_affinity.argtypes = [vp]
    L.l3d_synchronize.argtypes = [vp]
    L.l3d_pair_tests.argtypes = [vp, C.POINTER(u64)]
    L.l3d_get_matches.argtypes = [vp, u32, vp, u64, vp, C.POINTER(u64)]
    L.l3d_get_pair_slots.argtypes = [vp, u32, vp, u64, C.POINTER(u32), C.POINTER(u32)]
    L.l3d_num_best.argtypes = [vp, C.POINTER(u32)]
    L.l3d_get_best.argtypes = [vp, vp, vp, vp]
    L.l3d_view_info.argtypes = [vp, u32, C.POINTER(f32), C.POINTER(f32)]
    L.l3d_translation.argtypes = [vp, vp]
    L.l3d_num_affinity.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.l3d_get_affinity.argtypes = [vp, vp, vp, C.POINTER(f32)]
    L.l3d_get_sparse_matrix.argtypes = [vp, i32, vp, vp]
    L.l3d_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.l3d_set_timing_level.argtypes = [vp, C.c_int]
    L.l3d_debug_counter.argtypes = [C.c_char_p]
    L.l3d_debug_counter.restype = C.c_ulonglong
    L.l3d_match_plan.argtypes = [u64, u32, u32, u32, u32, C.POINTER(MatchPlanInfo)]
    L.l3d_match_tile_rows.argtypes = [u64]; L.l3d_match_tile_rows.restype = u32
    L.l3d_tail_shard_count.argtypes = [vp, vp]
    L.l3d_tail_shard_layout.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
    L.l3d_tail_shard_commit.argtypes = [vp]
    L.l3d_affinity_shard_begin.argtypes = [vp, u32, u32, vp, vp, vp]
    L.l3d_affinity_shard_finish.argtypes = [vp]
    L.l3d_affinity_shard_abort.argtypes = [vp]
    L.l3d_shard_options.argtypes = [vp, C.c_uint32, C.c_int]
    L.l3d_match_lines.argtypes = [i32, vp, u32, vp, u32, vp, vp, vp, vp, vp, u32, u32, f32, C.c_int32, vp,
                                  C.POINTER(u64)]
    L.l3d_set_brute_force.argtypes = [vp, i32]
    L.l3d_slots_exchanged.argtypes = [vp]
    L.l3d_slot_index_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.l3d_pack_slot_indices.argtypes = [vp, u32, u32]
    L.l3d_expand_slot_indices.argtypes = [vp, u32, u32]
    L.l3d_reconstruct_3d_lines.argtypes = [vp, u32, i32, f32, i32, u32]
    L.l3d_num_3d_lines.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.l3d_get_3d_lines.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.l3d_diffuse_affinity.argtypes = [i32, vp, u32, u32, u32, vp]
    L.l3d_output_filename.argtypes = [vp, i32, C.c_char_p, u32]
    L.l3d_save_3d_lines_txt.argtypes = [vp, C.c_char_p, i32]
    L.l3d_save_result_stl.argtypes = [vp, C.c_char_p, i32]
    L.l3d_save_3d_lines_bin.argtypes = [vp, C.c_char_p, i32]
    L.l3d_save_result_obj.argtypes = [vp, C.c_char_p, i32]
    L.l3d_get_segment_coords2d.argtypes = [vp, u32, u32, vp]
    L.l3d_find_collinear_segments.argtypes = [i32, vp, u32, f32, vp, vp, u64, vp]
    L.l3d_principal_direction.argtypes = [vp, vp]
    L.l3d_line_opt_stats.argtypes = [vp, C.POINTER(LineOptStats)]
    L.l3d_line_to_cayley.argtypes = [vp, vp, vp]
    L.l3d_cayley_to_segment.argtypes = [vp, vp, vp, vp, vp]
    L.l3d_line_opt_eval.argtypes = [i32, u32, vp, vp, vp, vp, vp, vp, vp]
    L.l3d_line_opt_solve.argtypes = [i32, u32, vp, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp]
    L.l3d_selftest_arith.argtypes = [i32, u64, u64, vp]
    L.l3d_selftest_scan.argtypes = [i32, u32, vp, u32, u32, vp, i32, i32, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.l3d_detect_segments.argtypes = [vp, u32, vp, i32, u32, vp]
    L.l3d_detect_view_segments.argtypes = [vp, u32, vp, vp, C.POINTER(DetectOptions), vp]
    L.l3d_get_detected_segments.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.l3d_get_detect_stats.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.l3d_debug_lsd_stages.argtypes = [vp, u32, vp, i32, i32, vp]
    L.l3d_debug_tail_records.argtypes = [vp, i32, C.POINTER(TailRecords)]
    L.l3d_debug_affinity_records.argtypes = [vp, i32, C.POINTER(AffinityRecords)]
    L.l3d_debug_keep_rows.argtypes = [vp, i32, C.POINTER(KeepRows)]
    L.l3d_cull_forms.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(CullFormsInfo)]
    L.l3d_debug_cull.argtypes = [vp, u32, i32, C.POINTER(CullState)]
    L.l3d_add_view_image.argtypes = [vp, u32, C.POINTER(Image), C.POINTER(DetectOptions), vp, vp, vp, f32, vp, u32,
                                     C.POINTER(u32)]
    L.l3d_add_view_image_worldpoints.argtypes = [vp, u32, C.POINTER(Image), C.POINTER(DetectOptions), vp, vp, vp, f32,
                                                 vp, u32, C.POINTER(u32)]
    L.l3d_undistort_images.argtypes = [vp, u32, vp, vp, vp]
    L.l3d_undistort_images_model.argtypes = [vp, u32, vp, vp, vp]
    L.l3d_sfm_get_camera_model.argtypes = [vp, u32, vp]
    L.l3d_sfm_get_camera_params.argtypes = [vp, u32, vp, u32, vp]; L.l3d_sfm_get_camera_params.restype = C.c_char_p
    L.l3d_score_matches.argtypes = [i32, vp, u32, vp, vp, vp, u32, vp, vp, f32, f32, vp]
    L.l3d_triangulate_points.argtypes = [i32, u32, vp, u64, vp, vp, vp, vp, vp]
    f64 = C.c_double
    L.l3d_rotation_from_rpy.argtypes = [f64, f64, f64, vp]
    L.l3d_rotation_from_q.argtypes = [f64, f64, f64, f64, vp]
    L.l3d_decompose_projection_matrix.argtypes = [vp, vp, vp, vp]
    L.l3d_project_segments.argtypes = [i32, u32, vp, u32, vp, vp, f64, vp, vp, u64, C.POINTER(u64)]
    L.l3d_render_line_maps.argtypes = [i32, u32, vp, vp, vp, u32, vp, vp]
    L.l3d_draw_line_maps.argtypes = [i32, u32, vp, vp, u32, vp, u32, vp]
    L.l3d_view_camera.argtypes = [vp, u32, C.POINTER(Camera)]
    L.l3d_project_lines.argtypes = [vp, u32, vp, f64, vp]
    L.l3d_get_projected_lines.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.l3d_render_lines.argtypes = [vp, u32, vp, f64, u32, vp, vp]
    L.l3d_draw_lines.argtypes = [vp, u32, vp, vp, f64, u32, u32, vp, vp]
    L.l3d_set_projection_budget.argtypes = [vp, u64]
    L.l3d_associate_segments.argtypes = [i32, u32, vp, vp, vp, vp, C.POINTER(AssociateParams), vp]
    L.l3d_associate_view_segments.argtypes = [vp, u32, vp, C.POINTER(AssociateParams), f64, vp, vp, vp, vp]
    L.l3d_compare_segments.argtypes = [i32, u32, vp, vp, u32, vp, vp, C.POINTER(CompareParams), vp, vp,
                                       C.POINTER(CompareSummary), C.POINTER(CompareSummary)]
    L.l3d_compare_lines.argtypes = [vp, u32, vp, vp, C.POINTER(CompareParams), vp, vp, C.POINTER(CompareSummary),
                                    C.POINTER(CompareSummary)]
    L.l3d_merge_segments.argtypes = [i32, u32, vp, vp, C.POINTER(MergeParams), vp, u32, vp, vp, C.POINTER(u32), u32, vp,
                                     C.POINTER(u32), C.POINTER(MergeSummary)]
    L.l3d_merge_lines.argtypes = [vp, C.POINTER(MergeParams), C.POINTER(MergeSummary)]
    L.l3d_align_segments.argtypes = [i32, u32, vp, vp, u32, vp, vp, C.POINTER(AlignParams), C.POINTER(Similarity),
                                     C.POINTER(Similarity), C.POINTER(AlignSummary), vp, vp, vp, vp]
    L.l3d_align_lines.argtypes = [vp, u32, vp, vp, C.POINTER(AlignParams), C.POINTER(Similarity), C.POINTER(Similarity),
                                  C.POINTER(AlignSummary), vp, vp, vp, vp]
    L.l3d_transform_segments.argtypes = [u32, vp, C.POINTER(Similarity), vp]
    L.l3d_refine_cameras.argtypes = [i32, u32, vp, vp, u32, vp, vp, vp, C.POINTER(PoseParams), vp, vp, vp, vp]
    L.l3d_refine_view_cameras.argtypes = [vp, u32, vp, C.POINTER(PoseParams), vp, vp, vp, vp, vp]
    L.l3d_wireframe_segments.argtypes = [i32, u32, vp, vp, C.POINTER(WireframeParams), C.POINTER(vp)]
    L.l3d_wireframe_lines.argtypes = [vp, C.POINTER(WireframeParams), C.POINTER(vp)]
    L.l3d_wireframe_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.l3d_wireframe_get.argtypes = [vp, vp, vp, vp, C.POINTER(WireframeSummary)]
    L.l3d_wireframe_save_obj.argtypes = [vp, C.c_char_p]
    L.l3d_wireframe_close.argtypes = [vp]; L.l3d_wireframe_close.restype = None
    L.l3d_plane_segments.argtypes = [i32, u32, vp, vp, C.POINTER(PlanesParams), C.POINTER(vp)]
    L.l3d_plane_lines.argtypes = [vp, C.POINTER(PlanesParams), C.POINTER(vp)]
    L.l3d_planes_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.l3d_planes_get.argtypes = [vp, vp, vp, vp, vp, C.POINTER(PlanesSummary)]
    L.l3d_planes_save_obj.argtypes = [vp, C.c_char_p]
    L.l3d_planes_close.argtypes = [vp]; L.l3d_planes_close.restype = None
    L.l3d_direction_segments.argtypes = [i32, u32, vp, vp, C.POINTER(DirectionsParams), C.POINTER(vp)]
    L.l3d_direction_lines.argtypes = [vp, C.POINTER(DirectionsParams), C.POINTER(vp)]
    L.l3d_directions_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.l3d_directions_get.argtypes = [vp, vp, vp, vp, vp, C.POINTER(DirectionsSummary)]
    L.l3d_directions_save_obj.argtypes = [vp, C.c_char_p]
    L.l3d_directions_close.argtypes = [vp]; L.l3d_directions_close.restype = None
    L.l3d_refit_segments.argtypes = [i32, u32, vp, vp, u32, vp, vp, vp, C.POINTER(RefitParams), C.POINTER(vp)]
    L.l3d_refit_view_lines.argtypes = [vp, u32, vp, vp, C.POINTER(RefitParams), C.POINTER(RefitSummary), C.POINTER(vp)]
    L.l3d_refit_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.l3d_refit_get.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(RefitSummary)]
    L.l3d_refit_close.argtypes = [vp]; L.l3d_refit_close.restype = None
    L.l3d_refit_span.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.l3d_refit_sweep.argtypes = [u32, vp, vp, vp, u32, C.c_double, C.c_double, vp, C.POINTER(u32)]
    L.l3d_bundle_segments.argtypes = [i32, u32, vp, vp, u32, vp, vp, vp, vp, C.POINTER(BundleParams), C.POINTER(vp)]
    L.l3d_bundle_view_lines.argtypes = [vp, u32, vp, vp, vp, C.POINTER(BundleParams), C.POINTER(BundleSummary), C.POINTER(vp)]
    L.l3d_bundle_counts.argtypes = [vp] + [C.POINTER(u64)] * 7
    L.l3d_bundle_get.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(BundleSummary)]
    L.l3d_bundle_close.argtypes = [vp]; L.l3d_bundle_close.restype = None
    L.l3d_bundle_solve.argtypes = [u32, vp, vp, vp]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("l3d_last_error", "l3d_build_info", "l3d_create", "l3d_destroy"):
            fn.restype = C.c_int
    _lib = L
    return L


def last_error():
    return load().l3d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
