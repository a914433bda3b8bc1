"""ctypes loader for liborbx.so (the HIP kernels + C ABI of include/orbx.h).

There is no CPU fallback: if the shared library is missing or cannot be
loaded, or no gfx950 device is visible when a handle is created, the call
raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C orb_slam2_commit_amd/csrc``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBX_LIB_OVERRIDE") or os.path.join(_HERE, "liborbx.so")  # override: A/B experiments only

ORBX_OK = 0
ORBX_ERR_ARG = -1
ORBX_ERR_CAPACITY = -2
ORBX_ERR_HIP = -3
ORBX_ERR_NODEV = -4
ORBX_ERR_SIZE = -5
ORBX_ERR_STATE = -6
ORBX_DEPTH_U16 = 2  # CV_16U
ORBX_DEPTH_F32 = 5  # CV_32F
_ERRS = {ORBX_ERR_ARG: "bad argument", ORBX_ERR_CAPACITY: "capacity", ORBX_ERR_HIP: "HIP runtime error",
         ORBX_ERR_NODEV: "no HIP device", ORBX_ERR_SIZE: "unsupported geometry", ORBX_ERR_STATE: "no extraction yet"}

# Layout-identical to cv::KeyPoint / orbx_keypoint (28 bytes).
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28


class OrbxError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s failed: %s (%d)" % (what, _ERRS.get(code, "error"), code))
        self.code = code


class ExtractorParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


class BowSide(C.Structure):
    _fields_ = [("n", C.c_int), ("desc", C.c_void_p), ("angle", C.c_void_p), ("valid", C.c_void_p),
                ("n_nodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p), ("feat", C.c_void_p)]


class BowProblem(C.Structure):
    _fields_ = [("a", BowSide), ("b", BowSide), ("nnratio", C.c_float), ("check_ori", C.c_int), ("mode", C.c_int),
                ("match", C.c_void_p), ("nmatches", C.c_void_p), ("a_n_dev", C.c_void_p), ("a_nodes_dev", C.c_void_p),
                ("b_n_dev", C.c_void_p), ("b_nodes_dev", C.c_void_p)]


class BaProblem(C.Structure):
    _fields_ = [("n_cams", C.c_int), ("Tcw", C.c_void_p), ("fixed", C.c_void_p), ("intr", C.c_void_p),
                ("n_points", C.c_int), ("Xw", C.c_void_p), ("n_edges", C.c_int), ("edge_point", C.c_void_p),
                ("edge_cam", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p)]


class BaResult(C.Structure):
    _fields_ = [("Tcw", C.c_void_p), ("Xw", C.c_void_p), ("edge_outlier", C.c_void_p), ("Tcw_d", C.c_void_p),
                ("Xw_d", C.c_void_p), ("iterations", C.c_int * 2), ("trials", C.c_int), ("chi2", C.c_double * 2),
                ("ran", C.c_int)]


class PnpProblem(C.Structure):
    _fields_ = [("n", C.c_int), ("p3d", C.c_void_p), ("p2d", C.c_void_p), ("sigma2", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class PnpParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int), ("max_iterations", C.c_int),
                ("min_set", C.c_int), ("epsilon", C.c_float), ("th2", C.c_float)]


class ProjFrame(C.Structure):
    _fields_ = [("n", C.c_int), ("keys_un", C.c_void_p), ("desc", C.c_void_p), ("u_right", C.c_void_p),
                ("occ", C.c_void_p), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float), ("nlevels", C.c_int),
                ("scale_factors", C.c_float * 16), ("inv_level_sigma2", C.c_float * 16),
                ("log_scale_factor", C.c_float), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("b", C.c_float),
                ("Tcw", C.c_float * 16), ("grid_min_x", C.c_float), ("grid_min_y", C.c_float),
                ("grid_min_set", C.c_int)]


class ProjProblem(C.Structure):
    _fields_ = [("kind", C.c_int), ("frustum", C.c_int), ("f", ProjFrame), ("n_points", C.c_int),
                ("desc", C.c_void_p), ("flags", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p),
                ("dist_minmax", C.c_void_p), ("angle", C.c_void_p), ("octave", C.c_void_p), ("track", C.c_void_p),
                ("track_level", C.c_void_p), ("th", C.c_float), ("nnratio", C.c_float),
                ("view_cos_limit", C.c_float), ("check_ori", C.c_int), ("mono", C.c_int), ("orb_dist", C.c_int),
                ("last_Tcw", C.c_float * 16), ("frame_out", C.c_void_p), ("point_match", C.c_void_p),
                ("nmatches", C.c_void_p), ("f_n_dev", C.c_void_p), ("n_points_dev", C.c_void_p),
                ("Tcw_dev", C.c_void_p), ("gate", C.c_void_p), ("gate_below", C.c_int)]


class Sim3Problem(C.Structure):
    _fields_ = [("kf1", ProjFrame), ("kf2", ProjFrame)] + \
               [(k, C.c_void_p) for k in ("desc1", "pos1", "dist_minmax1", "flags1", "desc2", "pos2", "dist_minmax2",
                                          "flags2")] + \
               [("s12", C.c_float), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("th", C.c_float),
                ("match12", C.c_void_p), ("nfound", C.c_void_p)]


class InitProblem(C.Structure):
    _fields_ = [("f1", ProjFrame), ("f2", ProjFrame), ("prev_matched", C.c_void_p), ("window", C.c_int),
                ("nnratio", C.c_float), ("check_ori", C.c_int), ("match12", C.c_void_p), ("nmatches", C.c_void_p)]


class PoseProblem(C.Structure):
    _fields_ = [("n", C.c_int), ("obs", C.c_void_p), ("Xw", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("Tcw", C.c_float * 16), ("Tcw_out", C.c_void_p), ("outlier", C.c_void_p), ("ngood", C.c_void_p),
                ("iterations", C.c_void_p), ("n_dev", C.c_void_p), ("Tcw_dev", C.c_void_p)]


class OptSim3Problem(C.Structure):  # orbx_optimize_sim3_problem (Optimizer::OptimizeSim3)
    _fields_ = [("n", C.c_int)] + \
               [(k, C.c_void_p) for k in ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")] + \
               [("K1", C.c_float * 4), ("K2", C.c_float * 4), ("S12", C.c_double * 8), ("th2", C.c_float),
                ("fix_scale", C.c_int)] + \
               [(k, C.c_void_p) for k in ("S12_out", "inlier", "n_in", "n_bad", "iterations", "trials", "n_dev")]


class EssGraphProblem(C.Structure):  # orbx_essential_graph_problem (Optimizer::OptimizeEssentialGraph)
    _fields_ = [("n_vertices", C.c_int), ("vertex_id", C.c_void_p), ("Scw", C.c_void_p), ("Snc", C.c_void_p),
                ("fixed_vertex", C.c_int), ("fix_scale", C.c_int), ("n_edges", C.c_int), ("edge_v0", C.c_void_p),
                ("edge_v1", C.c_void_p), ("edge_kind", C.c_void_p), ("iterations", C.c_int),
                ("lambda_init", C.c_double), ("n_points", C.c_int), ("Xw", C.c_void_p), ("point_ref", C.c_void_p)]


class EssGraphResult(C.Structure):  # orbx_essential_graph_result
    _fields_ = [(k, C.c_void_p) for k in ("Scw_out", "Tcw_out", "Xw_out", "iterations", "trials", "chi2_initial",
                                          "chi2_final", "solver_failures")]


class TriKF(C.Structure):
    _fields_ = [("n", C.c_int), ("keys_un", C.c_void_p), ("desc", C.c_void_p), ("u_right", C.c_void_p),
                ("has_mp", C.c_void_p), ("n_nodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p),
                ("feat", C.c_void_p)]


class TriProblem(C.Structure):
    _fields_ = [("kf1", TriKF), ("kf2", TriKF), ("F12", C.c_float * 9), ("C1w", C.c_float * 3),
                ("T2w", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("scale_factors2", C.c_float * 16), ("level_sigma2_2", C.c_float * 16), ("only_stereo", C.c_int),
                ("check_ori", C.c_int), ("match12", C.c_void_p), ("nmatches", C.c_void_p)]


class NewPointsKF(C.Structure):  # orbx_new_points_kf (LocalMapping::CreateNewMapPoints)
    _fields_ = [("kf", TriKF), ("keys_xy", C.c_void_p), ("depth", C.c_void_p), ("mp_pos", C.c_void_p),
                ("Tcw", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float), ("n_levels", C.c_int), ("scale_factors", C.c_float * 16),
                ("level_sigma2", C.c_float * 16)]


class NewPointsProblem(C.Structure):  # orbx_new_points_problem
    _fields_ = [("current", NewPointsKF), ("n_neighbours", C.c_int), ("neighbours", C.POINTER(NewPointsKF)),
                ("monocular", C.c_int), ("scale_factor", C.c_float)]


class NewPointsResult(C.Structure):  # orbx_new_points_result
    _fields_ = [(k, C.c_void_p) for k in ("n_new", "neighbours_done", "point_idx", "point_pos", "point_normal",
                                          "point_dist", "nb_skip", "nb_nmatches", "nb_baseline", "nb_median_depth",
                                          "has_mp1")]


class NewPointsDebugOptions(C.Structure):  # include/orbx_debug.h orbx_new_points_debug_options
    _fields_ = [("raise_after_neighbour", C.c_int), ("probes", C.c_int)]


class FramePoints(C.Structure):
    _fields_ = [("kps", C.c_void_p), ("depth", C.c_void_p), ("count", C.c_void_p), ("cap", C.c_int),
                ("Twc", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("nlevels", C.c_int), ("scale_factors", C.c_float * 16), ("pos", C.c_void_p), ("normal", C.c_void_p),
                ("dist_minmax", C.c_void_p), ("angle", C.c_void_p), ("octave", C.c_void_p), ("flags", C.c_void_p)]


class TrackStep(C.Structure):
    _fields_ = [("op", C.c_int), ("cap", C.c_int), ("count", C.c_void_p), ("kps", C.c_void_p), ("u_right", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("n_points", C.c_void_p), ("pos", C.c_void_p),
                ("flags", C.c_void_p), ("frame_out", C.c_void_p), ("nmatches", C.c_void_p), ("min_matches", C.c_int),
                ("outlier", C.c_void_p), ("ngood", C.c_void_p), ("min_good", C.c_int), ("fmap", C.c_void_p),
                ("seen", C.c_void_p), ("local_flags", C.c_void_p), ("occ", C.c_void_p), ("lost", C.c_void_p),
                ("obs", C.c_void_p), ("Xw", C.c_void_p), ("inv_sigma2", C.c_void_p), ("edge_feature", C.c_void_p),
                ("n_edges", C.c_void_p)]


class TrackGather(C.Structure):
    _fields_ = [("f_kps", C.c_void_p), ("f_uright", C.c_void_p), ("f_count", C.c_void_p), ("match", C.c_void_p),
                ("kf_kps", C.c_void_p), ("kf_depth", C.c_void_p), ("Twc", C.c_float * 12), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("inv_level_sigma2", C.c_void_p),
                ("obs", C.c_void_p), ("Xw", C.c_void_p), ("inv_sigma2", C.c_void_p), ("edge_feature", C.c_void_p),
                ("n_edges", C.c_void_p)]


class BaDebugOptions(C.Structure):  # include/orbx_debug.h orbx_ba_debug_options
    _fields_ = [("ldlt", C.c_int), ("nan_trial", C.c_int), ("raise_stop_after", C.c_int), ("trace", C.c_int),
                ("fused_ctl", C.c_int)]


class Camera(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("dist", C.c_float * 5), ("n_dist", C.c_int)]


class RandState(C.Structure):
    _fields_ = [("r", C.c_uint32 * 34), ("i", C.c_int32)]


class PnpResult(C.Structure):
    _fields_ = [("no_more", C.c_int), ("found", C.c_int), ("n_inliers", C.c_int), ("used", C.c_int),
                ("Tcw", C.c_float * 16)]


class Sim3SolverProblem(C.Structure):  # orbx_sim3_solver_problem (Sim3Solver; Sim3Problem is SearchBySim3's)
    _fields_ = [("n", C.c_int), ("x3dc1", C.c_void_p), ("x3dc2", C.c_void_p), ("sigma2_1", C.c_void_p),
                ("sigma2_2", C.c_void_p)] + \
               [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] + \
               [("fix_scale", C.c_int)]


class Sim3Params(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int), ("max_iterations", C.c_int)]


class Sim3Result(C.Structure):
    _fields_ = [("no_more", C.c_int), ("found", C.c_int), ("n_inliers", C.c_int), ("used", C.c_int),
                ("T12", C.c_float * 16)]


class InitializerResult(C.Structure):  # orbx_initializer_result (Initializer::Initialize)
    _fields_ = [("ok", C.c_int), ("degenerate", C.c_int), ("SH", C.c_float), ("SF", C.c_float),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("it_h", C.c_int), ("it_f", C.c_int),
                ("model", C.c_int), ("n_hyp", C.c_int), ("n_good", C.c_int * 8), ("parallax", C.c_float * 8),
                ("best", C.c_int), ("n_matches", C.c_int), ("n_inliers", C.c_int), ("inliers_h", C.c_void_p),
                ("inliers_f", C.c_void_p)]


# Every entry point of include/orbx.h with its ctypes signature.
P = C.c_void_p
SIGNATURES = {
    "orbx_extractor_create": ([C.POINTER(ExtractorParams), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_extractor_destroy": ([P], None),
    "orbx_extractor_get_levels": ([P], C.c_int),
    "orbx_extractor_scale_tables": ([P, P, P, P, P], C.c_int),
    "orbx_extractor_tables": ([P, P, P, P], C.c_int),
    "orbx_extractor_set_pyramid_readback": ([P, C.c_int], C.c_int),
    "orbx_extractor_max_keypoints": ([P, C.c_int, C.c_int], C.c_int),
    "orbx_extract": ([P, P, C.c_int, C.c_int, C.c_size_t, P, C.c_int, P, C.POINTER(C.c_int)], C.c_int),
    "orbx_pyramid_level": ([P, C.c_int, C.c_int, P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "orbx_extract_batch_device": ([P, C.c_int, P, C.c_int, C.c_int, C.c_size_t, P, P, P, C.c_int, P], C.c_int),
    "orbx_stereo_match": ([P, P, P, P, C.c_int, P, P, C.c_int, C.c_float, C.c_float, P, P], C.c_int),
    "orbx_frame_stereo": ([P, P, C.c_size_t, P, C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_float, P, P, C.c_int, P,
                           P, P, C.c_int, P, P, P], C.c_int),
    "orbx_stereo_frames_device": ([P, C.c_int, P, C.c_int, C.c_int, C.c_size_t, P, P, P, C.c_int, C.c_float,
                                   C.c_float, P, P, P, P], C.c_int),
    "orbx_cvt_gray": ([P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_size_t,
                       C.c_size_t, C.c_int], C.c_int),
    "orbx_cvt_gray_device": ([P, P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P,
                              C.c_size_t, C.c_size_t, P], C.c_int),
    "orbx_frame_rgbd": ([P, P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_size_t, C.c_int, C.c_int,
                         C.c_int, C.c_float, C.POINTER(Camera), C.c_float, P, P, C.c_int, C.POINTER(C.c_int), P, P,
                         P], C.c_int),
    "orbx_rgbd_frames_device": ([P, C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, P,
                                 C.c_int, C.c_size_t, C.c_size_t, C.c_float, C.POINTER(Camera), C.c_float, P, P, P,
                                 C.c_int, P, P, P, P, P], C.c_int),
    "orbx_descriptor_distance_device": ([P, P, C.c_int, P, P], C.c_int),
    "orbx_search_by_bow_kf_f": ([C.POINTER(BowSide), C.POINTER(BowSide), C.c_float, C.c_int, P,
                                 C.POINTER(C.c_int), C.c_int], C.c_int),
    "orbx_search_by_bow_kf_kf": ([C.POINTER(BowSide), C.POINTER(BowSide), C.c_float, C.c_int, P,
                                  C.POINTER(C.c_int), C.c_int], C.c_int),
    "orbx_search_by_bow_device": ([C.POINTER(BowProblem), C.c_int, P], C.c_int),
    "orbx_pnp_create": ([C.POINTER(PnpProblem), C.POINTER(PnpParams), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_pnp_create_many": ([P, C.c_int, C.POINTER(PnpParams), C.c_int, P], C.c_int),
    "orbx_pnp_create_many_device": ([P, P, P, P, P, C.c_int, C.POINTER(PnpParams), C.c_int, P], C.c_int),
    "orbx_pnp_destroy": ([P], C.c_int),
    "orbx_pnp_get_params": ([P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)], C.c_int),
    "orbx_pnp_set_ransac_parameters": ([P, P, C.POINTER(PnpParams)], C.c_int),
    "orbx_pnp_iterate": ([P, C.c_int, P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), P, P,
                          C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "orbx_pnp_iterate_stream": ([P, C.c_int, C.POINTER(RandState), C.POINTER(C.c_int), P, P, C.POINTER(C.c_int),
                                 C.POINTER(C.c_int)], C.c_int),
    "orbx_voc_load_text": ([C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_voc_destroy": ([P], C.c_int),
    "orbx_voc_info": ([P, P], C.c_int),
    "orbx_voc_transform": ([P, P, P, C.c_int, C.c_int, P, P, P, P, P, P, P], C.c_int),
    "orbx_voc_transform_device": ([P, P, C.c_int, C.c_longlong, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P, P],
                                  C.c_int),
    "orbx_kfdb_create": ([P, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_kfdb_destroy": ([P], C.c_int),
    "orbx_kfdb_check_bow": ([P, P, C.c_int, C.c_uint32], C.c_int),
    "orbx_kfdb_add": ([P, C.c_int64, P, P, C.c_int], C.c_int),
    "orbx_kfdb_erase": ([P, C.c_int64], C.c_int),
    "orbx_kfdb_clear": ([P], C.c_int),
    "orbx_kfdb_set_neighbours": ([P, P, P, P, C.c_int], C.c_int),
    "orbx_kfdb_reloc_candidates": ([P, C.c_uint64, P, P, C.c_int, P, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "orbx_kfdb_loop_candidates": ([P, C.c_uint64, P, P, C.c_int, P, C.c_int, C.c_float, P, C.c_int,
                                   C.POINTER(C.c_int)], C.c_int),
    "orbx_kfdb_reloc_candidates_device": ([P, C.c_uint64, P, P, P, P, C.c_int, P, P], C.c_int),
    "orbx_kfdb_loop_candidates_device": ([P, C.c_uint64, P, P, P, P, C.c_int, C.c_float, P, C.c_int, P, P],
                                         C.c_int),
    "orbx_kfdb_score": ([P, P, P, C.c_int, P, C.c_int, P], C.c_int),
    "orbx_kfdb_read_state": ([P, P, C.c_int, P, P, P, P, P, P], C.c_int),
    "orbx_kfdb_size": ([P, C.POINTER(C.c_int), C.POINTER(C.c_longlong)], C.c_int),
    "orbx_covis_create": ([C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_covis_destroy": ([P], C.c_int),
    "orbx_covis_clear": ([P], C.c_int),
    "orbx_covis_check_row": ([P, P, P, C.c_int], C.c_int),
    "orbx_covis_set_keyframe": ([P, C.c_int64, C.c_int, P, P, P], C.c_int),
    "orbx_covis_erase_keyframe": ([P, C.c_int64], C.c_int),
    "orbx_covis_set_points_bad": ([P, P, C.c_int], C.c_int),
    "orbx_covis_size": ([P, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_int)], C.c_int),
    "orbx_covis_read_keyframe": ([P, C.c_int64, P, P, P, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "orbx_covis_read_points": ([P, P, C.c_int, P, P], C.c_int),
    "orbx_covis_update_connections": ([P, C.c_int64, C.c_int, P, P, C.c_int, C.POINTER(C.c_int), P, P, C.c_int,
                                       C.POINTER(C.c_int)], C.c_int),
    "orbx_covis_vote": ([P, P, C.c_int, P, P, P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                         C.POINTER(C.c_int32)], C.c_int),
    "orbx_covis_local_points": ([P, P, C.c_int, P, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "orbx_covis_cull": ([P, P, C.c_int, P, C.c_int, P, P, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "orbx_track_gather_device": ([C.POINTER(TrackGather), C.c_int, P], C.c_int),
    "orbx_frame_points_device": ([C.POINTER(FramePoints), C.c_int, P], C.c_int),
    "orbx_track_step_device": ([C.POINTER(TrackStep), C.c_int, P], C.c_int),
    "orbx_search_by_projection": ([C.POINTER(ProjProblem), C.c_int], C.c_int),
    "orbx_search_by_sim3": ([C.POINTER(Sim3Problem), C.c_int], C.c_int),
    "orbx_search_for_initialization": ([C.POINTER(InitProblem), C.c_int], C.c_int),
    "orbx_search_by_projection_device": ([C.POINTER(ProjProblem), C.c_int, P], C.c_int),
    "orbx_pose_optimization": ([C.POINTER(PoseProblem), C.c_int], C.c_int),
    "orbx_pose_optimization_device": ([C.POINTER(PoseProblem), C.c_int, P], C.c_int),
    "orbx_optimize_sim3": ([C.POINTER(OptSim3Problem), C.c_int], C.c_int),
    "orbx_optimize_sim3_device": ([C.POINTER(OptSim3Problem), C.c_int, P], C.c_int),
    "orbx_optimize_essential_graph": ([C.POINTER(EssGraphProblem), C.POINTER(EssGraphResult), C.c_int], C.c_int),
    "orbx_optimize_essential_graph_device": ([C.POINTER(EssGraphProblem), C.POINTER(EssGraphResult), P], C.c_int),
    "orbx_sim3_from_tcw": ([P, P], None),
    "orbx_search_for_triangulation": ([C.POINTER(TriProblem), C.c_int], C.c_int),
    "orbx_search_for_triangulation_device": ([C.POINTER(TriProblem), C.c_int, P], C.c_int),
    "orbx_new_points_create": ([C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_new_points_destroy": ([P], C.c_int),
    "orbx_new_points_stop_flag": ([P, C.POINTER(C.POINTER(C.c_int))], C.c_int),
    "orbx_create_new_map_points": ([P, C.POINTER(NewPointsProblem), C.POINTER(NewPointsResult)], C.c_int),
    "orbx_create_new_map_points_bool": ([P, C.POINTER(NewPointsProblem), C.POINTER(NewPointsResult), P], C.c_int),
    "orbx_create_new_map_points_device": ([P, C.POINTER(NewPointsProblem), C.POINTER(NewPointsResult), P], C.c_int),
    "orbx_distinctive_descriptors": ([P, P, C.c_int, P, P, C.c_int], C.c_int),
    "orbx_distinctive_descriptors_device": ([P, P, C.c_int, P, P, P], C.c_int),
    "orbx_undistort_keypoints": ([P, C.c_int, C.POINTER(Camera), P, C.c_int], C.c_int),
    "orbx_undistort_keypoints_device": ([P, P, C.c_int, C.c_int, P, P, P], C.c_int),
    "orbx_pnp_iterate_candidates": ([P, C.c_int, C.c_int, C.POINTER(RandState), P, P, C.POINTER(C.c_int)], C.c_int),
    "orbx_pnp_iterate_many": ([P, C.c_int, C.c_int, P, P, P], C.c_int),
    "orbx_sim3_create": ([C.POINTER(Sim3SolverProblem), C.POINTER(Sim3Params), C.c_int, C.POINTER(C.c_void_p)],
                         C.c_int),
    "orbx_sim3_create_many": ([P, C.c_int, C.POINTER(Sim3Params), C.c_int, P], C.c_int),
    "orbx_sim3_destroy": ([P], C.c_int),
    "orbx_sim3_set_ransac_parameters": ([P, C.POINTER(Sim3Params)], C.c_int),
    "orbx_sim3_get_params": ([P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
                             C.c_int),
    "orbx_sim3_iterate": ([P, C.c_int, P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), P, P,
                           C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "orbx_sim3_iterate_stream": ([P, C.c_int, C.POINTER(RandState), C.POINTER(C.c_int), P, P, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)], C.c_int),
    "orbx_sim3_get_estimate": ([P, P, P, C.POINTER(C.c_float)], C.c_int),
    "orbx_sim3_iterate_candidates": ([P, C.c_int, C.c_int, C.POINTER(RandState), P, P, C.POINTER(C.c_int)],
                                     C.c_int),
    "orbx_sim3_iterate_many": ([P, C.c_int, C.c_int, P, P, P], C.c_int),
    "orbx_initializer_create": ([P, C.c_int, P, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_initializer_destroy": ([P], C.c_int),
    "orbx_initializer_initialize": ([P, P, C.c_int, P, P, C.c_int, C.POINTER(C.c_int), P, P, P, P,
                                     C.POINTER(InitializerResult)], C.c_int),
    "orbx_initializer_initialize_stream": ([P, P, C.c_int, P, C.POINTER(RandState), P, P, P, P,
                                            C.POINTER(InitializerResult)], C.c_int),
    "orbx_rand_seed":([C.POINTER(RandState), C.c_uint32], None),
    "orbx_rand_next": ([C.POINTER(RandState)], C.c_int32),
    "orbx_ba_create": ([C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_ba_create_priority": ([C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_ba_create_masked": ([C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_stream_create": ([C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "orbx_stream_destroy": ([C.c_void_p], None),
    "orbx_ba_destroy": ([P], C.c_int),
    "orbx_ba_run": ([P, C.POINTER(BaProblem), C.POINTER(BaResult), P], C.c_int),
    "orbx_ba_run_bool": ([P, C.POINTER(BaProblem), C.POINTER(BaResult), P], C.c_int),
    "orbx_ba_run_global": ([P, C.POINTER(BaProblem), C.c_int, C.c_int, C.POINTER(BaResult), P, P], C.c_int),
    "orbx_ba_run_global_bool": ([P, C.POINTER(BaProblem), C.c_int, C.c_int, C.POINTER(BaResult), P, P], C.c_int),
    "orbx_ba_stop_flag":([P, C.POINTER(C.POINTER(C.c_int))], C.c_int),
    "orbx_ba_run_many": ([P, C.c_int, C.POINTER(BaProblem), C.POINTER(BaResult), P], C.c_int),
    "orbx_local_ba": ([C.POINTER(BaProblem), C.POINTER(BaResult), P, C.c_int], C.c_int),
    "orbx_device_count": ([], C.c_int),
    "orbx_version": ([], C.c_char_p),
    "orbx_sizeof": ([C.c_char_p], C.c_longlong),
    "orbx_profile_enable": ([P, C.c_int], C.c_int),
    "orbx_profile_reset": ([P], C.c_int),
    "orbx_profile_read": ([P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong),
                           C.POINTER(C.c_char_p)], C.c_int),
    # include/orbx_debug.h
    "orbx_debug_copy": ([P, C.c_int, C.c_int, C.c_int, P, C.c_size_t], C.c_longlong),
    "orbx_debug_launch_plan": ([C.POINTER(ExtractorParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P,
                                C.c_size_t], C.c_longlong),
    "orbx_debug_stereo_keypoints": ([P, P, P, P, C.c_int, P, P, C.c_int, C.c_float, C.c_float, P, P, P, P], C.c_int),
    "orbx_debug_stereo_keypoints_check": ([P, C.c_int, C.c_int, C.c_int, C.c_int], C.c_int),
    "orbx_debug_octree_candidates": ([P, C.c_int, P, P, P, P], C.c_int),
    "orbx_debug_octree_paths": ([P, C.c_int, P, P, C.c_int, P, P, P], C.c_int),    "orbx_debug_octree_candidates_check": ([C.POINTER(ExtractorParams), C.c_int, C.c_int, C.c_int, P, P], C.c_int),
    "orbx_debug_atan2_det": ([C.c_double, C.c_double], C.c_double),
    "orbx_debug_exp": ([P, C.c_int, P, C.c_int], C.c_int),
    "orbx_debug_initializer_host": ([P, C.c_int, P, C.c_float, C.c_int, P, C.c_int, P, P, C.c_int,
                                     C.POINTER(C.c_int), P, P, P, P, C.POINTER(InitializerResult)], C.c_int),
    "orbx_debug_acosf_det": ([C.c_float], C.c_float),
    "orbx_debug_lm_step": ([P, P, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int], C.c_int),
    "orbx_debug_sim3_exp": ([P, P, C.c_int, P, C.c_int], C.c_int),
    "orbx_debug_log": ([P, C.c_int, P, C.c_int], C.c_int),
    "orbx_debug_acos": ([P, C.c_int, P, C.c_int], C.c_int),
    "orbx_debug_sim3_log": ([P, C.c_int, P, P, C.c_int], C.c_int),
    "orbx_debug_essgraph_linearize": ([C.POINTER(EssGraphProblem), P, P, P, P, P, P, C.c_int], C.c_int),
    "orbx_debug_essgraph_solve": ([C.POINTER(EssGraphProblem), P, P, C.c_double, P, P, C.c_int], C.c_int),
    "orbx_debug_essgraph_phases": ([C.POINTER(EssGraphProblem), C.POINTER(EssGraphResult), P, P, C.c_int], C.c_int),
    "orbx_debug_ldlt": ([P, P, C.c_int, P, C.c_int, C.POINTER(C.c_float)], C.c_int),
    "orbx_debug_ldlt_ex": ([P, P, C.c_int, P, C.c_int, C.POINTER(C.c_float), C.c_int, P], C.c_int),
    "orbx_debug_ba_options": ([P, C.POINTER(BaDebugOptions)], C.c_int),
    "orbx_debug_ba_capture_select": ([P, C.c_int, C.c_int, C.c_int], C.c_int),
    "orbx_debug_ba_capture_read": ([P, C.c_int, P, C.c_size_t], C.c_longlong),
    "orbx_debug_new_points_options": ([P, C.POINTER(NewPointsDebugOptions)], C.c_int),
    "orbx_debug_new_points_probe": ([P, C.c_int, P, C.c_size_t], C.c_longlong),
    "orbx_debug_new_points_host": ([C.POINTER(NewPointsProblem), C.c_int, P, P, P, P, P, P, P, P, P, P], C.c_int),
    "orbx_debug_hbm_copy": ([P, P, C.c_size_t, C.c_int, C.POINTER(C.c_float)], C.c_int),
}

# include/orbx_debug.h ORBX_BA_CAP_*: item -> (id, dtype, trailing shape); HEADER (id 0) is read apart
BA_CAPTURE_ITEMS = {
    "lambda_chi": (1, np.float64, ()), "cq": (2, np.float64, (4,)), "ct": (3, np.float64, (3,)),
    "X": (4, np.float64, (3,)), "eerr": (5, np.float64, (3,)), "S": (6, np.float64, ()), "bs": (7, np.float64, ()),
    "xp": (8, np.float64, ()), "cbak": (9, np.float64, (7,)), "Xbak": (10, np.float64, (3,)),
    "xl": (11, np.float64, (3,)), "act": (12, np.int32, ()), "pose_cam": (13, np.int32, ()),
    "pt_id": (14, np.int32, ()), "erobust": (15, np.int32, ()),
}
BA_CAPTURE_HEADER = ("fired", "phase", "it", "q", "ok", "trial", "nc", "np", "ne", "na", "npa", "nposes")

_lib = None
# debug entries an ORBX_LIB_OVERRIDE library built from the parent commit may lack; the shipped
# library must have every entry of SIGNATURES
_NEWER_ENTRIES = {"orbx_debug_octree_paths"}


def lib():
    """Load liborbx.so (raises if it is absent: no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("liborbx.so not found at %s -- build it first (make -C orb_slam2_commit_amd/csrc)"
                               % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in SIGNATURES.items():
            if name in _NEWER_ENTRIES and os.environ.get("ORBX_LIB_OVERRIDE") and not hasattr(L, name):
                continue  # a side-by-side library of an earlier commit (A/B runs); calling the entry still raises
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


def check(code, what):
    if code != ORBX_OK:
        raise OrbxError(code, what)


def ptr(a):
    """Host numpy array or torch tensor (host or device) -> void*."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        # a writable buffer's address through ctypes.from_buffer (~1 us; ctypes.data_as ~4 us), else
        # (read-only, empty, non-contiguous) the array interface's data pointer
        try:
            return C.c_void_p(C.addressof(C.c_char.from_buffer(a)))
        except (TypeError, ValueError, BufferError):
            return C.c_void_p(a.__array_interface__["data"][0])
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))
