"""ctypes binding of the C-ABI in include/sfm_hip.h (libsfm_hip.so, gfx950).

Every C signature is written once, in the ``SIGNATURES`` table below; ``load()`` applies it and ``EXPORTS`` is its keys.
There is no CPU fallback: ``load()`` raises if the library is missing, and every compute call
raises if no MI355X is visible.  Status codes map back to the exceptions the reference raises
(``ValueError`` for bad shapes / invalid rotations, utils.py:43-51, 93-95).
"""
import ctypes
import os
from types import SimpleNamespace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SFM_HIP_LIBRARY selects another build of the same library (tools/asan_host_check.sh points it at the
# -fsanitize=address,undefined host build); the default is the in-tree gfx950 build next to this file.
LIB_PATH = os.environ.get("SFM_HIP_LIBRARY") or os.path.join(_HERE, "libsfm_hip.so")

OK = 0
E_SHAPE, E_BAD_ROTATION, E_QW_ZERO, E_SQRT_DOMAIN, E_HIP, E_NO_DEVICE, E_HANDLE, E_RANK, E_RCCL = -1, -2, -3, -4, -5, -6, -7, -8, -9
E_SINGULAR = -10
Q1_PNP_ROW_OVERLAP, Q2_LOC_JAC_SIGN, QUIRKS_REFERENCE = 1, 2, 3
SCHUR_AUTO, SCHUR_PAIRS, SCHUR_MFMA, SCHUR_ROWS = 0, 1, 2, 3
OPT_SCHUR, OPT_TIMING, OPT_DEBUG, OPT_DETERMINISTIC, OPT_GRAPH, OPT_TIMING_STRIDE = 1, 2, 3, 4, 5, 6
K_PREP, K_LINEARIZE, K_SCHUR, K_SOLVE, K_BACKSUB, K_REDUCE, K_COUNT = 0, 1, 2, 3, 4, 5, 6
KERNEL_NAMES = ("prep", "linearize", "schur", "solve", "backsub", "reduce")
INFO_SCHUR_KERNEL, INFO_UPLOAD_BYTES, INFO_N_CAMS, INFO_N_PTS, INFO_N_OBS, INFO_MAX_TRACK, INFO_GRAPH_REPLAYS = 1, 2, 3, 4, 5, 6, 7
INFO_REDUCE_IN_SOLVE = 8
INFO_PCG_HELD_POINTS = 9
INFO_SOLVE_PATH = 10
SOLVE_SMALL, SOLVE_FLOW, SOLVE_STEPS = 0, 1, 2
PCG_CONVERGED, PCG_MAX_ITERS, PCG_BREAKDOWN = 0, 1, 2
LM_STOP_MAX_TRIALS, LM_STOP_FTOL, LM_STOP_XTOL, LM_STOP_GTOL, LM_STOP_LAMBDA_MAX, LM_STOP_BREAKDOWN, LM_STOP_SINGULAR = 0, 1, 2, 3, 4, 5, 6
LM_STOP_NAMES = ("max_trials", "ftol", "xtol", "gtol", "lambda_max", "breakdown", "singular")
LM_MIN_GAIN = 1e-3
MATCH_L2, MATCH_HAMMING = 0, 1
MATCH_KNN2, MATCH_NN1, MATCH_MUTUAL = 0, 1, 2
GUIDE_NONE, GUIDE_FUNDAMENTAL, GUIDE_HOMOGRAPHY = 0, 1, 2
DESC_U8, DESC_F32 = 0, 1
DESC_INFO_N, DESC_INFO_DIM, DESC_INFO_EXACT, DESC_INFO_UPLOAD_BYTES = 1, 2, 3, 4
SIFT_INFO_N, SIFT_INFO_N_OCTAVES, SIFT_INFO_N_PRE, SIFT_INFO_N_LAYERS, SIFT_INFO_KEEPS_PYRAMID = 1, 2, 3, 4, 5
SIFT_LEVEL_GAUSS, SIFT_LEVEL_DOG = 0, 1
TRACK_INFO_N_VIEWS, TRACK_INFO_N_KEYS, TRACK_INFO_N_ROWS, TRACK_INFO_UPLOAD_BYTES, TRACK_INFO_DOWNLOAD_BYTES = 1, 2, 3, 4, 5
TRACK_INFO_OBS_VIEWS, TRACK_INFO_OBS_PTS, TRACK_INFO_N_OBS = 6, 7, 8
TRACK_OK, TRACK_NO_SECOND, TRACK_ZERO_SECOND, TRACK_BAD_TRAIN = 0, 1, 2, 3
SYNC_REUSE, SYNC_GROWN, SYNC_REPLACED = 0, 1, 2
TRACKS_LINEAR, TRACKS_NONLINEAR = 1, 2
TRACK_TOO_FEW, TRACK_NONFINITE, TRACK_BEHIND = 1, 2, 4
TRACK_GROUPS = (0, 1, 4, 8, 16, 32, 64)
OBS_HIGH_ERROR, OBS_BEHIND, OBS_NONFINITE, OBS_POINT = 1, 2, 4, 8
PT_TOO_FEW, PT_LOW_ANGLE, PT_EMPTY = 1, 2, 4
RANSAC_TOO_FEW, RANSAC_NO_MODEL, RANSAC_KEPT_HYPOTHESIS, RANSAC_SAMPLED = 1, 2, 4, 8
RANSAC_MAX_HYP, RANSAC_DEFAULT_HYP = 65536, 128
RANSAC_SUMMARY = ("pts_solved", "pts_no_model", "pts_too_few", "pts_kept_hypothesis", "obs_inlier", "obs_outlier")
RESECT_TOO_FEW, RESECT_NO_MODEL, RESECT_KEPT_HYPOTHESIS, RESECT_SAMPLED, RESECT_HELD = 1, 2, 4, 8, 16
RESECT_MAX_HYP, RESECT_DEFAULT_HYP, RESECT_MAX_OBS = 65536, 128, 1 << 20
RESECT_SUMMARY = ("cams_solved", "cams_no_model", "cams_too_few", "cams_kept_hypothesis", "obs_inlier", "obs_outlier")
TWOVIEW_TOO_FEW, TWOVIEW_NO_MODEL, TWOVIEW_KEPT_HYPOTHESIS = 1, 2, 4
TWOVIEW_MAX_HYP, TWOVIEW_DEFAULT_HYP, TWOVIEW_MIN_MATCHES = 65536, 128, 9
TWOVIEW_SUMMARY = ("sets_solved", "sets_no_model", "sets_too_few", "sets_kept_hypothesis", "matches_inlier", "matches_outlier")
TWOVIEW_OUTPUTS = ("inlier", "n_inliers", "best_hyp", "status", "summary")
HOMOGRAPHY_TOO_FEW, HOMOGRAPHY_NO_MODEL, HOMOGRAPHY_KEPT_HYPOTHESIS = 1, 2, 4
HOMOGRAPHY_MAX_HYP, HOMOGRAPHY_DEFAULT_HYP, HOMOGRAPHY_MIN_MATCHES = 65536, 128, 5
HOMOGRAPHY_SUMMARY = TWOVIEW_SUMMARY
HOMOGRAPHY_OUTPUTS = TWOVIEW_OUTPUTS
ESSENTIAL_TOO_FEW, ESSENTIAL_NO_MODEL = 1, 2
ESSENTIAL_MAX_HYP, ESSENTIAL_DEFAULT_HYP, ESSENTIAL_MIN_MATCHES, ESSENTIAL_MAX_SOLUTIONS = 65536, 128, 6, 10
ESSENTIAL_SUMMARY = ("sets_solved", "sets_no_model", "sets_too_few", "unused", "matches_inlier", "matches_outlier")
ESSENTIAL_OUTPUTS = ("F", "inlier", "n_inliers", "best_hyp", "best_root", "n_valid", "status", "summary")
SIMILARITY_TOO_FEW, SIMILARITY_NO_MODEL, SIMILARITY_KEPT_HYPOTHESIS = 1, 2, 4
SIMILARITY_RIGID = 1
SIMILARITY_MAX_HYP, SIMILARITY_DEFAULT_HYP, SIMILARITY_MIN_SET = 65536, 128, 4
SIMILARITY_SUMMARY = ("sets_solved", "sets_no_model", "sets_too_few", "sets_kept_hypothesis", "pairs_inlier", "pairs_outlier")
SIMILARITY_OUTPUTS = TWOVIEW_OUTPUTS
ROTAVG_NO_MODEL, ROTAVG_KEPT_HYPOTHESIS, ROTAVG_CG_LIMIT = 1, 2, 4
ROTAVG_UNREACHED, ROTAVG_HELD = 1, 2
ROTAVG_MAX_HYP, ROTAVG_DEFAULT_HYP = 65536, 128
ROTAVG_SUMMARY = ("views_with_rotation", "views_unreached", "views_held", "edges_inlier", "edges_outlier", "rounds_stood")
ROTAVG_OUTPUTS = ("edge_inlier", "edge_cos", "view_status", "n_inliers", "best_hyp", "status", "summary")
TRANSAVG_NO_MODEL, TRANSAVG_KEPT_ROUNDS, TRANSAVG_CG_LIMIT = 1, 2, 4
TRANSAVG_NO_ROTATION, TRANSAVG_UNREACHED, TRANSAVG_HELD = 1, 2, 4
TRANSAVG_SUMMARY = ("views_with_position", "views_no_rotation", "views_unreached", "views_held", "edges_inlier", "edges_used_outlier")
TRANSAVG_OUTPUTS = ("edge_inlier", "edge_cos", "edge_len", "view_status", "n_inliers", "status", "summary", "log")
LINK_UNMATCHED, LINK_SHORT, LINK_CONFLICT = -1, -2, -3
LINK_SUMMARY = ("matches_used", "components", "tracks", "conflicts", "short", "observations", "longest_track", "largest_component")
LINK_OUTPUTS = ("key_track", "pt_ptr", "cam_idx", "key_idx", "summary", "label")
LINK_PLAN = ("union_grid", "group", "order_grid", "big_grid", "scan_keys", "tiles_keys", "scan_components", "tiles_components")
LINK_SCAN_AUTO, LINK_SCAN_ONE_BLOCK, LINK_SCAN_DEVICE = 0, 1, 2
TRIPLET_SUMMARY = ("triplets", "triplets_consistent", "edges_tested", "edges_kept", "edges_dropped", "edges_untested", "edges_masked",
                   "largest_n_tri")
TRIPLET_OUTPUTS = ("edge_keep", "n_tri", "n_ok", "kept_idx", "summary")
RETRIEVE_MAX_WORDS, RETRIEVE_MAX_LEN, RETRIEVE_MAX_DIM, RETRIEVE_MAX_VIEWS, RETRIEVE_MAX_K, RETRIEVE_MAX_ITERS = 1024, 131072, 256, 65536, 64, 64
RETRIEVE_MAX_VIEW_KEYS, RETRIEVE_CAP_DEFAULT, RETRIEVE_CAP_MAX = 1 << 22, 1 << 20, 1 << 22
PAIR_HOW_FORWARD, PAIR_HOW_BACKWARD, PAIR_HOW_SEQUENTIAL = 1, 2, 4
DESCRIBE_OUTPUTS = ("desc", "norm2", "word_count", "assign", "residual")
PAIRS_OUTPUTS = ("nbr", "nbr_score", "pairs", "how", "pair_score", "dot")
POSE_FROM_F, POSE_FROM_H = 0, 1
POSE_EMPTY, POSE_NO_MODEL, POSE_NO_POSE, POSE_TIED, POSE_NO_PARALLAX = 1, 2, 4, 8, 16
POSE_CANDIDATES = 4
POSE_KINDS = {"fundamental": POSE_FROM_F, "homography": POSE_FROM_H}
POSE_SUMMARY = ("sets_posed", "sets_no_pose", "sets_empty", "sets_tied", "matches_front", "matches_not_front")
POSE_OUTPUTS = ("normal", "cand_front", "n_front", "n_parallax", "best_cand", "status", "obs_front", "X", "summary")
REFINE_EMPTY, REFINE_TOO_FEW, REFINE_BAD_POSE, REFINE_SINGULAR, REFINE_NONFINITE, REFINE_KEPT_INPUT = 1, 2, 4, 8, 16, 32
REFINE_MIN_USED = 8
REFINE_SUMMARY = ("sets_refined", "sets_bad_pose", "sets_too_few", "sets_kept_input", "matches_inlier", "matches_not_inlier")
REFINE_OUTPUTS = ("F", "cost", "info", "n_used", "status", "obs_res", "obs_inlier", "obs_front", "X", "n_inliers", "n_front", "n_parallax",
                  "summary")
LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2
CAM_EMPTY, CAM_NONFINITE, CAM_BEHIND, CAM_HELD = 1, 2, 4, 8
COV_CAM_HELD, COV_CAM_PIVOT, COV_PT_EMPTY, COV_PT_SINGULAR = 8, 16, 4, 8
LOSS_NAMES = {"none": LOSS_NONE, "huber": LOSS_HUBER, "cauchy": LOSS_CAUCHY}
SCREEN_SUMMARY = ("obs_before", "obs_kept", "high_error", "behind", "nonfinite", "obs_dropped_with_point", "pts_too_few",
                  "pts_low_angle")

_lib = None
vp, ci, cd, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
_dp = ctypes.POINTER(cd)
_ip = ctypes.POINTER(ci)
fp = ctypes.POINTER(ctypes.c_float)
_lp = ctypes.POINTER(i64)
_pp = ctypes.POINTER(vp)


# sfm_sift_params of the SIFT detection below (the signature table names it)
class SiftParams(ctypes.Structure):
    _fields_ = [("n_octave_layers", ctypes.c_int), ("contrast_threshold", ctypes.c_double),
                ("edge_threshold", ctypes.c_double), ("sigma", ctypes.c_double), ("keep_pyramid", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


# sfm_lm_options / sfm_lm_trial of the controlled minimisation (sfm_ba_minimize_pcg)
class LmOptions(ctypes.Structure):
    _fields_ = [("lambda0", ctypes.c_double), ("lambda_min", ctypes.c_double), ("lambda_max", ctypes.c_double),
                ("ftol", ctypes.c_double), ("xtol", ctypes.c_double), ("gtol", ctypes.c_double),
                ("cg_tol", ctypes.c_double), ("cg_max_iters", ctypes.c_int), ("max_trials", ctypes.c_int),
                ("quirks", ctypes.c_int), ("group", ctypes.c_int)]


class LmTrial(ctypes.Structure):
    _fields_ = [("lam", ctypes.c_double), ("cost", ctypes.c_double), ("cost_trial", ctypes.c_double),
                ("predicted", ctypes.c_double), ("rho", ctypes.c_double), ("step_norm", ctypes.c_double),
                ("grad_inf", ctypes.c_double), ("cg_rel", ctypes.c_double), ("cg_iters", ctypes.c_int),
                ("cg_status", ctypes.c_int), ("accepted", ctypes.c_int), ("reserved", ctypes.c_int)]


LM_TRIAL_DTYPE = np.dtype([(name, np.float64 if t is ctypes.c_double else np.int32) for name, t in LmTrial._fields_])
LM_DEFAULTS = dict(lambda0=5.0, lambda_min=1e-8, lambda_max=1e8, ftol=1e-8, xtol=0.0, gtol=0.0, cg_tol=1e-10, cg_max_iters=0,
                   max_trials=50, quirks=QUIRKS_REFERENCE, group=0)


# The one place a C signature is written down on this side: every symbol include/sfm_hip.h declares -> its argument types
# (tests/test_abi_and_host.py compares names and argument counts with the header).  load() applies the table; every
# function returns int except sfm_last_error.
SIGNATURES = {
    "sfm_version": [],
    "sfm_init": [ci],
    "sfm_shutdown": [],
    "sfm_set_stream": [vp],
    "sfm_synchronize": [],
    "sfm_set_cu_limit": [ci],
    "sfm_cu_count": [_ip, _ip],
    "sfm_last_error": [],
    "sfm_quat_to_rot": [ci, _dp, _dp, _ip],
    "sfm_rot_to_quat": [ci, _dp, _dp, _ip],
    "sfm_jac_cam": [ci, _dp, _dp, _dp, ci, _dp, _ip],
    "sfm_jac_pt": [ci, ci, _dp, _dp, _dp],
    "sfm_tri_nonlinear": [ci, ci, _dp, _dp, _dp, cd, ci, _dp],
    "sfm_tri_linear": [ci, ci, _dp, _dp, _dp],
    "sfm_triangulate": [ci, ci, _dp, _dp, cd, ci, _dp],
    "sfm_pnp_nonlinear": [ci, _dp, _dp, _dp, _dp, _dp, cd, ci, ci, _dp, _dp],
    "sfm_pnp_nonlinear_batch": [ci, _ip, ci, _dp, _dp, _dp, _dp, _dp, cd, ci, ci, _dp, _dp, _ip],
    "sfm_pnp_linear_ransac": [ci, _dp, _dp, _dp, ci, _ip, cd, _dp, _dp, _ip, _ip, _ip],
    "sfm_pnp_six_point_hypotheses": [ci, _dp, _dp, _dp, ci, _ip, cd, _dp, _dp, _ip],
    "sfm_pnp_ransac_evaluate": [ci, _dp, _dp, _dp, ci, _ip, cd, _dp, _dp, _ip, _ip],
    "sfm_pnp_inlier_mask": [ci, _dp, _dp, _dp, _dp, _dp, cd, _ip, _ip],
    "sfm_pnp_ransac_begin": [ci, _dp, _dp, _dp, ci, _ip, cd, _dp, _dp, _ip, _ip, _pp],
    "sfm_pnp_ransac_finish": [vp, _dp, _dp, cd, cd, ci, ci, _ip, _ip, _dp, _dp],
    "sfm_pnp_session_destroy": [vp],
    "sfm_comm_available": [],
    "sfm_comm_unique_id": [ctypes.c_char_p],
    "sfm_comm_create": [ci, ci, ctypes.c_char_p, _pp],
    "sfm_comm_destroy": [vp],
    "sfm_ba_set_comm": [vp, vp],
    "sfm_fundamental_ransac": [ci, _dp, _dp, ci, _ip, cd, _dp, _ip, _ip, _ip],
    "sfm_fundamental_eight_point": [ci, _dp, ci, _ip, _dp, _ip],
    "sfm_essential_from_fundamental": [_dp, _dp, _dp, _dp],
    "sfm_pose_candidates": [_dp, _dp, _dp],
    "sfm_cheirality": [ci, ci, _dp, _dp, _dp, _ip, _ip, _ip],
    "sfm_ba_solve": [ci, ci, i64, _ip, _ip, _dp, _dp, _dp, cd, ci, ci],
    "sfm_ba_create": [ci, ci, i64, _ip, _ip, _dp, _pp],
    "sfm_ba_destroy": [vp],
    "sfm_ba_set_option": [vp, ci, ci],
    "sfm_ba_set_state": [vp, _dp, _dp],
    "sfm_ba_set_stream": [vp, vp],
    "sfm_ba_info": [vp, ci, _lp],
    "sfm_ba_set_cameras": [vp, _dp],
    "sfm_ba_set_points": [vp, ci, ci, _dp],
    "sfm_ba_get_stats": [vp, _dp, ci, _ip],
    "sfm_ba_flush": [vp],
    "sfm_pool_redzone_active": [],
    "sfm_ba_iterate": [vp, cd, ci, ci],
    "sfm_ba_get_state": [vp, _dp, _dp],
    "sfm_ba_append": [vp, ci, _dp, ci, _dp, i64, _ip, _ip, _dp],
    "sfm_ba_kernel_time": [vp, ci, _dp, _ip],
    "sfm_ba_reset_timing": [vp],
    "sfm_ba_debug_stamps": [vp, ctypes.POINTER(ctypes.c_uint64), ci],
    "sfm_ba_linearize_reduce": [vp, cd, ci],
    "sfm_ba_solve_update": [vp, cd, ci],
    "sfm_ba_reduced_buffer": [vp, _pp, _lp, _ip],
    "sfm_ba_bind_reduced_buffer": [vp, vp, i64],
    "sfm_ba_residual_jacobian": [ci, ci, i64, _ip, _ip, _dp, _dp, _dp, ci, _dp, _dp, _dp],
    "sfm_ba_reduced_system": [ci, ci, i64, _ip, _ip, _dp, _dp, _dp, cd, ci, ci, _dp, _dp],
    "sfm_pool_mode": [i64, _lp, _lp],
    "sfm_tri_nonlinear_dev": [ci, ci, vp, vp, vp, cd, ci, vp, vp],
    "sfm_tri_linear_dev": [ci, ci, vp, vp, vp, vp],
    "sfm_triangulate_dev": [ci, ci, vp, vp, cd, ci, vp, vp],
    "sfm_pnp_nonlinear_batch_dev": [ci, vp, ci, vp, vp, vp, vp, vp, cd, ci, ci, vp, vp, vp, ci, vp],
    "sfm_gather_points_dev": [ci, vp, vp, vp, vp, vp, vp],
    "sfm_ba_points_ptr": [vp, _pp, _pp, _pp, _ip],
    "sfm_ba_stream": [vp, _pp],
    "sfm_ba_event_overhead": [vp, ci, _dp],
    "sfm_ba_get_state_rot": [vp, _dp, _dp, _dp],
    "sfm_ba_rederive_quaternions": [vp, ci, ci],
    "sfm_ba_flow_tasks": [ci, _ip, ci],
    "sfm_ba_flow_grid": [ci, ci],
    "sfm_ba_flow_tasks_deferred": [ci, _ip, ci],
    "sfm_desc_create": [ci, ci, ci, ci, vp, _pp],
    "sfm_desc_destroy": [vp],
    "sfm_desc_info": [vp, ci, _lp],
    "sfm_match": [vp, ci, _pp, ci, _ip, fp, _ip, fp, ctypes.POINTER(ctypes.c_uint8)],
    "sfm_match_dev": [vp, ci, _pp, ci, vp, vp, vp, vp, vp, vp],
    "sfm_match_guided": [vp, _dp, _dp, ci, _pp, _pp, _pp, _ip, _dp, cd, vp, vp, vp, vp, vp, vp],
    "sfm_match_guided_dev": [vp, vp, vp, ci, _pp, _pp, _pp, _ip, _dp, cd, vp, vp, vp, vp, vp, vp, vp],
    "sfm_homography_adjugate": [_dp, _dp],
    "sfm_sift_detect": [vp, ci, ci, ci, i64, ctypes.POINTER(SiftParams), _pp],
    "sfm_sift_result_info": [vp, ci, _lp],
    "sfm_sift_result_level_shape": [vp, ci, _ip, _ip],
    "sfm_sift_result_copy": [vp, fp, fp, fp, fp, fp, _ip, fp],
    "sfm_sift_result_copy_pre": [vp, fp, fp, fp, fp, _ip],
    "sfm_sift_result_copy_level": [vp, ci, ci, ci, fp],
    "sfm_sift_result_destroy": [vp],
    "sfm_sift_blur_kernel": [cd, ci, fp, _ip],
    "sfm_track_create": [_pp],
    "sfm_track_destroy": [vp],
    "sfm_track_info": [vp, ci, ci, _lp],
    "sfm_track_add_view": [vp, ci, _dp, _dp, _ip],
    "sfm_track_drop_last_view": [vp],
    "sfm_track_match_dedup_dev": [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp],
    "sfm_track_extend_dev": [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp],
    "sfm_track_match_views": [vp, ci, vp, ci, _pp, ci, ci, vp],
    "sfm_track_extend_status": [vp, ci, _ip, _ip, _ip],
    "sfm_track_kept_copy": [vp, ci, _ip, _ip],
    "sfm_track_write_kept": [vp, ci, ci, vp],
    "sfm_track_pairs_dev": [vp, ci, ci, vp, vp, vp, vp, vp, vp],
    "sfm_track_pairs": [vp, ci, ci, _ip, _ip, _ip, _dp, _dp],
    "sfm_track_update_usage": [vp, ci, ci, _ip, _ip],
    "sfm_match_guided_track": [vp, ci, vp, ci, _ip, _pp, _ip, _dp, cd, vp, vp, vp, vp, vp, vp, vp],
    "sfm_match_guided_set_pairs": [vp, ci, ci, ci, _ip, _ip],
    "sfm_track_constructed": [vp, ci, _ip, _ip, _ip],
    "sfm_track_unconstructed": [vp, ci, _ip, _ip],
    "sfm_track_copy_table": [vp, ci, _ip],
    "sfm_track_copy_row": [vp, ci, ci, _ip],
    "sfm_obs_set_normalised": [vp, ci, ci, _dp, _dp],
    "sfm_obs_build": [vp, ci, ci, _lp],
    "sfm_obs_copy": [vp, _ip, _ip, _ip, _dp],
    "sfm_ba_create_from_tracks": [vp, _pp],
    "sfm_ba_sync_tracks": [vp, vp, ci, _dp, ci, _dp, _ip, _lp],
    "sfm_ba_get_structure": [vp, _ip, _ip, _dp],
    "sfm_tri_tracks": [ci, ci, i64, _ip, _ip, _dp, _dp, ci, cd, ci, ci, _dp, _dp, _dp, _ip],
    "sfm_tri_tracks_dev": [ci, ci, i64, vp, vp, vp, vp, ci, cd, ci, ci, vp, vp, vp, vp, vp],
    "sfm_ba_refine_points": [vp, ci, cd, ci, ci, _dp, _ip],
    "sfm_tri_tracks_auto_group": [ci, i64, ci],
    "sfm_tri_tracks_ransac": [ci, ci, i64, _ip, _ip, _dp, _dp, _dp, cd, cd, ci, cd, ci, ci, _dp, _dp,
                              ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_tri_tracks_ransac_dev": [ci, ci, i64, vp, vp, vp, vp, vp, cd, cd, ci, cd, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp],
    "sfm_ba_retriangulate": [vp, cd, cd, ci, cd, ci, ci, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_tri_ransac_pair": [ci, ci, ci, _ip, _ip],
    "sfm_ba_screen": [vp, cd, cd, ci, ci, _dp, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), _dp, _ip, _lp],
    "sfm_ba_cull": [vp, cd, cd, ci, ci, _dp, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), _dp, _ip, _lp],
    "sfm_ba_set_loss": [vp, ci, cd],
    "sfm_ba_get_loss": [vp, _ip, _dp],
    "sfm_ba_loss_terms": [vp, _dp, _dp, _dp],
    "sfm_ba_reduced_system_loss": [ci, ci, i64, _ip, _ip, _dp, _dp, _dp, cd, ci, ci, ci, cd, _dp, _dp],
    "sfm_ba_refine_cameras": [vp, cd, ci, ci, ci, ctypes.POINTER(ctypes.c_uint8), _dp, _ip],
    "sfm_ba_refine_cameras_plan": [i64, _ip, _ip, _ip],
    "sfm_resect_ransac": [ci, _ip, i64, _dp, _dp, _dp, cd, ci, cd, ci, ci, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_resect_ransac_dev": [ci, _ip, i64, vp, vp, vp, cd, ci, cd, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp],
    "sfm_ba_resect": [vp, cd, ci, cd, ci, ci, ctypes.POINTER(ctypes.c_uint8), _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_resect_triple": [ci, ci, ci, _ip, _ip, _ip],
    "sfm_twoview_ransac": [ci, _ip, i64, _dp, _dp, cd, ci, ci, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_twoview_ransac_dev": [ci, _ip, i64, vp, vp, cd, ci, ci, vp, vp, vp, vp, vp, vp, vp],
    "sfm_twoview_sample": [ci, ci, ci, _ip],
    "sfm_homography_ransac": [ci, _ip, i64, _dp, _dp, cd, ci, ci, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_homography_ransac_dev": [ci, _ip, i64, vp, vp, cd, ci, ci, vp, vp, vp, vp, vp, vp, vp],
    "sfm_homography_sample": [ci, ci, ci, _ip],
    "sfm_essential_ransac": [ci, _ip, i64, _dp, _dp, _dp, _dp, cd, ci, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _ip,
                             _ip, _lp],
    "sfm_essential_ransac_dev": [ci, _ip, i64, vp, vp, _dp, _dp, cd, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "sfm_essential_sample": [ci, ci, ci, _ip],
    "sfm_essential_solve": [_dp, _dp, _dp, _ip],
    "sfm_similarity_ransac": [ci, _ip, i64, _dp, _dp, cd, ci, ci, ci, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip, _lp],
    "sfm_similarity_ransac_dev": [ci, _ip, i64, vp, vp, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp],
    "sfm_similarity_sample": [ci, ci, ci, _ip],
    "sfm_rotation_average": [ci, i64, _ip, _dp, ci, cd, ci, ci, ci, cd, ci, _dp, ctypes.POINTER(ctypes.c_uint8), _dp, _ip, _ip, _ip, _ip, _lp],
    "sfm_rotation_average_dev": [ci, i64, _ip, vp, ci, cd, ci, ci, ci, cd, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "sfm_rotation_tree": [ci, i64, _ip, ci, ci, ci, _ip, _ip],
    "sfm_rotation_edge_test": [_dp, _dp, _dp, cd, _dp],
    "sfm_rotation_plan": [ci, ci, i64, _ip, _ip],
    "sfm_translation_average": [ci, i64, _ip, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), ci, cd, cd, ci, ci, cd, ci, _dp,
                                ctypes.POINTER(ctypes.c_uint8), _dp, _dp, _ip, _ip, _ip, _lp, _dp],
    "sfm_translation_average_dev": [ci, i64, _ip, vp, vp, vp, ci, cd, cd, ci, ci, cd, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "sfm_translation_edge_test": [_dp, _dp, _dp, cd, _dp, _dp],
    "sfm_link_tracks": [ci, _ip, ci, _ip, _lp, _ip, _ip, ctypes.POINTER(ctypes.c_uint8), ci, ci, ci, _ip, _ip, _ip, _ip, _lp, _ip],
    "sfm_link_tracks_dev": [ci, _ip, ci, _ip, _lp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, _ip, _lp, vp],
    "sfm_link_tracks_plan": [ci, i64, i64, ci, ci, _ip],
    "sfm_link_tracks_views": [vp, ci, _ip, ctypes.POINTER(ctypes.c_uint8), ci, vp, _lp],
    "sfm_view_triplets": [ci, i64, _ip, _dp, ctypes.POINTER(ctypes.c_uint8), cd, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_uint8), _lp, _lp,
                          _ip, _lp, _ip],
    "sfm_view_triplets_dev": [ci, i64, _ip, vp, vp, cd, ci, ci, ci, ci, vp, vp, vp, vp, vp, _ip, vp],
    "sfm_view_triplet_test": [_dp, _dp, _dp, cd, _dp],
    "sfm_vocab_train": [ci, _pp, ci, ci, ctypes.c_uint64, i64, ctypes.POINTER(ctypes.c_uint8), _lp],
    "sfm_vocab_init_rows": [i64, ci, ctypes.c_uint64, i64, _lp],
    "sfm_view_describe": [vp, ci, _pp, ctypes.POINTER(ctypes.c_int8), _lp, _ip, _ip, _ip],
    "sfm_view_describe_dev": [vp, ci, _pp, vp, vp, vp, vp, vp, vp],
    "sfm_view_pairs": [ci, ci, ctypes.POINTER(ctypes.c_int8), _lp, ci, cd, ci, ci, i64, _ip, _dp, _ip, _ip, _dp, _ip, _lp],
    "sfm_view_pairs_dev": [ci, ci, vp, vp, ci, cd, ci, ci, i64, vp, vp, vp, vp, vp, vp, _lp, vp],
    "sfm_view_score": [ci, i64, i64, _dp],
    "sfm_ba_transform": [vp, cd, _dp, _dp],
    "sfm_ba_align": [vp, ci, _ip, _dp, cd, ci, ci, ci, ci, _dp, ctypes.POINTER(ctypes.c_uint8), _ip, _ip, _ip],
    "sfm_twoview_pose": [ci, _ip, i64, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), _dp, _ip, _dp, _dp, cd, ci, _dp, _dp, _dp, _ip, _ip, _ip,
                         _ip, _ip, ctypes.POINTER(ctypes.c_uint8), _dp, _lp],
    "sfm_twoview_pose_dev": [ci, _ip, i64, vp, vp, vp, _dp, _ip, _dp, _dp, cd, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "sfm_twoview_pose_test": [_dp, _dp, _dp, _dp, cd, _ip, _ip],
    "sfm_twoview_pose_pairs": [vp, ci, ci, ctypes.POINTER(ctypes.c_uint8), _dp, ci, _dp, _dp, cd, ci, _ip, _ip, _ip, _dp, _dp, _dp, _ip,
                               _ip, _ip, _ip, _ip, ctypes.POINTER(ctypes.c_uint8), _dp],
    "sfm_twoview_refine": [ci, _ip, i64, _dp, _dp, ctypes.POINTER(ctypes.c_uint8), _dp, _dp, _dp, _dp, cd, ci, cd, cd, _dp, _dp, _dp, _dp, _dp,
                           _ip, _ip, _dp, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), _dp, _ip, _ip, _ip, _lp],
    "sfm_twoview_refine_dev": [ci, _ip, i64, vp, vp, vp, vp, vp, _dp, _dp, cd, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                               vp, vp, vp, vp],
    "sfm_twoview_refine_test": [_dp, _dp, _dp, _dp, cd, cd, cd, cd, _dp, _dp],
    "sfm_twoview_refine_pairs": [vp, ci, ci, ctypes.POINTER(ctypes.c_uint8), _dp, _dp, _dp, _dp, cd, ci, cd, cd, _ip, _ip, _ip, _dp, _dp,
                                 _dp, _dp, _dp, _ip, _ip, _dp, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), _dp, _ip,
                                 _ip, _ip],
    "sfm_twoview_verify_pairs": [vp, ci, ci, cd, ci, ci, _ip, _ip, _ip, ctypes.POINTER(ctypes.c_uint8), _dp, _ip, _ip],
    "sfm_ba_covariance": [vp, cd, ci, ci, ctypes.POINTER(ctypes.c_uint8), ci, _dp, _dp, _ip, _ip, _dp],
    "sfm_ba_covariance_plan": [ci, _ip, _ip, _ip, _ip],
    "sfm_ba_covariance_times": [vp, _dp],
    "sfm_ba_iterate_pcg": [vp, cd, ci, ci, ctypes.POINTER(ctypes.c_uint8), cd, ci, ci, _ip, _dp, _ip, _dp, _ip, _ip],
    "sfm_ba_pcg_times": [vp, _dp],
    "sfm_ba_cost": [vp, ci, ci, _dp],
    "sfm_lm_options_default": [ctypes.POINTER(LmOptions)],
    "sfm_lm_trial_size": [],
    "sfm_ba_minimize_pcg": [vp, ctypes.POINTER(LmOptions), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(LmTrial), _ip, _ip, _ip,
                            _dp, _dp, _ip],
}
EXPORTS = tuple(SIGNATURES)


class SfmHipError(RuntimeError):
    """HIP / device / handle failures (no reference counterpart)."""


class SfmSingularError(SfmHipError):
    """SFM_E_SINGULAR: a system that has to be positive definite is not; ``camera`` names where it was found."""

    def __init__(self, message, camera=None):
        super().__init__(message)
        self.camera = camera


def load():
    """Load libsfm_hip.so (built in-tree by ``__graft_entry__.build()`` / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SfmHipError(
            "libsfm_hip.so not found at %s — build it with `make -C %s` (there is no CPU fallback)"
            % (LIB_PATH, os.path.join(_HERE, "csrc")))
    # When PyTorch is in the process it must load its ROCm runtime FIRST: torch bundles its own
    # libamdhip64/libhsa-runtime64, and two HSA runtimes in one process leave the second one without
    # devices ("no ROCm-capable device is detected").  With torch imported first, libsfm_hip.so binds to
    # the already-loaded runtime and both share streams and device memory.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_char_p if name == "sfm_last_error" else ci
    _lib = lib
    return lib


def last_error():
    return load().sfm_last_error().decode("utf-8", "replace")


def check(status):
    """Map a C-ABI status to the exception the reference would raise."""
    if status == OK:
        return
    msg = last_error()
    if status == E_BAD_ROTATION:
        raise ValueError("convert_quaternion_to_rotation : Invalid output rotation matrix (%s)" % msg)
    if status == E_QW_ZERO:
        raise ValueError("convert_rotation_to_quaternion : Invalid output qw (%s)" % msg)
    if status == E_SQRT_DOMAIN:
        raise ValueError("math domain error (%s)" % msg)
    if status == E_SHAPE:
        raise ValueError(msg)
    if status == E_RANK:
        raise ValueError(msg)
    raise SfmHipError("libsfm_hip status %d: %s" % (status, msg))


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def dptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None      # None: an optional array the caller leaves out


def iptr(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def _lptr(a):
    return a.ctypes.data_as(_lp) if a is not None else None


def init(device=0):
    check(load().sfm_init(int(device)))


def set_stream(stream_ptr):
    check(load().sfm_set_stream(ctypes.c_void_p(stream_ptr) if stream_ptr else None))


def synchronize():
    check(load().sfm_synchronize())


def set_cu_limit(n):
    """Make every launch shape and plan for min(n, the device's compute units); 0 removes the limit (sfm_set_cu_limit: a hook
    for tests, refused with ValueError while a BaProblem exists)."""
    check(load().sfm_set_cu_limit(int(n)))


def cu_count():
    """(the device's compute units -- 256 before init --, the count the plans see)."""
    dev, eff = ctypes.c_int(), ctypes.c_int()
    check(load().sfm_cu_count(ctypes.byref(dev), ctypes.byref(eff)))
    return int(dev.value), int(eff.value)


def flow_grid(n_cus, n_tasks):
    """Workgroups of the data-flow solve's launch on n_cus compute units for n_tasks tasks (host only); 0: no such launch."""
    return int(load().sfm_ba_flow_grid(int(n_cus), int(n_tasks)))


def _task_table(fn, n):
    rows = fn(int(n), None, 0)
    out = np.zeros((max(rows, 1), 4), dtype=np.int32)
    if rows > 0:
        fn(int(n), iptr(out), rows)
    return out[:rows]


def flow_tasks(nbk):
    """Task table of the data-flow reduced solve for nbk block columns (host only; no device call): (n, 4) int32 rows
    {type, row, column, sort key} in the order the workgroups take them."""
    return _task_table(load().sfm_ba_flow_tasks, nbk)


def flow_tasks_deferred(n_cams):
    """Task table of the data-flow solve for n_cams cameras when the split-K reduce rides in its launch (host only): rows
    {type, row, column, key}; type 5 = camera sums (camera, part), 6 = rows 8q..8q+7 (q = key & 3) of block (row, column) of S."""
    return _task_table(load().sfm_ba_flow_tasks_deferred, n_cams)


def pool_redzone_active():
    """True when the process runs with SFM_POOL_REDZONE=1 (device buffers between checked guard zones; tests only)."""
    return bool(load().sfm_pool_redzone_active())


def pool_mode(probe_bytes=1000):
    """(mode bits, mapped bytes behind a probe buffer, guard-mode allocations so far): bit 0 = SFM_POOL_REDZONE,
    bit 1 = SFM_POOL_GUARD (every buffer ends at the end of its own mapping, the next page is unmapped)."""
    slack = ctypes.c_int64(); allocs = ctypes.c_int64()
    mode = load().sfm_pool_mode(int(probe_bytes), ctypes.byref(slack), ctypes.byref(allocs))
    return mode, int(slack.value), int(allocs.value)


# ---- device-pointer, stream-ordered forms (pointers as integers, e.g. torch.Tensor.data_ptr()) ------------------
def _vp(ptr):
    return ctypes.c_void_p(int(ptr)) if ptr else None


def tri_nonlinear_dev(m, n_views, d_projs, d_uv, d_x_in, lam, iters, d_x_out, stream=0):
    check(load().sfm_tri_nonlinear_dev(int(m), int(n_views), _vp(d_projs), _vp(d_uv), _vp(d_x_in), float(lam), int(iters),
                                       _vp(d_x_out), _vp(stream)))


def tri_linear_dev(m, n_views, d_projs, d_uv, d_x_out, stream=0):
    check(load().sfm_tri_linear_dev(int(m), int(n_views), _vp(d_projs), _vp(d_uv), _vp(d_x_out), _vp(stream)))


def triangulate_dev(m, n_views, d_projs, d_uv, lam, iters, d_x_out, stream=0):
    check(load().sfm_triangulate_dev(int(m), int(n_views), _vp(d_projs), _vp(d_uv), float(lam), int(iters), _vp(d_x_out), _vp(stream)))


def pnp_nonlinear_batch_dev(n_views, d_offsets, total, d_uv_pix, d_x, d_k, d_r0, d_c0, lam, iters, quirks, d_r_out, d_c_out,
                            d_status, stream=0, max_view_points=0):
    check(load().sfm_pnp_nonlinear_batch_dev(int(n_views), _vp(d_offsets), int(total), _vp(d_uv_pix), _vp(d_x), _vp(d_k), _vp(d_r0),
                                             _vp(d_c0), float(lam), int(iters), int(quirks), _vp(d_r_out), _vp(d_c_out),
                                             _vp(d_status), int(max_view_points), _vp(stream)))


def gather_points_dev(n, d_index, d_px, d_py, d_pz, d_x_out, stream=0):
    check(load().sfm_gather_points_dev(int(n), _vp(d_index), _vp(d_px), _vp(d_py), _vp(d_pz), _vp(d_x_out), _vp(stream)))


# ------------------------------------------------------------------------------------------------
def quat_to_rot(q):
    q = f64(q).reshape(-1, 4)
    n = q.shape[0]
    rot = np.empty((n, 3, 3)); st = np.empty(n, dtype=np.int32)
    check(load().sfm_quat_to_rot(n, dptr(q), dptr(rot), iptr(st)))
    return rot, st


def rot_to_quat(rot):
    rot = f64(rot).reshape(-1, 3, 3)
    n = rot.shape[0]
    q = np.empty((n, 4)); st = np.empty(n, dtype=np.int32)
    check(load().sfm_rot_to_quat(n, dptr(rot), dptr(q), iptr(st)))
    return q, st


def jac_cam(rot, loc, pts_h, quirks=QUIRKS_REFERENCE):
    rot = f64(rot).reshape(-1, 3, 3); loc = f64(loc).reshape(-1, 3); pts_h = f64(pts_h).reshape(-1, 4)
    n = rot.shape[0]
    jp = np.empty((n, 2, 7)); st = np.empty(n, dtype=np.int32)
    check(load().sfm_jac_cam(n, dptr(rot), dptr(loc), dptr(pts_h), quirks, dptr(jp), iptr(st)))
    return jp, st


def jac_pt(projs, pts_h):
    projs = f64(projs); pts_h = f64(pts_h).reshape(-1, 4)
    n, nv = projs.shape[0], projs.shape[1]
    jx = np.empty((n, 2 * nv, 3))
    check(load().sfm_jac_pt(n, nv, dptr(projs), dptr(pts_h), dptr(jx)))
    return jx


def tri_nonlinear(projs, uv, x_in, lam, iters):
    """projs (V,3,4); uv (V,2,m); x_in (4,m) -> (4,m)."""
    projs = f64(projs); uv = f64(uv); x_in = f64(x_in)
    nv, m = projs.shape[0], x_in.shape[1]
    out = np.empty((4, m))
    check(load().sfm_tri_nonlinear(m, nv, dptr(projs), dptr(uv), dptr(x_in), float(lam), int(iters), dptr(out)))
    return out


def tri_linear(projs, uv):
    """DLT triangulation: projs (V,3,4); uv (V,2,m) -> (4,m) with W = 1."""
    projs = f64(projs); uv = f64(uv)
    nv, m = projs.shape[0], uv.shape[2]
    out = np.empty((4, m))
    check(load().sfm_tri_linear(m, nv, dptr(projs), dptr(uv), dptr(out)))
    return out


def triangulate(projs, uv, lam, iters):
    """Linear then nonlinear triangulation in one call (initial points stay on the device)."""
    projs = f64(projs); uv = f64(uv)
    nv, m = projs.shape[0], uv.shape[2]
    out = np.empty((4, m))
    check(load().sfm_triangulate(m, nv, dptr(projs), dptr(uv), float(lam), int(iters), dptr(out)))
    return out


def _check_group(group):
    """``group`` as an int, or ValueError: one of TRACK_GROUPS, and not a bool."""
    if isinstance(group, bool) or group not in TRACK_GROUPS:
        raise ValueError("group must be one of %s, got %r" % (TRACK_GROUPS, group))
    return int(group)


def _cam_mask(mask, n_cams):
    """A camera mask as a contiguous uint8 (n_cams,) array of 0 / 1 (None stays None), or ValueError."""
    if mask is None:
        return None
    mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).ravel()
    if mask.shape[0] != int(n_cams):
        raise ValueError("mask must have one entry per camera (%d), got %d" % (n_cams, mask.shape[0]))
    return mask


def _check_cam_scale(cam_scale, n_cams):
    """``cam_scale`` as a float64 (n_cams,) array of finite values (None stays None), or ValueError."""
    if cam_scale is None:
        return None
    cam_scale = f64(cam_scale)
    if cam_scale.shape != (int(n_cams),):
        raise ValueError("cam_scale must be (n_cams,) with n_cams = %d, got %s" % (n_cams, cam_scale.shape))
    if not np.all(np.isfinite(cam_scale)):
        raise ValueError("cam_scale must be finite")
    return cam_scale


def _u8ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if a is not None else None


def _tracks_mode_group(mode, iters, group):
    mode, iters, group = int(mode), int(iters), int(group)
    if mode not in (TRACKS_LINEAR, TRACKS_NONLINEAR, TRACKS_LINEAR | TRACKS_NONLINEAR):
        raise ValueError("mode must be TRACKS_LINEAR, TRACKS_NONLINEAR or both, got %d" % mode)
    if group not in TRACK_GROUPS:
        raise ValueError("group must be one of %s, got %d" % (TRACK_GROUPS, group))
    if iters < 0:
        raise ValueError("iters must be >= 0")
    return mode, iters, group


def check_tracks(pt_ptr, cam_idx, uv, projs, x_init, mode, iters, group):
    """Shapes and dtypes of a ``tri_tracks`` call, without a device: returns the converted arrays or raises ValueError."""
    mode, iters, group = _tracks_mode_group(mode, iters, group)
    for name, arr in (("pt_ptr", pt_ptr), ("cam_idx", cam_idx)):
        if not np.issubdtype(np.asarray(arr).dtype, np.integer):
            raise ValueError("%s must be an integer array" % name)
    pt_ptr = i32(pt_ptr); cam_idx = i32(cam_idx); uv = f64(uv); projs = f64(projs)
    if pt_ptr.ndim != 1 or pt_ptr.shape[0] < 1 or cam_idx.ndim != 1:
        raise ValueError("pt_ptr must be (n_pts + 1,) and cam_idx (M,)")
    n_pts, n_obs = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    if uv.shape != (2, n_obs):
        raise ValueError("uv must be (2, M) with M = %d, got %s" % (n_obs, uv.shape))
    if projs.ndim != 3 or projs.shape[0] < 1 or projs.shape[1:] != (3, 4):
        raise ValueError("projs must be (n_views, 3, 4), got %s" % (projs.shape,))
    if pt_ptr[0] != 0 or pt_ptr[-1] != n_obs:
        raise ValueError("pt_ptr must start at 0 and end at M = %d, got %d .. %d" % (n_obs, pt_ptr[0], pt_ptr[-1]))
    if x_init is None:
        if not mode & TRACKS_LINEAR:
            raise ValueError("X_init is required without TRACKS_LINEAR")
    else:
        x_init = f64(x_init)
        if x_init.shape != (4, n_pts):
            raise ValueError("X_init must be (4, n_pts) with n_pts = %d, got %s" % (n_pts, x_init.shape))
    return pt_ptr, cam_idx, uv, projs, x_init, mode, iters, group


def check_screen(n_cams, max_err2, cos_min_angle, min_obs, cam_scale, group=0):
    """Arguments of a ``BaProblem.screen`` / ``cull`` call, without a device: returns them converted or raises ValueError."""
    max_err2, cos_min_angle = float(max_err2), float(cos_min_angle)
    if not max_err2 >= 0.0:
        raise ValueError("max_err2 must be >= 0 (inf switches the test off), got %r" % max_err2)
    if not cos_min_angle >= -1.0:
        raise ValueError("cos_min_angle must be >= -1 (>= 1 switches the test off), got %r" % cos_min_angle)
    if int(min_obs) != min_obs or min_obs < 0:
        raise ValueError("min_obs must be an integer >= 0, got %r" % (min_obs,))
    group = _check_group(group)
    return max_err2, cos_min_angle, int(min_obs), _check_cam_scale(cam_scale, n_cams), group


def _check_robust(max_err2, max_hyp, iters, lam=None, cos_min_angle=None):
    """The options the robust operations share, refused in the order of the C entry points: returns
    ``(max_err2, cos_min_angle, max_hyp, lam, iters)`` converted or raises ValueError.  ``lam`` / ``cos_min_angle`` None:
    the operation has no such option."""
    max_err2 = float(max_err2)
    cos_min_angle = None if cos_min_angle is None else float(cos_min_angle)
    lam = None if lam is None else float(lam)
    if not max_err2 >= 0.0:
        raise ValueError("max_err2 must be >= 0, got %r" % max_err2)
    if cos_min_angle is not None and not cos_min_angle >= -1.0:
        raise ValueError("cos_min_angle must be >= -1 (>= 1 switches the gate off), got %r" % cos_min_angle)
    max_hyp = _count("max_hyp", max_hyp)
    if max_hyp > RANSAC_MAX_HYP:      # one bound and one default for all three (the C side's kHypMax, kHypDefault)
        raise ValueError("max_hyp must be in 1 .. %d (0 = %d), got %r" % (RANSAC_MAX_HYP, RANSAC_DEFAULT_HYP, max_hyp))
    if lam is not None and not lam >= 0.0:
        raise ValueError("lam must be >= 0, got %r" % lam)
    return max_err2, cos_min_angle, max_hyp, lam, _count("iters", iters)


def _check_offsets(name, ptr, m):
    """The offsets of the groups of a free-form call as int32 (groups + 1,): they start at 0, do not decrease and end at
    M = ``m``, or ValueError."""
    ptr = np.ascontiguousarray(ptr, dtype=np.int32).ravel()
    if ptr.shape[0] < 1 or ptr[0] != 0 or ptr[-1] != m or np.any(np.diff(ptr) < 0):
        raise ValueError("%s must start at 0, not decrease and end at M = %d" % (name, m))
    return ptr


def check_ransac(n_cams, max_err2, cos_min_angle=1.0, max_hyp=0, lam=0.5, iters=3, cam_scale=None, group=0):
    """Arguments of a ``tri_tracks_ransac`` / ``BaProblem.retriangulate`` call, without a device: returns
    ``(max_err2, cos_min_angle, max_hyp, lam, iters, cam_scale, group)`` converted or raises ValueError -- everything
    sfm_tri_tracks_ransac refuses."""
    options = _check_robust(max_err2, max_hyp, iters, lam, cos_min_angle)
    group = _check_group(group)
    return options + (_check_cam_scale(cam_scale, n_cams), group)


def check_resect(n_cams, max_err2, max_hyp=0, lam=0.5, iters=3, mask=None, cam_scale=None):
    """Arguments of a ``resect_ransac`` / ``BaProblem.resect`` call, without a device: returns
    ``(max_err2, max_hyp, lam, iters, mask, cam_scale)`` converted or raises ValueError -- everything sfm_resect_ransac
    refuses before it looks at the views."""
    max_err2, _, max_hyp, lam, iters = _check_robust(max_err2, max_hyp, iters, lam)
    return max_err2, max_hyp, lam, iters, _cam_mask(mask, n_cams), _check_cam_scale(cam_scale, n_cams)


def check_resect_views(view_ptr, uv, X):
    """The free form's arrays, without a device: ``(view_ptr int32 (V + 1,), uv (2, M), X (3, M))`` converted or ValueError --
    view_ptr must start at 0, not decrease and end at M."""
    uv, X = f64(uv), f64(X)
    if uv.ndim != 2 or uv.shape[0] != 2 or X.ndim != 2 or X.shape != (3, uv.shape[1]):
        raise ValueError("uv must be (2, M) and X (3, M), got %r and %r" % (uv.shape, X.shape))
    return _check_offsets("view_ptr", view_ptr, uv.shape[1]), uv, X


def check_twoview(max_err2, max_hyp=0, iters=2):
    """Options of a ``twoview_ransac`` call, without a device: returns ``(max_err2, max_hyp, iters)`` converted or raises
    ValueError -- everything sfm_twoview_ransac refuses before it looks at the sets."""
    max_err2, _, max_hyp, _, iters = _check_robust(max_err2, max_hyp, iters)
    return max_err2, max_hyp, iters


def check_twoview_sets(set_ptr, left, right):
    """The arrays of a ``twoview_ransac`` call, without a device: ``(set_ptr int32 (S + 1,), left (2, M), right (2, M))``
    converted or ValueError -- set_ptr must start at 0, not decrease and end at M."""
    left, right = f64(left), f64(right)
    if left.ndim != 2 or left.shape[0] != 2 or right.shape != left.shape:
        raise ValueError("left and right must both be (2, M), got %r and %r" % (left.shape, right.shape))
    return _check_offsets("set_ptr", set_ptr, left.shape[1]), left, right


def check_similarity(max_err2, max_hyp=0, iters=2, rigid=False):
    """Options of a ``similarity_ransac`` / ``BaProblem.align`` call, without a device: returns
    ``(max_err2, max_hyp, iters, flags)`` converted or raises ValueError -- everything sfm_similarity_ransac refuses before
    it looks at the sets."""
    max_err2, _, max_hyp, _, iters = _check_robust(max_err2, max_hyp, iters)
    return max_err2, max_hyp, iters, SIMILARITY_RIGID if rigid else 0


def check_similarity_sets(set_ptr, src, dst):
    """The arrays of a ``similarity_ransac`` call, without a device: ``(set_ptr int32 (S + 1,), src (3, M), dst (3, M))``
    converted or ValueError -- set_ptr must start at 0, not decrease and end at M."""
    src, dst = f64(src), f64(dst)
    if src.ndim != 2 or src.shape[0] != 3 or dst.shape != src.shape:
        raise ValueError("src and dst must both be (3, M), got %r and %r" % (src.shape, dst.shape))
    return _check_offsets("set_ptr", set_ptr, src.shape[1]), src, dst


def check_loss(kind, delta):
    """Arguments of a ``BaProblem.set_loss`` call, without a device: returns ``(kind, delta)`` converted or raises ValueError.
    ``kind`` is ``LOSS_NONE`` / ``LOSS_HUBER`` / ``LOSS_CAUCHY`` or its name; ``delta`` (normalised units) must be finite and
    > 0 unless the kind is ``LOSS_NONE``, which ignores it."""
    if isinstance(kind, str):
        if kind.lower() not in LOSS_NAMES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(LOSS_NAMES), kind))
        kind = LOSS_NAMES[kind.lower()]
    if isinstance(kind, bool) or int(kind) != kind or int(kind) not in (LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY):
        raise ValueError("loss kind must be LOSS_NONE, LOSS_HUBER or LOSS_CAUCHY, got %r" % (kind,))
    kind = int(kind)
    if kind == LOSS_NONE:
        return kind, 1.0
    delta = float(delta)
    if not (np.isfinite(delta) and delta > 0.0):
        raise ValueError("loss delta must be finite and > 0, got %r" % delta)
    return kind, delta


def check_pcg(n_cams, lam, iters, mask=None, tol=1e-10, max_cg=0, group=0):
    """Arguments of a ``BaProblem.iterate_pcg`` call, without a device: returns ``(lam, iters, mask, tol, max_cg, group)``
    converted (``mask`` as uint8 (n_cams,) or None) or raises ValueError -- the rules of sfm_ba_iterate_pcg."""
    lam, tol = float(lam), float(tol)
    if not (np.isfinite(lam) and lam >= 0.0):
        raise ValueError("lam must be finite and >= 0, got %r" % lam)
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError("iters must be an integer >= 0, got %r" % (iters,))
    if not (0.0 < tol < 1.0):
        raise ValueError("tol must lie in (0, 1), got %r" % tol)
    if isinstance(max_cg, bool) or int(max_cg) != max_cg or max_cg < 0:
        raise ValueError("max_cg must be an integer >= 0 (0: min(7 V_free, 1000)), got %r" % (max_cg,))
    return lam, int(iters), _cam_mask(mask, n_cams), tol, int(max_cg), _check_group(group)


def _count(name, value):
    try:
        ok = not isinstance(value, bool) and int(value) == value and value >= 0
    except (OverflowError, ValueError, TypeError):      # inf, nan, not a number
        ok = False
    if not ok:
        raise ValueError("%s must be an integer >= 0, got %r" % (name, value))
    return int(value)


def check_lm(n_cams, mask=None, **options):
    """Options of a ``BaProblem.minimize_pcg`` call, without a device: ``(LmOptions, mask)`` -- the defaults of
    sfm_lm_options_default (``LM_DEFAULTS``) overridden by the keywords, ``mask`` as uint8 (n_cams,) or None -- or
    ValueError for everything sfm_ba_minimize_pcg refuses."""
    unknown = sorted(set(options) - set(LM_DEFAULTS))
    if unknown:
        raise ValueError("unknown option(s) %s; the options are %s" % (unknown, sorted(LM_DEFAULTS)))
    o = dict(LM_DEFAULTS)
    o.update(options)
    lo, l0, hi = float(o["lambda_min"]), float(o["lambda0"]), float(o["lambda_max"])
    if not (np.isfinite(lo) and np.isfinite(l0) and np.isfinite(hi) and 0.0 < lo <= l0 <= hi):
        raise ValueError("0 < lambda_min <= lambda0 <= lambda_max, all finite, is required, got %r, %r, %r" % (lo, l0, hi))
    for name in ("ftol", "xtol", "gtol"):
        if not float(o[name]) >= 0.0:
            raise ValueError("%s must be >= 0 (0 switches the test off), got %r" % (name, o[name]))
    if not (0.0 < float(o["cg_tol"]) < 1.0):
        raise ValueError("cg_tol must lie in (0, 1), got %r" % (o["cg_tol"],))
    out = LmOptions(l0, lo, hi, float(o["ftol"]), float(o["xtol"]), float(o["gtol"]), float(o["cg_tol"]),
                    _count("cg_max_iters", o["cg_max_iters"]), _count("max_trials", o["max_trials"]), int(o["quirks"]),
                    _check_group(o["group"]))
    return out, _cam_mask(mask, n_cams)


def tri_tracks(pt_ptr, cam_idx, uv, projs, X_init=None, mode=TRACKS_NONLINEAR, lam=0.5, iters=100, group=0):
    """Triangulate / refine every point from its own track (sfm_tri_tracks): pt_ptr (n+1,), cam_idx (M,), uv (2, M),
    projs (V, 3, 4), X_init (4, n) or None with TRACKS_LINEAR -> (X (4, n), cost (2, n), status (n,) of TRACK_* bits)."""
    pt_ptr, cam_idx, uv, projs, x_init, mode, iters, group = check_tracks(pt_ptr, cam_idx, uv, projs, X_init, mode, iters, group)
    n_pts, n_obs = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    out = np.zeros((4, n_pts)); cost = np.zeros((2, n_pts)); status = np.zeros(n_pts, dtype=np.int32)
    check(load().sfm_tri_tracks(n_pts, projs.shape[0], n_obs, iptr(pt_ptr), iptr(cam_idx), dptr(uv), dptr(projs), mode,
                                float(lam), iters, group, dptr(x_init), dptr(out), dptr(cost), iptr(status)))
    return out, cost, status


def tracks_auto_group(n_pts, n_obs, max_track):
    """The lane-group width ``group=0`` selects for a call of these sizes (sfm_tri_tracks_auto_group; host only)."""
    return int(load().sfm_tri_tracks_auto_group(int(n_pts), int(n_obs), int(max_track)))


def tri_tracks_dev(n_pts, n_views, n_obs, d_pt_ptr, d_cam_idx, d_uv, d_projs, mode, lam, iters, group, d_x_init, d_x_out,
                   d_cost=0, d_status=0, stream=0):
    mode, iters, group = _tracks_mode_group(mode, iters, group)
    check(load().sfm_tri_tracks_dev(int(n_pts), int(n_views), int(n_obs), _vp(d_pt_ptr), _vp(d_cam_idx), _vp(d_uv), _vp(d_projs),
                                    mode, float(lam), iters, group, _vp(d_x_init), _vp(d_x_out), _vp(d_cost), _vp(d_status),
                                    _vp(stream)))


def tri_ransac_pair(n, max_hyp, h):
    """``(H, i, j)``: the hypothesis count of a track of ``n`` observations and the pair of hypothesis ``h``
    (sfm_tri_ransac_pair; host only).  ``i = j = -1`` when ``h`` is not in ``0 .. H - 1``."""
    i, j = ctypes.c_int(-1), ctypes.c_int(-1)
    count = int(load().sfm_tri_ransac_pair(int(n), int(max_hyp), int(h), ctypes.byref(i), ctypes.byref(j)))
    return count, int(i.value), int(j.value)


def _ransac_outputs(n, m):
    """The five output arrays of a robust triangulation of n points and m observations, as a namespace."""
    return SimpleNamespace(inlier=np.zeros(m, dtype=np.uint8), n_inliers=np.zeros(n, dtype=np.int32),
                           best_hyp=np.zeros(n, dtype=np.int32), status=np.zeros(n, dtype=np.int32),
                           summary=np.zeros(6, dtype=np.int64))


def _ransac_pointers(o):
    return _u8ptr(o.inlier), iptr(o.n_inliers), iptr(o.best_hyp), iptr(o.status), _lptr(o.summary)


def tri_tracks_ransac(pt_ptr, cam_idx, uv, projs, max_err2, cos_min_angle=1.0, max_hyp=0, lam=0.5, iters=3, cam_scale=None,
                      X_init=None, group=0):
    """Robust triangulation of every point from its own track (sfm_tri_tracks_ransac): pair hypotheses scored by their
    inlier count, then a refit over the winner's inliers.  Arrays as ``tri_tracks``; ``cam_scale`` (V,) multiplies a
    view's residuals (None: 1).  Returns ``X (4, n), inlier (M,) uint8, n_inliers (n,), best_hyp (n,), status (n,) of
    RANSAC_* bits, summary (6,) int64`` in the order of ``RANSAC_SUMMARY``."""
    pt_ptr, cam_idx, uv, projs, x_init, _mode, _iters, _group = check_tracks(
        pt_ptr, cam_idx, uv, projs, X_init, TRACKS_LINEAR | TRACKS_NONLINEAR, 0, 0)
    max_err2, cos_min_angle, max_hyp, lam, iters, cam_scale, group = check_ransac(projs.shape[0], max_err2, cos_min_angle, max_hyp,
                                                                                  lam, iters, cam_scale, group)
    n_pts, n_obs = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    out = np.zeros((4, n_pts))
    o = _ransac_outputs(n_pts, n_obs)
    check(load().sfm_tri_tracks_ransac(n_pts, projs.shape[0], n_obs, iptr(pt_ptr), iptr(cam_idx), dptr(uv), dptr(projs),
                                       dptr(cam_scale), max_err2, cos_min_angle, max_hyp, lam, iters, group, dptr(x_init),
                                       dptr(out), *_ransac_pointers(o)))
    return out, o.inlier, o.n_inliers, o.best_hyp, o.status, o.summary


def tri_tracks_ransac_dev(n_pts, n_views, n_obs, d_pt_ptr, d_cam_idx, d_uv, d_projs, max_err2, cos_min_angle=1.0, max_hyp=0,
                          lam=0.5, iters=3, group=0, d_cam_scale=0, d_x_init=0, d_x_out=0, d_inlier=0, d_n_inliers=0, d_best_hyp=0,
                          d_status=0, d_summary=0, stream=0):
    """``tri_tracks_ransac`` on device pointers and a caller's stream (sfm_tri_tracks_ransac_dev); ``d_x_out`` may equal
    ``d_x_init``, optional arrays are 0."""
    max_err2, cos_min_angle, max_hyp, lam, iters, _s, group = check_ransac(n_views, max_err2, cos_min_angle, max_hyp, lam, iters,
                                                                           None, group)
    check(load().sfm_tri_tracks_ransac_dev(int(n_pts), int(n_views), int(n_obs), _vp(d_pt_ptr), _vp(d_cam_idx), _vp(d_uv),
                                           _vp(d_projs), _vp(d_cam_scale), max_err2, cos_min_angle, max_hyp, lam, iters, group,
                                           _vp(d_x_init), _vp(d_x_out), _vp(d_inlier), _vp(d_n_inliers), _vp(d_best_hyp),
                                           _vp(d_status), _vp(d_summary), _vp(stream)))


def resect_triple(n, max_hyp, h):
    """``(H, i, j, l)``: the hypothesis count of a camera of ``n`` observations and the triple of hypothesis ``h``
    (sfm_resect_triple; host only).  ``i = j = l = -1`` when ``h`` is not in ``0 .. H - 1``."""
    i, j, l = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    count = int(load().sfm_resect_triple(int(n), int(max_hyp), int(h), ctypes.byref(i), ctypes.byref(j), ctypes.byref(l)))
    return count, int(i.value), int(j.value), int(l.value)


def resect_ransac(view_ptr, uv, X, max_err2, max_hyp=0, lam=0.5, iters=3, quirks=QUIRKS_REFERENCE, cam_scale=None, cams_init=None):
    """Robust resection of every view from its own observations (sfm_resect_ransac): three-point hypotheses scored by
    their inlier count, then a refit over the winner's inliers.  ``view_ptr`` (V + 1,) delimits the observations of a view
    in ``uv`` (2, M) normalised keys and ``X`` (3, M) their points; ``cam_scale`` (V,) multiplies a view's residuals (None:
    1); ``cams_init`` (V, 7) is what an unsolved view returns (None: the identity at the origin).  Returns ``cams (V, 7),
    inlier (M,) uint8, n_inliers (V,), best_hyp (V,), status (V,) of RESECT_* bits, summary (6,) int64`` in the order of
    ``RESECT_SUMMARY``."""
    view_ptr, uv, X = check_resect_views(view_ptr, uv, X)
    n_views, n_obs = view_ptr.shape[0] - 1, uv.shape[1]
    max_err2, max_hyp, lam, iters, _mask, cam_scale = check_resect(n_views, max_err2, max_hyp, lam, iters, None, cam_scale)
    if cams_init is not None:
        cams_init = f64(cams_init)
        if cams_init.shape != (n_views, 7):
            raise ValueError("cams_init must be (%d, 7), got %r" % (n_views, cams_init.shape))
    cams = np.zeros((n_views, 7))
    o = _ransac_outputs(n_views, n_obs)
    check(load().sfm_resect_ransac(n_views, iptr(view_ptr), n_obs, dptr(uv), dptr(X), dptr(cam_scale), max_err2, max_hyp, lam,
                                   iters, int(quirks), dptr(cams_init), dptr(cams), *_ransac_pointers(o)))
    return cams, o.inlier, o.n_inliers, o.best_hyp, o.status, o.summary


def resect_ransac_dev(view_ptr, n_obs, d_uv, d_X, max_err2, max_hyp=0, lam=0.5, iters=3, quirks=QUIRKS_REFERENCE, d_cam_scale=0,
                      d_cams_init=0, d_cams_out=0, d_inlier=0, d_n_inliers=0, d_best_hyp=0, d_status=0, d_summary=0, stream=0):
    """``resect_ransac`` on device pointers and a caller's stream (sfm_resect_ransac_dev); ``view_ptr`` stays a host array,
    ``d_cams_out`` may equal ``d_cams_init``, optional arrays are 0."""
    view_ptr = np.ascontiguousarray(view_ptr, dtype=np.int32).ravel()
    max_err2, max_hyp, lam, iters, _mask, _s = check_resect(view_ptr.shape[0] - 1, max_err2, max_hyp, lam, iters)
    check(load().sfm_resect_ransac_dev(view_ptr.shape[0] - 1, iptr(view_ptr), int(n_obs), _vp(d_uv), _vp(d_X), _vp(d_cam_scale),
                                       max_err2, max_hyp, lam, iters, int(quirks), _vp(d_cams_init), _vp(d_cams_out), _vp(d_inlier),
                                       _vp(d_n_inliers), _vp(d_best_hyp), _vp(d_status), _vp(d_summary), _vp(stream)))


def twoview_sample(n, max_hyp, h):
    """``(H, idx)``: the hypothesis count of a set of ``n`` matches and the eight ascending match indices of hypothesis
    ``h`` (sfm_twoview_sample; host only).  ``idx`` is eight times -1 when ``h`` is not in ``0 .. H - 1``."""
    idx = np.full(8, -1, dtype=np.int32)
    count = int(load().sfm_twoview_sample(int(n), int(max_hyp), int(h), iptr(idx)))
    return count, tuple(int(i) for i in idx)


def twoview_ransac(set_ptr, left, right, max_err2, max_hyp=0, iters=2, outputs=TWOVIEW_OUTPUTS):
    """Robust fundamental matrix of every set of matches (sfm_twoview_ransac): stratified eight-point hypotheses scored by
    their inlier count under the squared Sampson distance ``max_err2`` (pixels squared), then up to ``iters`` refits over
    the inliers.  ``set_ptr`` (S + 1,) delimits the matches of a set in ``left`` / ``right`` (2, M) pixel coordinates.
    Returns ``F (S, 3, 3)`` of Frobenius norm 1 (zeros without a model), ``inlier (M,) uint8, n_inliers (S,), best_hyp
    (S,), status (S,) of TWOVIEW_* bits, summary (6,) int64`` in the order of ``TWOVIEW_SUMMARY``; an output not named in
    ``outputs`` is not computed and comes back as None."""
    set_ptr, left, right = check_twoview_sets(set_ptr, left, right)
    max_err2, max_hyp, iters = check_twoview(max_err2, max_hyp, iters)
    unknown = set(outputs) - set(TWOVIEW_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (TWOVIEW_OUTPUTS, sorted(unknown)))
    n_sets, n_obs = set_ptr.shape[0] - 1, left.shape[1]
    F = np.zeros((n_sets, 3, 3))
    o = _ransac_outputs(n_sets, n_obs)
    ptrs = [p if name in outputs else None for name, p in zip(TWOVIEW_OUTPUTS, _ransac_pointers(o))]
    check(load().sfm_twoview_ransac(n_sets, iptr(set_ptr), n_obs, dptr(left), dptr(right), max_err2, max_hyp, iters, dptr(F), *ptrs))
    return (F,) + tuple(getattr(o, name) if name in outputs else None for name in TWOVIEW_OUTPUTS)


def twoview_ransac_dev(set_ptr, n_obs, d_left, d_right, max_err2, max_hyp=0, iters=2, d_F_out=0, d_inlier=0, d_n_inliers=0,
                       d_best_hyp=0, d_status=0, d_summary=0, stream=0):
    """``twoview_ransac`` on device pointers and a caller's stream (sfm_twoview_ransac_dev); ``set_ptr`` stays a host array,
    optional arrays are 0."""
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int32).ravel()
    max_err2, max_hyp, iters = check_twoview(max_err2, max_hyp, iters)
    check(load().sfm_twoview_ransac_dev(set_ptr.shape[0] - 1, iptr(set_ptr), int(n_obs), _vp(d_left), _vp(d_right), max_err2,
                                        max_hyp, iters, _vp(d_F_out), _vp(d_inlier), _vp(d_n_inliers), _vp(d_best_hyp),
                                        _vp(d_status), _vp(d_summary), _vp(stream)))


def homography_sample(n, max_hyp, h):
    """``(H, idx)``: the hypothesis count of a set of ``n`` matches and the four ascending match indices of hypothesis
    ``h`` (sfm_homography_sample; host only).  ``idx`` is four times -1 when ``h`` is not in ``0 .. H - 1``."""
    idx = np.full(4, -1, dtype=np.int32)
    count = int(load().sfm_homography_sample(int(n), int(max_hyp), int(h), iptr(idx)))
    return count, tuple(int(i) for i in idx)


def homography_ransac(set_ptr, left, right, max_err2, max_hyp=0, iters=2, outputs=HOMOGRAPHY_OUTPUTS):
    """Robust homography of every set of matches (sfm_homography_ransac): stratified four-point hypotheses scored by their
    inlier count under a transfer error of ``max_err2`` (pixels squared) in both images, then up to ``iters`` refits over
    the inliers.  The arrays and options are those of ``twoview_ransac`` (``check_twoview_sets``, ``check_twoview``).
    Returns ``H (S, 3, 3)`` of Frobenius norm 1, mapping left to right (zeros without a model), ``inlier (M,) uint8,
    n_inliers (S,), best_hyp (S,), status (S,) of HOMOGRAPHY_* bits, summary (6,) int64`` in the order of
    ``HOMOGRAPHY_SUMMARY``; an output not named in ``outputs`` is not computed and comes back as None."""
    set_ptr, left, right = check_twoview_sets(set_ptr, left, right)
    max_err2, max_hyp, iters = check_twoview(max_err2, max_hyp, iters)
    unknown = set(outputs) - set(HOMOGRAPHY_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (HOMOGRAPHY_OUTPUTS, sorted(unknown)))
    n_sets, n_obs = set_ptr.shape[0] - 1, left.shape[1]
    H = np.zeros((n_sets, 3, 3))
    o = _ransac_outputs(n_sets, n_obs)
    ptrs = [p if name in outputs else None for name, p in zip(HOMOGRAPHY_OUTPUTS, _ransac_pointers(o))]
    check(load().sfm_homography_ransac(n_sets, iptr(set_ptr), n_obs, dptr(left), dptr(right), max_err2, max_hyp, iters, dptr(H), *ptrs))
    return (H,) + tuple(getattr(o, name) if name in outputs else None for name in HOMOGRAPHY_OUTPUTS)


def homography_ransac_dev(set_ptr, n_obs, d_left, d_right, max_err2, max_hyp=0, iters=2, d_H_out=0, d_inlier=0, d_n_inliers=0,
                          d_best_hyp=0, d_status=0, d_summary=0, stream=0):
    """``homography_ransac`` on device pointers and a caller's stream (sfm_homography_ransac_dev); ``set_ptr`` stays a host
    array, optional arrays are 0."""
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int32).ravel()
    max_err2, max_hyp, iters = check_twoview(max_err2, max_hyp, iters)
    check(load().sfm_homography_ransac_dev(set_ptr.shape[0] - 1, iptr(set_ptr), int(n_obs), _vp(d_left), _vp(d_right), max_err2,
                                           max_hyp, iters, _vp(d_H_out), _vp(d_inlier), _vp(d_n_inliers), _vp(d_best_hyp),
                                           _vp(d_status), _vp(d_summary), _vp(stream)))


# ---- robust similarity between two 3D frames (sfm_similarity_*; no reference counterpart) -------------------------------
def similarity_sample(n, max_hyp, h):
    """``(H, idx)``: the hypothesis count of a set of ``n`` correspondences and the three ascending indices of hypothesis
    ``h`` (sfm_similarity_sample; host only).  ``idx`` is three times -1 when ``h`` is not in ``0 .. H - 1``."""
    idx = np.full(3, -1, dtype=np.int32)
    count = int(load().sfm_similarity_sample(int(n), int(max_hyp), int(h), iptr(idx)))
    return count, tuple(int(i) for i in idx)


def similarity_ransac(set_ptr, src, dst, max_err2, max_hyp=0, iters=2, rigid=False, outputs=SIMILARITY_OUTPUTS):
    """Robust similarity ``dst ~ s A src + t`` of every set of 3D-3D correspondences (sfm_similarity_ransac): stratified
    three-point hypotheses scored by their inlier count under a squared distance of ``max_err2`` in the ``dst`` frame, then
    up to ``iters`` refits over the inliers; ``rigid`` holds ``s = 1``.  ``set_ptr`` (S + 1,) delimits the correspondences of
    a set in ``src`` / ``dst`` (3, M).  Returns ``sim (S, 13)`` -- s, A row-major, t; zeros without a model -- and ``inlier
    (M,) uint8, n_inliers (S,), best_hyp (S,), status (S,) of SIMILARITY_* bits, summary (6,) int64`` in the order of
    ``SIMILARITY_SUMMARY``; an output not named in ``outputs`` is not computed and comes back as None."""
    set_ptr, src, dst = check_similarity_sets(set_ptr, src, dst)
    max_err2, max_hyp, iters, flags = check_similarity(max_err2, max_hyp, iters, rigid)
    unknown = set(outputs) - set(SIMILARITY_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (SIMILARITY_OUTPUTS, sorted(unknown)))
    n_sets, n_obs = set_ptr.shape[0] - 1, src.shape[1]
    sim = np.zeros((n_sets, 13))
    o = _ransac_outputs(n_sets, n_obs)
    ptrs = [p if name in outputs else None for name, p in zip(SIMILARITY_OUTPUTS, _ransac_pointers(o))]
    check(load().sfm_similarity_ransac(n_sets, iptr(set_ptr), n_obs, dptr(src), dptr(dst), max_err2, max_hyp, iters, flags,
                                       dptr(sim), *ptrs))
    return (sim,) + tuple(getattr(o, name) if name in outputs else None for name in SIMILARITY_OUTPUTS)


def similarity_ransac_dev(set_ptr, n_obs, d_src, d_dst, max_err2, max_hyp=0, iters=2, rigid=False, d_sim_out=0, d_inlier=0,
                          d_n_inliers=0, d_best_hyp=0, d_status=0, d_summary=0, stream=0):
    """``similarity_ransac`` on device pointers and a caller's stream (sfm_similarity_ransac_dev); ``set_ptr`` stays a host
    array, optional arrays are 0."""
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int32).ravel()
    max_err2, max_hyp, iters, flags = check_similarity(max_err2, max_hyp, iters, rigid)
    check(load().sfm_similarity_ransac_dev(set_ptr.shape[0] - 1, iptr(set_ptr), int(n_obs), _vp(d_src), _vp(d_dst), max_err2,
                                           max_hyp, iters, flags, _vp(d_sim_out), _vp(d_inlier), _vp(d_n_inliers),
                                           _vp(d_best_hyp), _vp(d_status), _vp(d_summary), _vp(stream)))


def split_similarity(sim):
    """``(s, A (3, 3), t (3,))`` of one model of 13 doubles."""
    sim = f64(sim).reshape(13)
    return float(sim[0]), sim[1:10].reshape(3, 3).copy(), sim[10:13].copy()


# ---- what the view-graph operations share: their argument checks and their optional outputs ------------------------------
def _integer(name, value):
    if isinstance(value, (bool, np.bool_)) or int(value) != value:
        raise ValueError("%s must be an integer, got %r" % (name, value))
    return int(value)


def _graph_edges(edges):
    """``edges`` as it came, an array: ValueError unless it holds integers in the shape (E, 2)."""
    edges_in = np.asarray(edges)
    if edges_in.ndim != 2 or edges_in.shape[1] != 2 or (edges_in.size and not np.all(edges_in == np.floor(edges_in))):
        raise ValueError("edges must be integers of shape (E, 2), got %r" % (edges_in.shape,))
    return edges_in


def _refuse_bad_edges(edges_in, n_views):
    """ValueError naming the first edge that does not join two different views in 0 .. n_views - 1."""
    bad = (edges_in < 0) | (edges_in >= n_views)
    bad = bad[:, 0] | bad[:, 1] | (edges_in[:, 0] == edges_in[:, 1])
    if bad.any():
        e = int(np.argmax(bad))
        raise ValueError("edge %d = (%d, %d) must join two different views in 0 .. %d" % (e, edges_in[e, 0], edges_in[e, 1], n_views - 1))


def _refuse_bad_rotations(R, what, skip_zero=False):
    """The ValueError of the library's verify_rotation naming the first row of ``R (n, 9)`` that fails it (``what`` is a format
    for its index); with ``skip_zero`` nine zeros stand for "no rotation" and pass."""
    bad = ~_verify_rotations(R)
    if skip_zero:
        bad &= np.any(R != 0.0, axis=1)
    if bad.any():
        raise ValueError("convert_quaternion_to_rotation : Invalid output rotation matrix (%s is not a rotation)"
                         % (what % int(np.argmax(bad))))


def _cos_or_degrees(cos, deg):
    """``cos`` if given, else the cosine of ``deg`` degrees."""
    return float(np.cos(np.deg2rad(float(deg)))) if cos is None else cos


def _optional_outputs(outputs, known, arrays, scalars=()):
    """``(wanted, result)`` of a call with optional output arrays: ``wanted[name]`` is ``arrays[name]`` where ``outputs`` names it
    and None otherwise -- ValueError for a name that is not in ``known``; ``result()``, after the call, is the tuple in the
    order of ``known``, the one-element arrays named in ``scalars`` as ints."""
    unknown = set(outputs) - set(known)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (known, sorted(unknown)))
    wanted = {k: (v if k in outputs else None) for k, v in arrays.items()}

    def result():
        return tuple(None if wanted[k] is None else (int(wanted[k][0]) if k in scalars else wanted[k]) for k in known)
    return wanted, result


# ---- rotation averaging over a view graph (sfm_rotation_*; no reference counterpart) ------------------------------------
def check_rotation_graph(n_views, edges, rel, root=0, cos_max=1.0, max_hyp=0, iters=2, steps=2, cg_tol=1e-12, cg_max=200):
    """The arguments of a ``rotation_average`` call, without a device: ``(n_views, edges int32 (E, 2), rel (E, 9), root,
    cos_max, max_hyp, iters, steps, cg_tol, cg_max)`` converted or ValueError -- everything sfm_rotation_average refuses, in
    its order; a ``Rel`` that is no rotation raises the ValueError of the library's verify_rotation and names the edge."""
    n_views, root = _integer("n_views", n_views), _integer("root", root)
    max_hyp, iters, steps, cg_max = _integer("max_hyp", max_hyp), _integer("iters", iters), _integer("steps", steps), _integer("cg_max", cg_max)
    cos_max, cg_tol = float(cos_max), float(cg_tol)
    edges_in = _graph_edges(edges)
    rel = f64(rel)
    n_edges = edges_in.shape[0]
    if rel.size != 9 * n_edges or rel.ndim not in (2, 3):
        raise ValueError("rel must be (E, 9) or (E, 3, 3) with E = %d, got %r" % (n_edges, rel.shape))
    rel = rel.reshape(n_edges, 9)
    if n_views < 2 or n_edges < 1 or n_edges >= 2 ** 30:
        raise ValueError("bad sizes V=%d E=%d (V >= 2, 1 <= E < 2^30)" % (n_views, n_edges))
    if not 0 <= root < n_views:
        raise ValueError("root = %d must be in 0 .. %d" % (root, n_views - 1))
    if not (0.0 < cos_max <= 1.0):
        raise ValueError("cos_max = %r must be in (0, 1]" % cos_max)
    if not 0 <= max_hyp <= ROTAVG_MAX_HYP:
        raise ValueError("max_hyp = %d must be in 1 .. %d (0 = %d)" % (max_hyp, ROTAVG_MAX_HYP, ROTAVG_DEFAULT_HYP))
    if iters < 0:
        raise ValueError("iters = %d must be >= 0" % iters)
    if steps < 1:
        raise ValueError("steps = %d must be >= 1" % steps)
    if not (0.0 < cg_tol < 1.0):
        raise ValueError("cg_tol = %r must be in (0, 1)" % cg_tol)
    if cg_max < 1:
        raise ValueError("cg_max = %d must be >= 1" % cg_max)
    _refuse_bad_edges(edges_in, n_views)
    edges = np.ascontiguousarray(edges_in, dtype=np.int32)
    _refuse_bad_rotations(rel, "Rel of edge %d")
    return n_views, edges, rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max


def _verify_rotations(R):
    """The library's verify_rotation (csrc/sfm_math.h) on rows of nine: False iff det - 1 >= 1e-8 or an entry of the inverse by
    adjugate exceeds the transpose's by more than 1e-8; a NaN passes, as it does there."""
    with np.errstate(all="ignore"):
        m = [R[:, k] for k in range(9)]
        det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
        inv_det = 1.0 / det
        inv = [(m[4] * m[8] - m[5] * m[7]), (m[2] * m[7] - m[1] * m[8]), (m[1] * m[5] - m[2] * m[4]),
               (m[5] * m[6] - m[3] * m[8]), (m[0] * m[8] - m[2] * m[6]), (m[2] * m[3] - m[0] * m[5]),
               (m[3] * m[7] - m[4] * m[6]), (m[1] * m[6] - m[0] * m[7]), (m[0] * m[4] - m[1] * m[3])]
        ok = ~(det - 1 >= 1e-8)
        for i in range(3):
            for j in range(3):
                ok &= ~(inv[3 * i + j] * inv_det - m[3 * j + i] > 1e-8)
    return ok


def rotation_edge_test(R_i, R_j, rel, cos_max):
    """``(inlier, lhs)`` of one edge against the rotations of its ends (sfm_rotation_edge_test; host only): ``lhs`` is the trace
    of ``R_j^T Rel R_i`` in the library's operation order, an inlier iff it is finite and ``>= fma(2, cos_max, 1)``."""
    R_i, R_j, rel = f64(R_i).reshape(9), f64(R_j).reshape(9), f64(rel).reshape(9)
    lhs = np.zeros(1)
    inlier = load().sfm_rotation_edge_test(dptr(R_i), dptr(R_j), dptr(rel), float(cos_max), dptr(lhs))
    return bool(inlier), float(lhs[0])


def rotation_tree(n_views, edges, root, max_hyp, h):
    """``(H, parent_edge (V,), depth (V,))``: the breadth-first spanning tree of hypothesis ``h`` of a view graph
    (sfm_rotation_tree; host only); -1 marks the tree's root (parent) and views it does not reach (both).  ``H`` is 0 for
    arguments the library refuses."""
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    parent = np.full(max(int(n_views), 1), -1, dtype=np.int32)
    depth = np.full(max(int(n_views), 1), -1, dtype=np.int32)
    count = int(load().sfm_rotation_tree(int(n_views), edges.shape[0], iptr(edges), int(root), int(max_hyp), int(h), iptr(parent), iptr(depth)))
    return count, parent, depth


def rotation_plan(n_views, max_hyp=0, cap_bytes=0):
    """``(batch, n_batches)`` of the hypotheses of a call for ``n_views`` views when the rotations of a batch stay within
    ``cap_bytes`` (sfm_rotation_plan; host only).  The cap also holds for the calls that follow -- a hook for tests; 0
    restores the library's 256 MiB."""
    batch, n_batches = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    check(load().sfm_rotation_plan(int(n_views), int(max_hyp), int(cap_bytes), iptr(batch), iptr(n_batches)))
    return int(batch[0]), int(n_batches[0])


def rotation_average(n_views, edges, rel, root=0, cos_max=None, max_hyp=0, iters=2, steps=2, cg_tol=1e-12, cg_max=200,
                     max_angle_deg=5.0, outputs=ROTAVG_OUTPUTS):
    """Robust absolute rotations of a view graph (sfm_rotation_average): edge ``e = (i, j)`` with ``rel[e]`` says
    ``R_j = rel[e] R_i``; spanning-tree hypotheses scored by their inlier count under a residual angle whose cosine is at
    least ``cos_max`` (default: that of ``max_angle_deg``), then up to ``iters`` rounds of ``steps`` Gauss-Newton steps over
    the inliers.  Returns ``R (V, 3, 3)`` -- zeros outside the root's component or without a model -- and ``edge_inlier (E,)
    uint8, edge_cos (E,), view_status (V,) of ROTAVG_UNREACHED / ROTAVG_HELD bits, n_inliers, best_hyp, status of ROTAVG_*
    bits, summary (6,) int64`` in the order of ``ROTAVG_SUMMARY``; an output not named in ``outputs`` is not computed and
    comes back as None."""
    cos_max = _cos_or_degrees(cos_max, max_angle_deg)
    V, edges, rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max = check_rotation_graph(
        n_views, edges, rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max)
    E = edges.shape[0]
    R = np.zeros((V, 9))
    w, result = _optional_outputs(outputs, ROTAVG_OUTPUTS, {
        "edge_inlier": np.zeros(E, dtype=np.uint8), "edge_cos": np.zeros(E), "view_status": np.zeros(V, dtype=np.int32),
        "n_inliers": np.zeros(1, dtype=np.int32), "best_hyp": np.zeros(1, dtype=np.int32), "status": np.zeros(1, dtype=np.int32),
        "summary": np.zeros(6, dtype=np.int64)}, scalars=("n_inliers", "best_hyp", "status"))
    check(load().sfm_rotation_average(V, E, iptr(edges), dptr(rel), root, cos_max, max_hyp, iters, steps, cg_tol, cg_max, dptr(R),
                                      _u8ptr(w["edge_inlier"]), dptr(w["edge_cos"]), iptr(w["view_status"]), iptr(w["n_inliers"]),
                                      iptr(w["best_hyp"]), iptr(w["status"]), _lptr(w["summary"])))
    return (R.reshape(V, 3, 3),) + result()


def rotation_average_dev(n_views, edges, d_rel, root=0, cos_max=None, max_hyp=0, iters=2, steps=2, cg_tol=1e-12, cg_max=200,
                         max_angle_deg=5.0, d_R_out=0, d_edge_inlier=0, d_edge_cos=0, d_view_status=0, d_n_inliers=0, d_best_hyp=0,
                         d_status=0, d_summary=0, stream=0):
    """``rotation_average`` with ``d_rel`` (E, 9) and the outputs as device pointers and a caller's stream
    (sfm_rotation_average_dev); ``edges`` stays a host array, optional arrays are 0."""
    cos_max = _cos_or_degrees(cos_max, max_angle_deg)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    check(load().sfm_rotation_average_dev(int(n_views), edges.shape[0], iptr(edges), _vp(d_rel), int(root), float(cos_max), int(max_hyp),
                                          int(iters), int(steps), float(cg_tol), int(cg_max), _vp(d_R_out), _vp(d_edge_inlier),
                                          _vp(d_edge_cos), _vp(d_view_status), _vp(d_n_inliers), _vp(d_best_hyp), _vp(d_status),
                                          _vp(d_summary), _vp(stream)))


# ---- view triplets: the cycle-consistency filter of a view graph (sfm_view_triplet*; no reference counterpart) ----------
def check_view_triplets(n_views, edges, rel, edge_mask=None, cos_loop=1.0, min_ok=1, min_pct=0, keep_untested=0, group=0):
    """The arguments of a ``view_triplets`` call, without a device: ``(n_views, edges int32 (E, 2), rel (E, 9), edge_mask uint8
    (E,) or None, cos_loop, min_ok, min_pct, keep_untested, group)`` converted or ValueError -- everything sfm_view_triplets
    refuses, in its order; a ``Rel`` that is no rotation raises the ValueError of the library's verify_rotation and names the
    edge."""
    n_views, min_ok, min_pct, group = _integer("n_views", n_views), _integer("min_ok", min_ok), _integer("min_pct", min_pct), _integer("group", group)
    keep_untested = int(keep_untested) if isinstance(keep_untested, (bool, np.bool_)) else _integer("keep_untested", keep_untested)
    cos_loop = float(cos_loop)
    edges_in = _graph_edges(edges)
    rel = f64(rel)
    n_edges = edges_in.shape[0]
    if rel.size != 9 * n_edges or rel.ndim not in (2, 3):
        raise ValueError("rel must be (E, 9) or (E, 3, 3) with E = %d, got %r" % (n_edges, rel.shape))
    rel = rel.reshape(n_edges, 9)
    if edge_mask is not None:
        edge_mask = np.ascontiguousarray(np.asarray(edge_mask).reshape(-1) != 0, dtype=np.uint8)
        if edge_mask.shape[0] != n_edges:
            raise ValueError("edge_mask must have E = %d entries, got %d" % (n_edges, edge_mask.shape[0]))
    if n_views < 3 or n_edges < 1 or n_edges >= 2 ** 30:
        raise ValueError("bad sizes V=%d E=%d (V >= 3, 1 <= E < 2^30)" % (n_views, n_edges))
    if not (0.0 < cos_loop <= 1.0):
        raise ValueError("cos_loop = %r must be in (0, 1]" % cos_loop)
    if min_ok < 0:
        raise ValueError("min_ok = %d must be >= 1 (0 = 1)" % min_ok)
    if not 0 <= min_pct <= 100:
        raise ValueError("min_pct = %d must be in 0 .. 100" % min_pct)
    if keep_untested not in (0, 1):
        raise ValueError("keep_untested = %d must be 0 or 1" % keep_untested)
    if group not in (0, 1, 4, 8, 16, 32, 64):
        raise ValueError("group %d is not one of 0, 1, 4, 8, 16, 32, 64" % group)
    _refuse_bad_edges(edges_in, n_views)
    edges = np.ascontiguousarray(edges_in, dtype=np.int32)
    _refuse_bad_rotations(rel, "Rel of edge %d")
    return n_views, edges, rel, edge_mask, cos_loop, min_ok, min_pct, keep_untested, group


def view_triplet_test(M_ab, M_bc, M_ac, cos_loop):
    """``(consistent, lhs)`` of one triplet of oriented edges over views ``a < b < c`` (sfm_view_triplet_test; host only):
    ``lhs`` is the trace of ``M_ac^T M_bc M_ab`` in the library's operation order, consistent iff it is finite and
    ``>= fma(2, cos_loop, 1)``."""
    M_ab, M_bc, M_ac = f64(M_ab).reshape(9), f64(M_bc).reshape(9), f64(M_ac).reshape(9)
    lhs = np.zeros(1)
    ok = load().sfm_view_triplet_test(dptr(M_ab), dptr(M_bc), dptr(M_ac), float(cos_loop), dptr(lhs))
    return bool(ok), float(lhs[0])


def view_triplets(n_views, edges, rel, edge_mask=None, cos_loop=None, min_ok=1, min_pct=0, keep_untested=0, group=0, max_loop_deg=5.0,
                  outputs=TRIPLET_OUTPUTS):
    """The triplet filter of a view graph (sfm_view_triplets): around every triangle the three relative rotations must
    compose to the identity within a loop angle whose cosine is at least ``cos_loop`` (default: that of ``max_loop_deg``).
    An edge is kept iff at least ``min_ok`` and ``min_pct`` per cent of its triplets are consistent; an edge in no triplet
    gets ``keep_untested``.  Returns ``edge_keep (E,) uint8, n_tri (E,) int64, n_ok (E,) int64, kept_idx (n_kept,) int32,
    summary (8,) int64`` in the order of ``TRIPLET_SUMMARY``; an output not named in ``outputs`` is not fetched and comes back
    as None."""
    cos_loop = _cos_or_degrees(cos_loop, max_loop_deg)
    V, edges, rel, edge_mask, cos_loop, min_ok, min_pct, keep_untested, group = check_view_triplets(
        n_views, edges, rel, edge_mask, cos_loop, min_ok, min_pct, keep_untested, group)
    E = edges.shape[0]
    w, result = _optional_outputs(outputs, TRIPLET_OUTPUTS, {
        "edge_keep": np.zeros(E, dtype=np.uint8), "n_tri": np.zeros(E, dtype=np.int64), "n_ok": np.zeros(E, dtype=np.int64),
        "kept_idx": np.full(E, -1, dtype=np.int32), "summary": np.zeros(8, dtype=np.int64)})
    n_kept = np.zeros(1, dtype=np.int32)
    check(load().sfm_view_triplets(V, E, iptr(edges), dptr(rel), _u8ptr(edge_mask), cos_loop, min_ok, min_pct, keep_untested, group,
                                   _u8ptr(w["edge_keep"]), _lptr(w["n_tri"]), _lptr(w["n_ok"]), iptr(w["kept_idx"]),
                                   _lptr(w["summary"]), iptr(n_kept)))
    if w["kept_idx"] is not None:
        w["kept_idx"] = w["kept_idx"][:int(n_kept[0])].copy()
    return result()


def view_triplets_dev(n_views, edges, d_rel, d_edge_mask=0, cos_loop=None, min_ok=1, min_pct=0, keep_untested=0, group=0,
                      max_loop_deg=5.0, d_edge_keep=0, d_n_tri=0, d_n_ok=0, d_kept_idx=0, d_summary=0, stream=0):
    """``view_triplets`` with ``d_rel`` (E, 9), ``d_edge_mask`` and the outputs as device pointers and a caller's stream
    (sfm_view_triplets_dev); ``edges`` stays a host array, optional arrays are 0.  Returns ``n_kept``."""
    cos_loop = _cos_or_degrees(cos_loop, max_loop_deg)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    n_kept = np.zeros(1, dtype=np.int32)
    check(load().sfm_view_triplets_dev(int(n_views), edges.shape[0], iptr(edges), _vp(d_rel), _vp(d_edge_mask), float(cos_loop), int(min_ok),
                                       int(min_pct), int(keep_untested), int(group), _vp(d_edge_keep), _vp(d_n_tri), _vp(d_n_ok),
                                       _vp(d_kept_idx), _vp(d_summary), iptr(n_kept), _vp(stream)))
    return int(n_kept[0])


# ---- translation averaging over a view graph (sfm_translation_*; no reference counterpart) ------------------------------
def check_translation_graph(n_views, edges, R, t, edge_mask=None, root=0, cos_max=1.0, mu=0.01, rounds=8, polish=1, cg_tol=1e-13,
                            cg_max=500):
    """The arguments of a ``translation_average`` call, without a device: ``(n_views, edges int32 (E, 2), R (V, 9), t (E, 3),
    edge_mask uint8 (E,) or None, root, cos_max, mu, rounds, polish, cg_tol, cg_max)`` converted or ValueError -- everything
    sfm_translation_average refuses, in its order; a non-zero ``R_v`` that is no rotation raises the ValueError of the
    library's verify_rotation and names the view."""
    n_views, root = _integer("n_views", n_views), _integer("root", root)
    rounds, polish, cg_max = _integer("rounds", rounds), _integer("polish", int(polish) if isinstance(polish, (bool, np.bool_)) else polish), _integer("cg_max", cg_max)
    cos_max, mu, cg_tol = float(cos_max), float(mu), float(cg_tol)
    edges_in = _graph_edges(edges)
    n_edges = edges_in.shape[0]
    R, t = f64(R), f64(t)
    if R.size != 9 * max(n_views, 0) or R.ndim not in (2, 3):
        raise ValueError("R must be (V, 9) or (V, 3, 3) with V = %d, got %r" % (n_views, R.shape))
    if t.size != 3 * n_edges or t.ndim not in (2, 3):
        raise ValueError("t must be (E, 3) or (E, 3, 1) with E = %d, got %r" % (n_edges, t.shape))
    R, t = R.reshape(-1, 9), t.reshape(n_edges, 3)
    if edge_mask is not None:
        edge_mask = np.ascontiguousarray(np.asarray(edge_mask).reshape(-1) != 0, dtype=np.uint8)
        if edge_mask.size != n_edges:
            raise ValueError("edge_mask must hold E = %d entries, got %d" % (n_edges, edge_mask.size))
    if n_views < 2 or n_edges < 1 or n_edges >= 2 ** 30:
        raise ValueError("bad sizes V=%d E=%d (V >= 2, 1 <= E < 2^30)" % (n_views, n_edges))
    if not 0 <= root < n_views:
        raise ValueError("root = %d must be in 0 .. %d" % (root, n_views - 1))
    if not (0.0 < cos_max <= 1.0):
        raise ValueError("cos_max = %r must be in (0, 1]" % cos_max)
    if not (0.0 <= mu <= 1.0):
        raise ValueError("mu = %r must be in (0, 1] (0 = 0.01)" % mu)
    if rounds < 0:
        raise ValueError("rounds = %d must be >= 0" % rounds)
    if polish not in (0, 1):
        raise ValueError("polish = %d must be 0 or 1" % polish)
    if not (0.0 < cg_tol < 1.0):
        raise ValueError("cg_tol = %r must be in (0, 1)" % cg_tol)
    if cg_max < 1:
        raise ValueError("cg_max = %d must be >= 1" % cg_max)
    _refuse_bad_edges(edges_in, n_views)
    edges = np.ascontiguousarray(edges_in, dtype=np.int32)
    _refuse_bad_rotations(R, "R of view %d", skip_zero=True)
    return n_views, edges, R, t, edge_mask, root, cos_max, mu, rounds, polish, cg_tol, cg_max


def translation_edge_test(d, c_i, c_j, cos_max):
    """``(inlier, dv, n2)`` of one edge with the world direction ``d`` against the positions of its ends
    (sfm_translation_edge_test; host only): ``dv = d . (c_j - c_i)``, ``n2 = |c_j - c_i|^2`` in the library's operation order,
    an inlier iff both are finite, ``dv > 0`` and ``dv * dv >= cos_max^2 * n2``."""
    d, c_i, c_j = f64(d).reshape(3), f64(c_i).reshape(3), f64(c_j).reshape(3)
    dv, n2 = np.zeros(1), np.zeros(1)
    inlier = load().sfm_translation_edge_test(dptr(d), dptr(c_i), dptr(c_j), float(cos_max), dptr(dv), dptr(n2))
    return bool(inlier), float(dv[0]), float(n2[0])


def translation_average(n_views, edges, R, t, edge_mask=None, root=0, cos_max=None, mu=0.01, rounds=8, polish=1, cg_tol=1e-13,
                        cg_max=500, max_angle_deg=5.0, outputs=TRANSAVG_OUTPUTS):
    """Robust positions of the views of a graph whose rotations are known (sfm_translation_average): edge ``e = (i, j)`` with
    ``t[e]`` the translation of the pair's pose ``X_j = Rel X_i + t``, ``R (V, 3, 3)`` the absolute rotations (zeros: none),
    ``edge_mask`` optional (0 excludes an edge).  A reweighted linear estimator: ``rounds`` Cauchy rounds after the first
    solve, an optional polish over the inliers; an edge is an inlier while the angle between its direction and ``c_j - c_i``
    has a cosine of at least ``cos_max`` (default: that of ``max_angle_deg``).  Returns ``C (V, 3)`` -- zeros for a view
    without a position -- and ``edge_inlier (E,) uint8, edge_cos (E,), edge_len (E,), view_status (V,) of TRANSAVG_NO_ROTATION /
    UNREACHED / HELD bits, n_inliers, status of TRANSAVG_* bits, summary (6,) int64`` in the order of ``TRANSAVG_SUMMARY``,
    ``log (rounds + 2, 4)``; an output not named in ``outputs`` is not computed and comes back as None."""
    cos_max = _cos_or_degrees(cos_max, max_angle_deg)
    V, edges, R, t, edge_mask, root, cos_max, mu, rounds, polish, cg_tol, cg_max = check_translation_graph(
        n_views, edges, R, t, edge_mask, root, cos_max, mu, rounds, polish, cg_tol, cg_max)
    E = edges.shape[0]
    C = np.zeros((V, 3))
    w, result = _optional_outputs(outputs, TRANSAVG_OUTPUTS, {
        "edge_inlier": np.zeros(E, dtype=np.uint8), "edge_cos": np.zeros(E), "edge_len": np.zeros(E),
        "view_status": np.zeros(V, dtype=np.int32), "n_inliers": np.zeros(1, dtype=np.int32), "status": np.zeros(1, dtype=np.int32),
        "summary": np.zeros(6, dtype=np.int64), "log": np.zeros((rounds + 2, 4))}, scalars=("n_inliers", "status"))
    check(load().sfm_translation_average(V, E, iptr(edges), dptr(R), dptr(t), _u8ptr(edge_mask), root, cos_max, mu, rounds, polish, cg_tol,
                                         cg_max, dptr(C), _u8ptr(w["edge_inlier"]), dptr(w["edge_cos"]), dptr(w["edge_len"]),
                                         iptr(w["view_status"]), iptr(w["n_inliers"]), iptr(w["status"]), _lptr(w["summary"]), dptr(w["log"])))
    return (C,) + result()


def translation_average_dev(n_views, edges, d_R, d_t, d_edge_mask=0, root=0, cos_max=None, mu=0.01, rounds=8, polish=1, cg_tol=1e-13,
                            cg_max=500, max_angle_deg=5.0, d_C_out=0, d_edge_inlier=0, d_edge_cos=0, d_edge_len=0, d_view_status=0,
                            d_n_inliers=0, d_status=0, d_summary=0, d_log=0, stream=0):
    """``translation_average`` with ``d_R`` (V, 9), ``d_t`` (E, 3), ``d_edge_mask`` (E,) bytes and the outputs as device pointers
    and a caller's stream (sfm_translation_average_dev); ``edges`` stays a host array, optional arrays are 0."""
    cos_max = _cos_or_degrees(cos_max, max_angle_deg)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    check(load().sfm_translation_average_dev(int(n_views), edges.shape[0], iptr(edges), _vp(d_R), _vp(d_t), _vp(d_edge_mask), int(root),
                                             float(cos_max), float(mu), int(rounds), int(polish), float(cg_tol), int(cg_max), _vp(d_C_out),
                                             _vp(d_edge_inlier), _vp(d_edge_cos), _vp(d_edge_len), _vp(d_view_status), _vp(d_n_inliers),
                                             _vp(d_status), _vp(d_summary), _vp(d_log), _vp(stream)))


# ---- track linking: multi-view tracks from verified pairwise matches (sfm_link_tracks*; no reference counterpart) ---------
def check_track_link(key_ptr, pair_views, pair_ptr, a, b, mask=None, min_len=2, group=0, scan=0):
    """The arguments of a ``track_link`` call, without a device: ``(key_ptr int32 (V + 1,), pair_views int32 (P, 2), pair_ptr
    int64 (P + 1,), a int32 (M,), b int32 (M,), mask uint8 (M,) or None, min_len, group, scan)`` converted or ValueError --
    everything sfm_link_tracks refuses, in its order, naming the item."""
    def integer(name, value):
        if isinstance(value, bool) or int(value) != value:
            raise ValueError("%s must be an integer, got %r" % (name, value))
        return int(value)

    def integers(name, value, dtype, shape):
        arr = np.asarray(value)
        if arr.size and not np.all(arr == np.floor(arr)):
            raise ValueError("%s must hold integers" % name)
        arr = arr.reshape(shape)
        if arr.size and (arr.min() < np.iinfo(dtype).min or arr.max() > np.iinfo(dtype).max):
            raise ValueError("%s does not fit %s" % (name, np.dtype(dtype).name))
        return np.ascontiguousarray(arr, dtype=dtype)
    min_len, group, scan = integer("min_len", min_len), integer("group", group), integer("scan", scan)
    key_ptr = integers("key_ptr", key_ptr, np.int64, (-1,))
    pair_views = integers("pair_views", pair_views, np.int64, (-1, 2))
    pair_ptr = integers("pair_ptr", pair_ptr, np.int64, (-1,))
    if key_ptr.size < 1 or pair_ptr.size != pair_views.shape[0] + 1:
        raise ValueError("key_ptr must hold V + 1 >= 1 entries and pair_ptr P + 1 = %d, got %d and %d"
                         % (pair_views.shape[0] + 1, key_ptr.size, pair_ptr.size))
    V, P = key_ptr.size - 1, pair_views.shape[0]
    if min_len < 2:
        raise ValueError("min_len = %d must be >= 2" % min_len)
    _check_group(group)
    if scan not in (0, 1, 2):
        raise ValueError("scan = %d must be 0 (automatic), 1 (one workgroup) or 2 (device-wide)" % scan)
    if key_ptr[0] != 0:
        raise ValueError("key_ptr[0] = %d must be 0" % key_ptr[0])
    down = np.diff(key_ptr) < 0
    if down.any():
        raise ValueError("key_ptr decreases at view %d" % int(np.argmax(down)))
    if key_ptr[-1] >= 2 ** 31:
        raise ValueError("K = %d must be below 2^31" % key_ptr[-1])
    if pair_ptr[0] != 0:
        raise ValueError("pair_ptr[0] = %d must be 0" % pair_ptr[0])
    for p in range(P):
        i, j = int(pair_views[p, 0]), int(pair_views[p, 1])
        if not (0 <= i < V and 0 <= j < V) or i == j:
            raise ValueError("pair %d = (%d, %d) must join two different views in 0 .. %d" % (p, i, j, V - 1))
        if pair_ptr[p + 1] < pair_ptr[p]:
            raise ValueError("pair_ptr decreases at pair %d" % p)
    M = int(pair_ptr[-1])
    a, b = integers("a", a, np.int64, (-1,)), integers("b", b, np.int64, (-1,))
    if a.size != M or b.size != M:
        raise ValueError("a and b must hold M = pair_ptr[P] = %d matches, got %d and %d" % (M, a.size, b.size))
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if mask.size != M:
            raise ValueError("mask must hold M = %d entries, got %d" % (M, mask.size))
    if M:
        n_keys = np.diff(key_ptr)
        pair_of = np.repeat(np.arange(P), np.diff(pair_ptr))
        bad = (a < 0) | (a >= n_keys[pair_views[pair_of, 0]]) | (b < 0) | (b >= n_keys[pair_views[pair_of, 1]])
        if bad.any():
            raise ValueError("match %d names a key outside its view" % int(np.argmax(bad)))
    return (key_ptr.astype(np.int32), np.ascontiguousarray(pair_views, dtype=np.int32), pair_ptr, a.astype(np.int32), b.astype(np.int32),
            mask, min_len, group, scan)


def track_link_plan(n_views, n_keys, n_matches, group=0, scan=0):
    """The launch plan of a ``track_link`` call as a dict over ``LINK_PLAN`` (sfm_link_tracks_plan; host only; the grids
    follow ``set_cu_limit``)."""
    plan = np.zeros(8, dtype=np.int32)
    check(load().sfm_link_tracks_plan(int(n_views), int(n_keys), int(n_matches), int(group), int(scan), iptr(plan)))
    return dict(zip(LINK_PLAN, (int(v) for v in plan)))


def track_link(key_ptr, pair_views, pair_ptr, a, b, mask=None, min_len=2, group=0, scan=0, outputs=LINK_OUTPUTS):
    """Multi-view tracks from pairwise matches (sfm_link_tracks): the connected components of the used matches over (view,
    key) nodes; a component with two keys of one view is dropped as a conflict, one below ``min_len`` as short.  Global key
    ``key_ptr[v] + k``; the matches of pair ``p = (i, j)`` are ``a[m]`` (keys of ``i``) and ``b[m]`` (keys of ``j``) for
    ``pair_ptr[p] <= m < pair_ptr[p + 1]``.  Returns a dict: ``key_track (K,)`` (track, or LINK_UNMATCHED / LINK_SHORT /
    LINK_CONFLICT), ``pt_ptr (n_tracks + 1,)``, ``cam_idx``, ``key_idx (n_obs,)`` by ascending view inside a track, ``summary
    (8,) int64`` in the order of ``LINK_SUMMARY``, ``label (K,)`` the smallest global key of every key's component; an output
    not named in ``outputs`` is not computed and comes back as None."""
    key_ptr, pair_views, pair_ptr, a, b, mask, min_len, group, scan = check_track_link(key_ptr, pair_views, pair_ptr, a, b, mask, min_len,
                                                                                       group, scan)
    unknown = set(outputs) - set(LINK_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (LINK_OUTPUTS, sorted(unknown)))
    V, P, K = key_ptr.size - 1, pair_views.shape[0], int(key_ptr[-1])
    summary = np.zeros(8, dtype=np.int64)              # always: it holds the two counts that size the CSR
    o = {"key_track": np.zeros(K, dtype=np.int32), "pt_ptr": np.zeros(K // 2 + 2, dtype=np.int32), "cam_idx": np.zeros(K, dtype=np.int32),
         "key_idx": np.zeros(K, dtype=np.int32), "label": np.zeros(K, dtype=np.int32)}
    w = {k: (v if k in outputs else None) for k, v in o.items()}
    check(load().sfm_link_tracks(V, iptr(key_ptr), P, iptr(pair_views), _lptr(pair_ptr), iptr(a), iptr(b), _u8ptr(mask), min_len, group, scan,
                                iptr(w["key_track"]), iptr(w["pt_ptr"]), iptr(w["cam_idx"]), iptr(w["key_idx"]), _lptr(summary),
                                iptr(w["label"])))
    n_tracks, n_obs = int(summary[2]), int(summary[5])
    for name, n in (("pt_ptr", n_tracks + 1), ("cam_idx", n_obs), ("key_idx", n_obs)):
        if w[name] is not None:
            w[name] = w[name][:n].copy()
    w["summary"] = summary if "summary" in outputs else None
    return w


def track_link_dev(key_ptr, pair_views, pair_ptr, d_a, d_b, d_mask=0, min_len=2, group=0, scan=0, d_key_track=0, d_pt_ptr=0, d_cam_idx=0,
                   d_key_idx=0, d_summary=0, d_label=0, stream=0):
    """``track_link`` with ``a``, ``b``, ``mask`` and the outputs as device pointers (``d_pt_ptr`` holds K / 2 + 2 entries,
    ``d_cam_idx`` and ``d_key_idx`` K) and a caller's stream (sfm_link_tracks_dev); ``key_ptr``, ``pair_views`` and ``pair_ptr``
    stay host arrays, optional arrays are 0.  Returns ``(n_tracks, n_obs)``."""
    key_ptr, pair_ptr = i32(key_ptr).reshape(-1), np.ascontiguousarray(pair_ptr, dtype=np.int64).reshape(-1)
    pair_views = i32(pair_views).reshape(-1, 2)
    n_tracks, n_obs = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    check(load().sfm_link_tracks_dev(key_ptr.size - 1, iptr(key_ptr), pair_views.shape[0], iptr(pair_views), _lptr(pair_ptr), _vp(d_a), _vp(d_b),
                                    _vp(d_mask), int(min_len), int(group), int(scan), _vp(d_key_track), _vp(d_pt_ptr), _vp(d_cam_idx),
                                    _vp(d_key_idx), _vp(d_summary), _vp(d_label), iptr(n_tracks), _lptr(n_obs), _vp(stream)))
    return int(n_tracks[0]), int(n_obs[0])


# ---- robust essential matrix (sfm_essential_*; no reference counterpart) ------------------------------------------------
def _check_intrinsics(K_left, K_right):
    out = []
    for name, K in (("K_left", K_left), ("K_right", K_right)):
        K = f64(K)
        if K.shape != (3, 3) or not np.all(np.isfinite(K)) or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
            raise ValueError("%s must be a finite upper triangular (3, 3) matrix with K[2][2] = 1" % name)
        out.append(K.reshape(9).copy())
    return out[0], out[1]


def check_essential(set_ptr, left, right, K_left, K_right, max_err2, max_hyp=0):
    """The arguments of an ``essential_ransac`` call, without a device: ``(set_ptr int32 (S + 1,), left (2, M), right (2, M),
    K_left (9,), K_right (9,), max_err2, max_hyp)`` converted or ValueError -- everything sfm_essential_ransac refuses."""
    max_err2, _, max_hyp, _, _ = _check_robust(max_err2, max_hyp, 0)
    K_left, K_right = _check_intrinsics(K_left, K_right)
    set_ptr, left, right = check_twoview_sets(set_ptr, left, right)
    return set_ptr, left, right, K_left, K_right, max_err2, max_hyp


def essential_sample(n, max_hyp, h):
    """``(H, idx)``: the hypothesis count of a set of ``n`` matches and the five ascending match indices of hypothesis
    ``h`` (sfm_essential_sample; host only).  ``idx`` is five times -1 when ``h`` is not in ``0 .. H - 1``."""
    idx = np.full(5, -1, dtype=np.int32)
    count = int(load().sfm_essential_sample(int(n), int(max_hyp), int(h), iptr(idx)))
    return count, tuple(int(i) for i in idx)


def essential_solve(a, b):
    """The essential matrices of five matches with the rays ``(a[k, 0], a[k, 1], 1)`` and ``(b[k, 0], b[k, 1], 1)``, b^T E a = 0
    (sfm_essential_solve: the solver the hypothesis kernel runs, on the host): ``E (n, 3, 3)``, n <= 10, each of Frobenius
    norm 1 with its entry of largest magnitude positive, by ascending ``E[0, 0]``."""
    a, b = f64(a), f64(b)
    if a.shape != (5, 2) or b.shape != (5, 2):
        raise ValueError("a and b must both be (5, 2), got %r and %r" % (a.shape, b.shape))
    E = np.zeros((ESSENTIAL_MAX_SOLUTIONS, 3, 3))
    n = np.zeros(1, dtype=np.int32)
    check(load().sfm_essential_solve(dptr(a), dptr(b), dptr(E), iptr(n)))
    return E[:int(n[0])].copy()


def essential_ransac(set_ptr, left, right, K_left, K_right, max_err2, max_hyp=0, outputs=ESSENTIAL_OUTPUTS):
    """Robust essential matrix of every set of matches (sfm_essential_ransac; the rule is in include/sfm_hip.h, 'robust
    essential matrix'): stratified five-point hypotheses, up to ten solutions each, scored by their inlier count under the
    squared Sampson distance ``max_err2`` (pixels squared); no refit.  ``set_ptr``, ``left``, ``right`` as in
    ``twoview_ransac``, the intrinsics as in ``twoview_pose``.  Returns a dict: ``E (S, 3, 3)`` canonical (zeros without a
    model) and, of ``ESSENTIAL_OUTPUTS``, what ``outputs`` names (None otherwise): ``F (S, 3, 3)`` in pixels with the norm and
    sign of ``twoview_ransac``'s, ``inlier (M,) uint8, n_inliers (S,), best_hyp (S,), best_root (S,), n_valid (S,), status
    (S,) of ESSENTIAL_* bits, summary (6,) int64`` in the order of ``ESSENTIAL_SUMMARY``."""
    set_ptr, left, right, K_left, K_right, max_err2, max_hyp = check_essential(set_ptr, left, right, K_left, K_right, max_err2, max_hyp)
    unknown = set(outputs) - set(ESSENTIAL_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (ESSENTIAL_OUTPUTS, sorted(unknown)))
    n_sets, n_obs = set_ptr.shape[0] - 1, left.shape[1]
    o = {"E": np.zeros((n_sets, 3, 3)), "F": np.zeros((n_sets, 3, 3)), "inlier": np.zeros(n_obs, dtype=np.uint8),
         "n_inliers": np.zeros(n_sets, dtype=np.int32), "best_hyp": np.zeros(n_sets, dtype=np.int32),
         "best_root": np.zeros(n_sets, dtype=np.int32), "n_valid": np.zeros(n_sets, dtype=np.int32),
         "status": np.zeros(n_sets, dtype=np.int32), "summary": np.zeros(6, dtype=np.int64)}
    cast = {"F": dptr, "inlier": _u8ptr, "summary": _lptr}
    ptrs = [cast.get(name, iptr)(o[name]) if name in outputs else None for name in ESSENTIAL_OUTPUTS]
    check(load().sfm_essential_ransac(n_sets, iptr(set_ptr), n_obs, dptr(left), dptr(right), dptr(K_left), dptr(K_right), max_err2,
                                      max_hyp, dptr(o["E"]), *ptrs))
    return {name: (o[name] if name == "E" or name in outputs else None) for name in o}


def essential_ransac_dev(set_ptr, n_obs, d_left, d_right, K_left, K_right, max_err2, max_hyp=0, d_E_out=0, d_F_out=0, d_inlier=0,
                         d_n_inliers=0, d_best_hyp=0, d_best_root=0, d_n_valid=0, d_status=0, d_summary=0, stream=0):
    """``essential_ransac`` on device pointers and a caller's stream (sfm_essential_ransac_dev); ``set_ptr`` and the
    intrinsics stay host arrays, optional arrays are 0."""
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int32).ravel()
    max_err2, _, max_hyp, _, _ = _check_robust(max_err2, max_hyp, 0)
    K_left, K_right = _check_intrinsics(K_left, K_right)
    check(load().sfm_essential_ransac_dev(set_ptr.shape[0] - 1, iptr(set_ptr), int(n_obs), _vp(d_left), _vp(d_right), dptr(K_left),
                                          dptr(K_right), max_err2, max_hyp, _vp(d_E_out), _vp(d_F_out), _vp(d_inlier),
                                          _vp(d_n_inliers), _vp(d_best_hyp), _vp(d_best_root), _vp(d_n_valid), _vp(d_status),
                                          _vp(d_summary), _vp(stream)))


# ---- relative pose of a verified pair (sfm_twoview_pose*; no reference counterpart) ------------------------------------
def check_pose(n_sets, models, kinds, K_left, K_right, cos2_min, min_parallax):
    """The arguments of a ``twoview_pose`` call besides the matches, without a device: ``(model (n_sets, 9) float64, kind
    (n_sets,) int32, K_left (9,), K_right (9,), cos2_min, min_parallax)`` converted or ValueError -- everything
    sfm_twoview_pose refuses.  ``kinds`` holds POSE_FROM_F / POSE_FROM_H or the names of ``POSE_KINDS``."""
    cos2_min = float(cos2_min)
    if not 0.0 <= cos2_min <= 1.0:
        raise ValueError("cos2_min must be in [0, 1], got %r" % cos2_min)
    min_parallax = _count("min_parallax", min_parallax)
    kind = np.zeros(n_sets, dtype=np.int32)
    kinds = list(kinds) if not isinstance(kinds, np.ndarray) else kinds.tolist()
    if len(kinds) != n_sets:
        raise ValueError("relative pose: %d sets, %d kinds" % (n_sets, len(kinds)))
    for s, k in enumerate(kinds):
        k = POSE_KINDS.get(k, k) if isinstance(k, str) else k
        if k not in (POSE_FROM_F, POSE_FROM_H):
            raise ValueError("relative pose: set %d has the unknown kind %r" % (s, kinds[s]))
        kind[s] = k
    model = f64(models).reshape(-1, 9) if n_sets else np.zeros((0, 9))
    if model.shape[0] != n_sets:
        raise ValueError("relative pose: %d sets, %d models" % (n_sets, model.shape[0]))
    out = []
    for name, K in (("K_left", K_left), ("K_right", K_right)):
        K = f64(K)
        if K.shape != (3, 3) or not np.all(np.isfinite(K)) or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
            raise ValueError("%s must be a finite upper triangular (3, 3) matrix with K[2][2] = 1" % name)
        out.append(K.reshape(9).copy())
    return model, kind, out[0], out[1], cos2_min, min_parallax


def twoview_pose_test(R, t, a, b, cos2_min):
    """``(front, parallax)`` of one match with the rays ``(a[0], a[1], 1)`` and ``(b[0], b[1], 1)`` against the pose
    ``(R, t)`` (sfm_twoview_pose_test: the function the kernels call, on the host)."""
    R, t, a, b = f64(R).reshape(9), f64(t).reshape(3), f64(a).reshape(2), f64(b).reshape(2)
    front, par = ci(0), ci(0)
    check(load().sfm_twoview_pose_test(dptr(R), dptr(t), dptr(a), dptr(b), float(cos2_min), ctypes.byref(front), ctypes.byref(par)))
    return int(front.value), int(par.value)


def twoview_pose(set_ptr, left, right, models, kinds, K_left, K_right, cos2_min, min_parallax=1, mask=None, outputs=POSE_OUTPUTS):
    """Relative pose of every set of matches from its verified model (sfm_twoview_pose; the rule is in include/sfm_hip.h,
    'relative pose of a verified pair'): four candidates from F or H, an integer cheirality vote over the matches ``mask``
    (M,) selects (None: all), the parallax count of the winner.  ``set_ptr``, ``left``, ``right`` as in ``twoview_ransac``;
    ``cos2_min`` is the squared cosine of the minimum triangulation angle.  Returns a dict: ``R (S, 3, 3)`` and ``t (S, 3)``
    with X_right = R X_left + t (zeros without a winner) and, of ``POSE_OUTPUTS``, what ``outputs`` names (None
    otherwise): ``normal (S, 3), cand_front (S, 4), n_front (S,), n_parallax (S,), best_cand (S,), status (S,) of POSE_*
    bits, obs_front (M,) uint8 (1 in front, 2 with parallax), X (3, M), summary (6,) int64`` in the order of
    ``POSE_SUMMARY``."""
    set_ptr, left, right = check_twoview_sets(set_ptr, left, right)
    n_sets, m = set_ptr.shape[0] - 1, left.shape[1]
    model, kind, kl, kr, cos2_min, min_parallax = check_pose(n_sets, models, kinds, K_left, K_right, cos2_min, min_parallax)
    unknown = set(outputs) - set(POSE_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (POSE_OUTPUTS, sorted(unknown)))
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        if mask.shape[0] != m:
            raise ValueError("mask must have one entry per match (%d), got %d" % (m, mask.shape[0]))
    o = {"R": np.zeros((n_sets, 3, 3)), "t": np.zeros((n_sets, 3))}
    shapes = {"normal": ((n_sets, 3), np.float64), "cand_front": ((n_sets, 4), np.int32), "n_front": (n_sets, np.int32),
              "n_parallax": (n_sets, np.int32), "best_cand": (n_sets, np.int32), "status": (n_sets, np.int32),
              "obs_front": (m, np.uint8), "X": ((3, m), np.float64), "summary": (6, np.int64)}
    for name in POSE_OUTPUTS:
        o[name] = np.zeros(shapes[name][0], dtype=shapes[name][1]) if name in outputs else None
    check(load().sfm_twoview_pose(n_sets, iptr(set_ptr), m, dptr(left), dptr(right), _u8ptr(mask), dptr(model), iptr(kind), dptr(kl),
                                  dptr(kr), cos2_min, min_parallax, dptr(o["R"]), dptr(o["t"]), dptr(o["normal"]),
                                  iptr(o["cand_front"]), iptr(o["n_front"]), iptr(o["n_parallax"]), iptr(o["best_cand"]),
                                  iptr(o["status"]), _u8ptr(o["obs_front"]), dptr(o["X"]), _lptr(o["summary"])))
    return o


def twoview_pose_dev(set_ptr, n_obs, d_left, d_right, models, kinds, K_left, K_right, cos2_min, min_parallax=1, d_mask=0, d_R_out=0,
                     d_t_out=0, d_normal=0, d_cand_front=0, d_n_front=0, d_n_parallax=0, d_best_cand=0, d_status=0, d_obs_front=0,
                     d_X_out=0, d_summary=0, stream=0):
    """``twoview_pose`` on device pointers and a caller's stream (sfm_twoview_pose_dev); ``set_ptr``, the models, kinds and
    intrinsics stay host arrays, optional arrays are 0."""
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int32).ravel()
    n_sets = max(set_ptr.shape[0] - 1, 0)
    model, kind, kl, kr, cos2_min, min_parallax = check_pose(n_sets, models, kinds, K_left, K_right, cos2_min, min_parallax)
    check(load().sfm_twoview_pose_dev(set_ptr.shape[0] - 1, iptr(set_ptr), int(n_obs), _vp(d_left), _vp(d_right), _vp(d_mask),
                                      dptr(model), iptr(kind), dptr(kl), dptr(kr), cos2_min, min_parallax, _vp(d_R_out), _vp(d_t_out),
                                      _vp(d_normal), _vp(d_cand_front), _vp(d_n_front), _vp(d_n_parallax), _vp(d_best_cand),
                                      _vp(d_status), _vp(d_obs_front), _vp(d_X_out), _vp(d_summary), _vp(stream)))


# ---- refinement of a relative pose (sfm_twoview_refine*; no reference counterpart) ------------------------------------------
def check_refine(n_sets, R_in, t_in, K_left, K_right, lam, iters, max_err2, cos2_min):
    """The arguments of a ``twoview_refine`` call besides the matches, without a device: ``(R (n_sets, 9), t (n_sets, 3), K_left
    (9,), K_right (9,), lam, iters, max_err2, cos2_min)`` converted or ValueError -- everything sfm_twoview_refine refuses."""
    lam, max_err2, cos2_min = float(lam), float(max_err2), float(cos2_min)
    if not lam >= 0.0:
        raise ValueError("lam must be >= 0, got %r" % lam)
    iters = _count("iters", iters)
    if not max_err2 >= 0.0:
        raise ValueError("max_err2 must be >= 0, got %r" % max_err2)
    if not 0.0 <= cos2_min <= 1.0:
        raise ValueError("cos2_min must be in [0, 1], got %r" % cos2_min)
    R = f64(R_in).reshape(-1, 9) if n_sets else np.zeros((0, 9))
    t = f64(t_in).reshape(-1, 3) if n_sets else np.zeros((0, 3))
    if R.shape[0] != n_sets or t.shape[0] != n_sets:
        raise ValueError("pose refinement: %d sets, %d rotations, %d translations" % (n_sets, R.shape[0], t.shape[0]))
    out = []
    for name, K in (("K_left", K_left), ("K_right", K_right)):
        K = f64(K)
        if K.shape != (3, 3) or not np.all(np.isfinite(K)) or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
            raise ValueError("%s must be a finite upper triangular (3, 3) matrix with K[2][2] = 1" % name)
        out.append(K.reshape(9).copy())
    return np.ascontiguousarray(R), np.ascontiguousarray(t), out[0], out[1], lam, iters, max_err2, cos2_min


def twoview_refine_test(R, t, K_left, K_right, xl, yl, xr, yr):
    """``(r, J (5,))``: the signed Sampson distance in pixels of one match at the pose ``(R, t)`` as given and its Jacobian row in
    the chart of the pose (sfm_twoview_refine_test: the functions the kernels call, on the host)."""
    R, t, kl, kr = f64(R).reshape(9), f64(t).reshape(3), f64(K_left).reshape(9), f64(K_right).reshape(9)
    r, J = ctypes.c_double(0.0), np.zeros(5)
    check(load().sfm_twoview_refine_test(dptr(R), dptr(t), dptr(kl), dptr(kr), float(xl), float(yl), float(xr), float(yr), ctypes.byref(r),
                                         dptr(J)))
    return float(r.value), J


def info_matrix(info):
    """The (5, 5) matrix U = sum J^T J of the packed upper triangle ``info`` (15,) a refinement returns."""
    U = np.zeros((5, 5))
    U[np.triu_indices(5)] = np.asarray(info, dtype=np.float64).reshape(15)
    return U + np.triu(U, 1).T


def twoview_refine(set_ptr, left, right, R_in, t_in, K_left, K_right, lam=0.0, iters=6, max_err2=4.0, cos2_min=1.0, mask=None,
                   outputs=REFINE_OUTPUTS):
    """Refine the relative pose of every set of matches by damped Gauss-Newton on the Sampson distance in pixels and judge the
    matches against the result (sfm_twoview_refine; the rule is in include/sfm_hip.h, 'refinement of a relative pose').
    ``set_ptr``, ``left``, ``right``, ``mask`` as in ``twoview_pose``; ``R_in (S, 3, 3)``, ``t_in (S, 3)`` with
    X_right = R X_left + t.  Returns a dict: ``R (S, 3, 3)``, ``t (S, 3)`` and, of ``REFINE_OUTPUTS``, what ``outputs`` names
    (None otherwise): ``F (S, 3, 3)`` of Frobenius norm 1, ``cost (2, S)`` before and after, ``info (S, 15)`` (see
    ``info_matrix``), ``n_used (S,)``, ``status (S,)`` of REFINE_* bits, ``obs_res (M,)`` the signed Sampson distance,
    ``obs_inlier (M,)``, ``obs_front (M,)`` uint8, ``X (3, M)``, ``n_inliers``, ``n_front``, ``n_parallax (S,)`` over the
    selected matches, ``summary (6,)`` int64 in the order of ``REFINE_SUMMARY``."""
    set_ptr, left, right = check_twoview_sets(set_ptr, left, right)
    n_sets, m = set_ptr.shape[0] - 1, left.shape[1]
    R, t, kl, kr, lam, iters, max_err2, cos2_min = check_refine(n_sets, R_in, t_in, K_left, K_right, lam, iters, max_err2, cos2_min)
    unknown = set(outputs) - set(REFINE_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (REFINE_OUTPUTS, sorted(unknown)))
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        if mask.shape[0] != m:
            raise ValueError("mask must have one entry per match (%d), got %d" % (m, mask.shape[0]))
    o = {"R": np.zeros((n_sets, 3, 3)), "t": np.zeros((n_sets, 3))}
    shapes = {"F": ((n_sets, 3, 3), np.float64), "cost": ((2, n_sets), np.float64), "info": ((n_sets, 15), np.float64),
              "n_used": (n_sets, np.int32), "status": (n_sets, np.int32), "obs_res": (m, np.float64), "obs_inlier": (m, np.uint8),
              "obs_front": (m, np.uint8), "X": ((3, m), np.float64), "n_inliers": (n_sets, np.int32), "n_front": (n_sets, np.int32),
              "n_parallax": (n_sets, np.int32), "summary": (6, np.int64)}
    for name in REFINE_OUTPUTS:
        o[name] = np.zeros(shapes[name][0], dtype=shapes[name][1]) if name in outputs else None
    check(load().sfm_twoview_refine(n_sets, iptr(set_ptr), m, dptr(left), dptr(right), _u8ptr(mask), dptr(R), dptr(t), dptr(kl), dptr(kr),
                                    lam, iters, max_err2, cos2_min, dptr(o["R"]), dptr(o["t"]), dptr(o["F"]), dptr(o["cost"]),
                                    dptr(o["info"]), iptr(o["n_used"]), iptr(o["status"]), dptr(o["obs_res"]), _u8ptr(o["obs_inlier"]),
                                    _u8ptr(o["obs_front"]), dptr(o["X"]), iptr(o["n_inliers"]), iptr(o["n_front"]),
                                    iptr(o["n_parallax"]), _lptr(o["summary"])))
    return o


def twoview_refine_dev(set_ptr, n_obs, d_left, d_right, d_R_in, d_t_in, K_left, K_right, lam=0.0, iters=6, max_err2=4.0, cos2_min=1.0,
                       d_mask=0, d_R_out=0, d_t_out=0, d_F_out=0, d_cost=0, d_info=0, d_n_used=0, d_status=0, d_obs_res=0, d_obs_inlier=0,
                       d_obs_front=0, d_X_out=0, d_n_inliers=0, d_n_front=0, d_n_parallax=0, d_summary=0, stream=0):
    """``twoview_refine`` on device pointers and a caller's stream (sfm_twoview_refine_dev); ``set_ptr`` and the intrinsics stay
    host arrays, optional arrays are 0."""
    set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int32).ravel()
    _R, _t, kl, kr, lam, iters, max_err2, cos2_min = check_refine(0, None, None, K_left, K_right, lam, iters, max_err2, cos2_min)
    check(load().sfm_twoview_refine_dev(set_ptr.shape[0] - 1, iptr(set_ptr), int(n_obs), _vp(d_left), _vp(d_right), _vp(d_mask),
                                        _vp(d_R_in), _vp(d_t_in), dptr(kl), dptr(kr), lam, iters, max_err2, cos2_min, _vp(d_R_out),
                                        _vp(d_t_out), _vp(d_F_out), _vp(d_cost), _vp(d_info), _vp(d_n_used), _vp(d_status),
                                        _vp(d_obs_res), _vp(d_obs_inlier), _vp(d_obs_front), _vp(d_X_out), _vp(d_n_inliers),
                                        _vp(d_n_front), _vp(d_n_parallax), _vp(d_summary), _vp(stream)))


def pnp_nonlinear(uv_pix, pts_h, intrinsic, rot0, loc0, lam, iters, quirks=QUIRKS_REFERENCE):
    uv_pix = f64(uv_pix); pts_h = f64(pts_h); intrinsic = f64(intrinsic); rot0 = f64(rot0); loc0 = f64(loc0).reshape(3)
    n = uv_pix.shape[1]
    rot = np.empty((3, 3)); loc = np.empty(3)
    check(load().sfm_pnp_nonlinear(n, dptr(uv_pix), dptr(pts_h), dptr(intrinsic), dptr(rot0), dptr(loc0),
                                   float(lam), int(iters), int(quirks), dptr(rot), dptr(loc)))
    return rot, loc.reshape(3, 1)


def pnp_linear_ransac(uv_pix, pts_h, intrinsic, samples, threshold, as_array=False):
    """Evaluate six-point DLT hypotheses (samples: (n_hyp, 6) indices drawn by the caller) and return
    (rot (3,3), loc (3,1), inlier index list (or int array with ``as_array``), best hypothesis index or -1)."""
    uv_pix = f64(uv_pix); pts_h = f64(pts_h); intrinsic = f64(intrinsic)
    samples = i32(samples).reshape(-1, 6)
    n, n_hyp = uv_pix.shape[1], samples.shape[0]
    rot = np.empty((3, 3)); loc = np.empty(3)
    mask = np.empty(n, dtype=np.int32)
    cnt = ctypes.c_int(); best = ctypes.c_int()
    check(load().sfm_pnp_linear_ransac(n, dptr(uv_pix), dptr(pts_h), dptr(intrinsic), n_hyp, iptr(samples),
                                       float(threshold), dptr(rot), dptr(loc), iptr(mask), ctypes.byref(cnt),
                                       ctypes.byref(best)))
    idx = np.flatnonzero(mask)
    return rot, loc.reshape(3, 1), (idx if as_array else idx.tolist()), best.value


def comm_available():
    """True when the library can load RCCL in this process (sfm_comm_available)."""
    return load().sfm_comm_available() == OK


def comm_unique_id():
    """128 opaque bytes identifying a new RCCL communicator (rank 0 calls this and hands them to the other ranks)."""
    buf = ctypes.create_string_buffer(128)
    check(load().sfm_comm_unique_id(buf))
    return buf.raw


class Comm:
    """A library-owned RCCL communicator of this process' GPU (sfm_comm_create / sfm_comm_destroy)."""

    def __init__(self, world_size, rank, unique_id):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        self._lib = load()
        self._h = ctypes.c_void_p()
        check(self._lib.sfm_comm_create(int(world_size), int(rank), bytes(unique_id), ctypes.byref(self._h)))
        self.world_size, self.rank = int(world_size), int(rank)

    def close(self):
        if self._h:
            check(self._lib.sfm_comm_destroy(self._h))      # refused (SfmHipError) while a problem still holds it
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def pnp_ransac_evaluate(uv_pix, pts_h, intrinsic, samples, threshold):
    """Every six-point hypothesis: (rot (n_hyp,3,3), loc (n_hyp,3), inlier counts under (R, C), inlier counts under (R, -C))."""
    uv_pix = f64(uv_pix); pts_h = f64(pts_h); intrinsic = f64(intrinsic)
    samples = i32(samples).reshape(-1, 6)
    n, n_hyp = uv_pix.shape[1], samples.shape[0]
    rot = np.empty((n_hyp, 3, 3)); loc = np.empty((n_hyp, 3))
    cnt = np.empty(n_hyp, dtype=np.int32); cnt_neg = np.empty(n_hyp, dtype=np.int32)
    check(load().sfm_pnp_ransac_evaluate(n, dptr(uv_pix), dptr(pts_h), dptr(intrinsic), n_hyp, iptr(samples),
                                         float(threshold), dptr(rot), dptr(loc), iptr(cnt), iptr(cnt_neg)))
    return rot, loc, cnt, cnt_neg


def pnp_ransac_begin(uv_pix, pts_h, intrinsic, samples, threshold):
    """``pnp_ransac_evaluate`` that keeps the view's keys and points on the device: returns (session handle, rot (n_hyp,3,3),
    loc (n_hyp,3), counts, counts_neg).  The handle goes to ``pnp_ransac_finish`` (or ``pnp_session_destroy``)."""
    uv_pix = f64(uv_pix); pts_h = f64(pts_h); intrinsic = f64(intrinsic)
    samples = i32(samples).reshape(-1, 6)
    n, n_hyp = uv_pix.shape[1], samples.shape[0]
    rot = np.empty((n_hyp, 3, 3)); loc = np.empty((n_hyp, 3))
    cnt = np.empty(n_hyp, dtype=np.int32); cnt_neg = np.empty(n_hyp, dtype=np.int32)
    handle = ctypes.c_void_p()
    check(load().sfm_pnp_ransac_begin(n, dptr(uv_pix), dptr(pts_h), dptr(intrinsic), n_hyp, iptr(samples), float(threshold),
                                      dptr(rot), dptr(loc), iptr(cnt), iptr(cnt_neg), ctypes.byref(handle)))
    return (handle, n), rot, loc, cnt, cnt_neg


def pnp_ransac_finish(session, rot, loc, threshold, lam, iters, quirks=QUIRKS_REFERENCE):
    """Inlier mask of the pose (rot, loc) on the session's resident view, the inlier columns compacted on the device, ``iters``
    nonlinear PnP iterations on them: returns (inlier indices (int array, ascending), R (3,3), C (3,1)).  Releases the session."""
    handle, n = session
    rot = f64(rot); loc = f64(loc).reshape(3)
    mask = np.empty(n, dtype=np.int32)
    cnt = ctypes.c_int()
    r_out = np.empty((3, 3)); c_out = np.empty(3)
    check(load().sfm_pnp_ransac_finish(handle, dptr(rot), dptr(loc), float(threshold), float(lam), int(iters), int(quirks),
                                       iptr(mask), ctypes.byref(cnt), dptr(r_out), dptr(c_out)))
    return np.flatnonzero(mask), r_out, c_out.reshape(3, 1)


def pnp_session_destroy(session):
    handle, _n = session
    check(load().sfm_pnp_session_destroy(handle))


def pnp_inlier_mask(uv_pix, pts_h, intrinsic, rot, loc, threshold, as_array=False):
    """Inlier index list (or int array) of one pose (pixel reprojection error below `threshold`, campose_processor.py:544-554)."""
    uv_pix = f64(uv_pix); pts_h = f64(pts_h); intrinsic = f64(intrinsic); rot = f64(rot); loc = f64(loc).reshape(3)
    n = uv_pix.shape[1]
    mask = np.empty(n, dtype=np.int32)
    cnt = ctypes.c_int()
    check(load().sfm_pnp_inlier_mask(n, dptr(uv_pix), dptr(pts_h), dptr(intrinsic), dptr(rot), dptr(loc), float(threshold),
                                     iptr(mask), ctypes.byref(cnt)))
    idx = np.flatnonzero(mask)
    return idx if as_array else idx.tolist()


def pnp_six_point_hypotheses(uv_pix, pts_h, intrinsic, samples, threshold):
    """Parity hook: (rot (n_hyp,3,3), loc (n_hyp,3), inlier counts (n_hyp,)) of every six-point hypothesis."""
    uv_pix = f64(uv_pix); pts_h = f64(pts_h); intrinsic = f64(intrinsic)
    samples = i32(samples).reshape(-1, 6)
    n, n_hyp = uv_pix.shape[1], samples.shape[0]
    rot = np.empty((n_hyp, 3, 3)); loc = np.empty((n_hyp, 3)); cnt = np.empty(n_hyp, dtype=np.int32)
    check(load().sfm_pnp_six_point_hypotheses(n, dptr(uv_pix), dptr(pts_h), dptr(intrinsic), n_hyp, iptr(samples),
                                              float(threshold), dptr(rot), dptr(loc), iptr(cnt)))
    return rot, loc, cnt


def fundamental_ransac(left, right, samples, threshold, return_count=False):
    """Eight-point RANSAC (epipolar_processor.py:22-57).  left/right: (>=2, n) pixel rows; samples: (n_hyp, 8)
    indices drawn by the caller (ignored when n == 8).  Returns (F (3,3), inlier index list or None, best
    hypothesis index or -1); with ``return_count`` a fourth item, the inlier count that chose the winner (the
    scoring kernel's, not the length of the list, which the finishing kernel recomputes)."""
    left = f64(np.asarray(left)[0:2]); right = f64(np.asarray(right)[0:2])
    n = left.shape[1]
    samples = i32(samples if samples is not None and n != 8 else np.arange(8)).reshape(-1, 8)
    fund = np.empty((3, 3)); mask = np.empty(max(n, 1), dtype=np.int32)
    cnt = ctypes.c_int(); best = ctypes.c_int()
    check(load().sfm_fundamental_ransac(n, dptr(left), dptr(right), samples.shape[0], iptr(samples), float(threshold),
                                        dptr(fund), iptr(mask), ctypes.byref(cnt), ctypes.byref(best)))
    inliers = None if best.value < 0 else np.flatnonzero(mask[:n]).tolist()
    if return_count:
        return fund, inliers, best.value, cnt.value
    return fund, inliers, best.value


def fundamental_eight_point(pairs, samples):
    """epipolar_processor.py:140-193 for every 8-index sample of the normalised pairs (n, 4) -> (F (n_hyp,3,3), status)."""
    pairs = f64(pairs); samples = i32(samples).reshape(-1, 8)
    out = np.empty((samples.shape[0], 3, 3)); st = np.empty(samples.shape[0], dtype=np.int32)
    check(load().sfm_fundamental_eight_point(pairs.shape[0], dptr(pairs), samples.shape[0], iptr(samples), dptr(out), iptr(st)))
    return out, st


def essential_from_fundamental(fund, left_k, right_k):
    """epipolar_processor.py:60-95."""
    fund = f64(fund); left_k = f64(left_k); right_k = f64(right_k)
    out = np.empty((3, 3))
    check(load().sfm_essential_from_fundamental(dptr(fund), dptr(left_k), dptr(right_k), dptr(out)))
    return out


def pose_candidates(esse):
    """campose_processor.py:29-100 -> (r1, r2, c1 (3,1), c2 = -c1)."""
    esse = f64(esse)
    rots = np.empty((2, 3, 3)); c1 = np.empty(3)
    check(load().sfm_pose_candidates(dptr(esse), dptr(rots), dptr(c1)))
    return rots[0].copy(), rots[1].copy(), c1.reshape(3, 1).copy(), -c1.reshape(3, 1)


def cheirality(ref_proj, projs, pts_sets):
    """campose_processor.py:102-189 for k candidates: projs (k,3,4), pts_sets (k,4,n) -> (masks (k,n), counts (k,), best)."""
    ref_proj = f64(ref_proj); projs = f64(projs).reshape(-1, 3, 4)
    pts_sets = f64(pts_sets).reshape(projs.shape[0], 4, -1)
    k, n = projs.shape[0], pts_sets.shape[2]
    mask = np.zeros((k, max(n, 1)), dtype=np.int32); counts = np.zeros(k, dtype=np.int32)
    best = ctypes.c_int()
    check(load().sfm_cheirality(k, n, dptr(ref_proj), dptr(projs), dptr(pts_sets), iptr(mask), iptr(counts), ctypes.byref(best)))
    return mask[:, :n], counts, best.value


def pnp_nonlinear_batch(offsets, uv_pix, pts_h, intrinsics, rot0, loc0, lam, iters, quirks=QUIRKS_REFERENCE):
    offsets = i32(offsets); uv_pix = f64(uv_pix); pts_h = f64(pts_h)
    intrinsics = f64(intrinsics).reshape(-1, 3, 3); rot0 = f64(rot0).reshape(-1, 3, 3); loc0 = f64(loc0).reshape(-1, 3)
    nv = offsets.shape[0] - 1
    total = uv_pix.shape[1]
    rot = np.empty((nv, 3, 3)); loc = np.empty((nv, 3)); st = np.empty(nv, dtype=np.int32)
    check(load().sfm_pnp_nonlinear_batch(nv, iptr(offsets), total, dptr(uv_pix), dptr(pts_h), dptr(intrinsics),
                                         dptr(rot0), dptr(loc0), float(lam), int(iters), int(quirks),
                                         dptr(rot), dptr(loc), iptr(st)))
    return rot, loc, st


def ba_residual_jacobian(n_cams, pt_ptr, cam_idx, uv_norm, cams, pts, quirks=QUIRKS_REFERENCE):
    pt_ptr = i32(pt_ptr); cam_idx = i32(cam_idx); uv_norm = f64(uv_norm); cams = f64(cams); pts = f64(pts)
    n, m = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    r = np.empty((m, 2)); jp = np.empty((m, 2, 7)); jx = np.empty((m, 2, 3))
    check(load().sfm_ba_residual_jacobian(n_cams, n, m, iptr(pt_ptr), iptr(cam_idx), dptr(uv_norm), dptr(cams),
                                          dptr(pts), quirks, dptr(r), dptr(jp), dptr(jx)))
    return r, jp, jx


def ba_reduced_system(n_cams, pt_ptr, cam_idx, uv_norm, cams, pts, lam, quirks=QUIRKS_REFERENCE,
                      schur_mode=SCHUR_AUTO, loss=None):
    """S, rhs of one linearisation; ``loss=(kind, delta)`` reweights it as ``BaProblem.set_loss`` does."""
    pt_ptr = i32(pt_ptr); cam_idx = i32(cam_idx); uv_norm = f64(uv_norm); cams = f64(cams); pts = f64(pts)
    n, m = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    s = np.empty((7 * n_cams, 7 * n_cams)); rhs = np.empty(7 * n_cams)
    if loss is not None:
        kind, delta = check_loss(*loss)
        check(load().sfm_ba_reduced_system_loss(n_cams, n, m, iptr(pt_ptr), iptr(cam_idx), dptr(uv_norm), dptr(cams),
                                                dptr(pts), float(lam), quirks, schur_mode, kind, delta, dptr(s), dptr(rhs)))
        return s, rhs
    check(load().sfm_ba_reduced_system(n_cams, n, m, iptr(pt_ptr), iptr(cam_idx), dptr(uv_norm), dptr(cams),
                                       dptr(pts), float(lam), quirks, schur_mode, dptr(s), dptr(rhs)))
    return s, rhs


def ba_solve(n_cams, pt_ptr, cam_idx, uv_norm, cams, pts, lam, iters, quirks=QUIRKS_REFERENCE):
    pt_ptr = i32(pt_ptr); cam_idx = i32(cam_idx); uv_norm = f64(uv_norm)
    cams = np.array(cams, dtype=np.float64, order="C", copy=True).reshape(-1, 7)
    pts = np.array(pts, dtype=np.float64, order="C", copy=True)
    n, m = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    check(load().sfm_ba_solve(n_cams, n, m, iptr(pt_ptr), iptr(cam_idx), dptr(uv_norm), dptr(cams), dptr(pts),
                              float(lam), int(iters), int(quirks)))
    return cams, pts


def refine_cameras_plan(n_obs):
    """How ``BaProblem.refine_cameras`` works on a camera of ``n_obs`` observations (sfm_ba_refine_cameras_plan; host only):
    ``(n_slices, slice_obs, size_class)`` -- the sums are formed per slice of ``slice_obs`` consecutive observations and
    added in slice order; size class 0 = empty, 1 / 2 / 3 = one launch for all iterations, 4 = two launches per pass."""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(load().sfm_ba_refine_cameras_plan(int(n_obs), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def covariance_plan(n_cams):
    """How ``BaProblem.covariance`` inverts the camera system of ``n_cams`` cameras (sfm_ba_covariance_plan; host only):
    ``(block size, blocks per side, kernel launches of the inverse, longest track a lane group takes)``."""
    a, b, c, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(load().sfm_ba_covariance_plan(int(n_cams), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


def sym3(packed):
    """(N, 6) packed (xx, xy, xz, yy, yz, zz) -> (N, 3, 3) symmetric blocks."""
    packed = np.asarray(packed)
    return packed[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


class BaProblem:
    """Device-resident BA problem (sfm_ba_create ... sfm_ba_destroy)."""

    def __init__(self, n_cams, pt_ptr, cam_idx, uv_norm):
        self._lib = load()
        pt_ptr = i32(pt_ptr); cam_idx = i32(cam_idx); uv_norm = f64(uv_norm)
        self.n_cams = int(n_cams)
        self.n_pts = pt_ptr.shape[0] - 1
        self.n_obs = cam_idx.shape[0]
        if uv_norm.shape != (2, self.n_obs):
            raise ValueError("uv_norm must be (2, M)")
        h = ctypes.c_void_p()
        check(self._lib.sfm_ba_create(self.n_cams, self.n_pts, self.n_obs, iptr(pt_ptr), iptr(cam_idx),
                                      dptr(uv_norm), ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_tracks(cls, store):
        """A problem whose structure is ``store``'s current observation list (``TrackStore.build_observations``), copied
        device to device (sfm_ba_create_from_tracks): nothing is uploaded."""
        self = cls.__new__(cls)
        self._lib = load()
        self._h = None
        h = ctypes.c_void_p()
        check(self._lib.sfm_ba_create_from_tracks(store._h, ctypes.byref(h)))
        self._h = h
        self._read_sizes()
        return self

    def _read_sizes(self):
        self.n_cams, self.n_pts, self.n_obs = self.info(INFO_N_CAMS), self.info(INFO_N_PTS), self.info(INFO_N_OBS)

    def sync_tracks(self, store, cams_new=None, pts_new=None):
        """Bring the problem up to ``store``'s current observation list (sfm_ba_sync_tracks); ``cams_new`` (k, 7) and
        ``pts_new`` (3, k) are the cameras and points the list has beyond the resident ones.  Returns
        ``(action, n_new_obs)``: ``SYNC_REUSE`` (nothing changed), ``SYNC_GROWN`` (the problem took the list over; only the
        new cameras and points went up) or ``SYNC_REPLACED`` (the problem is unchanged: build a new one)."""
        cams_new = f64(np.zeros((0, 7)) if cams_new is None else cams_new).reshape(-1, 7)
        pts_new = f64(np.zeros((3, 0)) if pts_new is None else pts_new).reshape(3, -1)
        action, n_new = ctypes.c_int(), ctypes.c_int64()
        check(self._lib.sfm_ba_sync_tracks(self._h, store._h, cams_new.shape[0], dptr(cams_new) if cams_new.size else None,
                                           pts_new.shape[1], dptr(pts_new) if pts_new.size else None, ctypes.byref(action),
                                           ctypes.byref(n_new)))
        if action.value == SYNC_GROWN:
            self._read_sizes()
        return action.value, int(n_new.value)

    def structure(self, want_uv=True):
        """(pt_ptr (N+1,), cam_idx (M,), uv_norm (2, M)): the resident observation list (sfm_ba_get_structure);
        ``want_uv=False`` leaves the keys on the device and returns None in their place."""
        n, m = self.info(INFO_N_PTS), self.info(INFO_N_OBS)
        pt_ptr, cam_idx = np.zeros(n + 1, dtype=np.int32), np.zeros(m, dtype=np.int32)
        uv = np.zeros((2, m)) if want_uv else None
        check(self._lib.sfm_ba_get_structure(self._h, iptr(pt_ptr), iptr(cam_idx) if m else None,
                                             dptr(uv) if m and want_uv else None))
        return pt_ptr, cam_idx, uv

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sfm_ba_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, option, value):
        check(self._lib.sfm_ba_set_option(self._h, option, value))

    def set_stream(self, stream_ptr):
        """Run this problem on an existing HIP stream (``torch.cuda.Stream.cuda_stream``); 0 / None = the library's own."""
        check(self._lib.sfm_ba_set_stream(self._h, ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def info(self, what):
        v = ctypes.c_int64()
        check(self._lib.sfm_ba_info(self._h, int(what), ctypes.byref(v)))
        return int(v.value)

    @property
    def upload_bytes(self):
        return self.info(INFO_UPLOAD_BYTES)

    def set_state(self, cams, pts):
        cams = f64(cams).reshape(-1, 7); pts = f64(pts)
        if cams.shape[0] != self.n_cams or pts.shape != (3, self.n_pts):
            raise ValueError("state shapes do not match the problem")
        check(self._lib.sfm_ba_set_state(self._h, dptr(cams), dptr(pts)))

    def transform(self, s, A, t):
        """Move the resident scene by ``X' = s A X + t`` on the device (sfm_ba_transform): points by the formula, every
        camera to ``C' = s A C + t``, ``q' = q(A R(q))``.  ValueError for a non-positive ``s``, an ``A`` that is no rotation,
        or a camera the move takes to a half turn (the scene is then unchanged)."""
        A, t = f64(A).reshape(3, 3), f64(t).reshape(3)
        check(self._lib.sfm_ba_transform(self._h, float(s), dptr(A), dptr(t)))

    def align(self, point_idx, targets, max_err2, max_hyp=0, iters=2, rigid=False, apply=True):
        """Align the resident scene to ``targets`` (3, n) of its points ``point_idx`` (n,) by a robust similarity
        (sfm_ba_align): the points are gathered on the device, ``similarity_ransac`` runs on them as one set, and with
        ``apply`` and a model the scene is moved by it without a round trip.  Returns ``(sim (13,), inlier (n,) uint8,
        n_inliers, best_hyp, status)``; too few correspondences or no model leave the scene untouched and say so in
        ``status``."""
        point_idx = np.ascontiguousarray(point_idx, dtype=np.int32).ravel()
        targets = f64(targets)
        n = point_idx.shape[0]
        if targets.shape != (3, n):
            raise ValueError("targets must be (3, %d), got %r" % (n, targets.shape))
        max_err2, max_hyp, iters, flags = check_similarity(max_err2, max_hyp, iters, rigid)
        sim = np.zeros(13)
        inlier = np.zeros(n, dtype=np.uint8)
        cnt, best, status = ci(0), ci(-1), ci(0)
        check(self._lib.sfm_ba_align(self._h, n, iptr(point_idx) if n else None, dptr(targets) if n else None, max_err2, max_hyp,
                                     iters, flags, 1 if apply else 0, dptr(sim), _u8ptr(inlier) if n else None,
                                     ctypes.byref(cnt), ctypes.byref(best), ctypes.byref(status)))
        return sim, inlier, int(cnt.value), int(best.value), int(status.value)

    def set_cameras(self, cams):
        cams = f64(cams).reshape(-1, 7)
        if cams.shape[0] != self.n_cams:
            raise ValueError("camera count does not match the problem")
        check(self._lib.sfm_ba_set_cameras(self._h, dptr(cams)))

    def set_points(self, first, pts):
        pts = f64(pts).reshape(3, -1)
        check(self._lib.sfm_ba_set_points(self._h, int(first), pts.shape[1], dptr(pts)))

    def iterate(self, lam, iters, quirks=QUIRKS_REFERENCE):
        check(self._lib.sfm_ba_iterate(self._h, float(lam), int(iters), int(quirks)))

    def linearize_reduce(self, lam, quirks=QUIRKS_REFERENCE):
        check(self._lib.sfm_ba_linearize_reduce(self._h, float(lam), int(quirks)))

    def solve_update(self, lam, quirks=QUIRKS_REFERENCE):
        check(self._lib.sfm_ba_solve_update(self._h, float(lam), int(quirks)))

    def flush(self):
        """Complete the back substitution ``solve_update`` may have left to the next linearisation (sfm_ba_flush)."""
        check(self._lib.sfm_ba_flush(self._h))

    def set_comm(self, comm):
        """Attach a library-owned RCCL communicator (``Comm``) or detach it (None): ``iterate`` then all-reduces the
        packed [S | rhs] buffer itself, once per iteration, on the problem's stream (sfm_ba_set_comm)."""
        check(self._lib.sfm_ba_set_comm(self._h, comm._h if comm is not None else None))
        self._comm = comm                      # keep it alive as long as it is attached

    def get_stats(self, max_iters=256):
        """Per-iteration cost sum |b - f|^2 (normalised image coordinates; delta^2 sum rho(s) while a loss is set) at the
        start of every iteration run since the state was last uploaded -- no state download needed (sfm_ba_get_stats)."""
        out = np.empty(max_iters); n = ctypes.c_int()
        check(self._lib.sfm_ba_get_stats(self._h, dptr(out), int(max_iters), ctypes.byref(n)))
        return out[:n.value].copy()

    def set_loss(self, kind, delta=1.0):
        """Robust loss of the iterations (sfm_ba_set_loss): ``LOSS_NONE`` / ``LOSS_HUBER`` / ``LOSS_CAUCHY`` (or its name)
        with scale ``delta`` in normalised units.  Completes a pending step with the old loss, restarts the cost history,
        uploads nothing; survives ``append``, ``cull`` and ``sync_tracks``."""
        kind, delta = check_loss(kind, delta)
        check(self._lib.sfm_ba_set_loss(self._h, kind, delta))

    def loss(self):
        """(kind, delta) as set by ``set_loss`` (sfm_ba_get_loss)."""
        kind, delta = ctypes.c_int(), ctypes.c_double()
        check(self._lib.sfm_ba_get_loss(self._h, ctypes.byref(kind), ctypes.byref(delta)))
        return int(kind.value), float(delta.value)

    def loss_terms(self):
        """(s, w, rho), each (M,): every observation's scaled squared residual, weight and loss value at the current state
        (sfm_ba_loss_terms); without a loss s = |b - f|^2, w = 1, rho = s."""
        m = self.info(INFO_N_OBS)
        s, w, rho = np.zeros(m), np.zeros(m), np.zeros(m)
        check(self._lib.sfm_ba_loss_terms(self._h, dptr(s), dptr(w), dptr(rho)))
        return s, w, rho

    def get_state(self):
        cams = np.empty((self.n_cams, 7)); pts = np.empty((3, self.n_pts))
        check(self._lib.sfm_ba_get_state(self._h, dptr(cams), dptr(pts)))
        return cams, pts

    def get_state_rot(self):
        """(cams (V,7), pts (3,N), rots (V,3,3)): the state plus R(q) of every camera, validated on the device."""
        cams = np.empty((self.n_cams, 7)); pts = np.empty((3, self.n_pts)); rots = np.empty((self.n_cams, 3, 3))
        check(self._lib.sfm_ba_get_state_rot(self._h, dptr(cams), dptr(pts), dptr(rots)))
        return cams, pts, rots

    def rederive_quaternions(self, first, count):
        """q <- q(R(q)) on the device for cameras [first, first + count) (sfm_ba_rederive_quaternions)."""
        check(self._lib.sfm_ba_rederive_quaternions(self._h, int(first), int(count)))

    def append(self, cams_new, pts_new, obs_cam, obs_pt, uv_norm):
        """Grow the resident scene (sfm_ba_append): new cameras (k,7), new points (3,k), new observations
        (camera index, point index, normalised key (2,m)) of pairs not yet present; nothing already on the
        device is uploaded again."""
        cams_new = f64(cams_new).reshape(-1, 7); pts_new = f64(pts_new).reshape(3, -1)
        obs_cam = i32(obs_cam).ravel(); obs_pt = i32(obs_pt).ravel(); uv_norm = f64(uv_norm).reshape(2, -1)
        if not (obs_cam.shape[0] == obs_pt.shape[0] == uv_norm.shape[1]):
            raise ValueError("append: obs_cam, obs_pt and uv_norm disagree in length")
        check(self._lib.sfm_ba_append(self._h, cams_new.shape[0], dptr(cams_new), pts_new.shape[1], dptr(pts_new),
                                      obs_cam.shape[0], iptr(obs_cam), iptr(obs_pt), dptr(uv_norm)))
        self.n_cams += cams_new.shape[0]
        self.n_pts += pts_new.shape[1]
        self.n_obs += obs_cam.shape[0]

    def refine_points(self, lam, iters, mode=TRACKS_NONLINEAR, group=0, want_outputs=True):
        """Structure-only refinement of the resident points, cameras held (sfm_ba_refine_points): returns
        (cost (2, N), status (N,)) as ``tri_tracks`` does; ``want_outputs=False`` downloads neither and returns None."""
        mode, iters, group = _tracks_mode_group(mode, iters, group)
        n = self.info(INFO_N_PTS)
        if not want_outputs:
            check(self._lib.sfm_ba_refine_points(self._h, mode, float(lam), iters, group, None, None))
            return None
        cost = np.zeros((2, n)); status = np.zeros(n, dtype=np.int32)
        check(self._lib.sfm_ba_refine_points(self._h, mode, float(lam), iters, group, dptr(cost), iptr(status)))
        return cost, status

    def retriangulate(self, max_err2, cos_min_angle=1.0, max_hyp=0, lam=0.5, iters=3, cam_scale=None, group=0, want_outputs=True):
        """Robust re-triangulation of the resident points, cameras held (sfm_ba_retriangulate): every point from the
        consistent subset of its own track, in place.  Returns a namespace with ``inlier`` (M,) uint8, ``n_inliers`` (N,),
        ``best_hyp`` (N,), ``status`` (N,) of ``RANSAC_*`` bits and ``summary`` (6,) int64 in the order of
        ``RANSAC_SUMMARY``; ``want_outputs=False`` downloads nothing and returns None."""
        max_err2, cos_min_angle, max_hyp, lam, iters, cam_scale, group = check_ransac(self.n_cams, max_err2, cos_min_angle,
                                                                                      max_hyp, lam, iters, cam_scale, group)
        out = _ransac_outputs(self.info(INFO_N_PTS), self.info(INFO_N_OBS)) if want_outputs else None
        check(self._lib.sfm_ba_retriangulate(self._h, max_err2, cos_min_angle, max_hyp, lam, iters, group, dptr(cam_scale),
                                             *(_ransac_pointers(out) if want_outputs else (None,) * 5)))
        return out

    def resect(self, max_err2, max_hyp=0, lam=0.5, iters=3, quirks=QUIRKS_REFERENCE, mask=None, cam_scale=None, want_outputs=True):
        """Robust resection of the resident cameras, points held (sfm_ba_resect): every camera from the consistent subset
        of its own observations, in place.  ``mask`` (V,): cameras with a zero entry are held and only judged.  Returns a
        namespace with ``inlier`` (M,) uint8 in the scene's observation order, ``n_inliers`` (V,), ``best_hyp`` (V,),
        ``status`` (V,) of ``RESECT_*`` bits and ``summary`` (6,) int64 in the order of ``RESECT_SUMMARY``;
        ``want_outputs=False`` downloads nothing and returns None."""
        v = self.info(INFO_N_CAMS)
        max_err2, max_hyp, lam, iters, mask, cam_scale = check_resect(v, max_err2, max_hyp, lam, iters, mask, cam_scale)
        out = _ransac_outputs(v, self.info(INFO_N_OBS)) if want_outputs else None
        check(self._lib.sfm_ba_resect(self._h, max_err2, max_hyp, lam, iters, int(quirks), _u8ptr(mask), dptr(cam_scale),
                                      *(_ransac_pointers(out) if want_outputs else (None,) * 5)))
        return out

    def refine_cameras(self, lam, iters, quirks=QUIRKS_REFERENCE, use_loss=False, mask=None, want_cost=False, want_status=False):
        """Motion-only refinement of the resident cameras, points held (sfm_ba_refine_cameras): ``iters`` damped steps per
        camera over its own observations, reweighted by the problem's loss when ``use_loss``.  ``mask`` (V,): cameras with
        a zero entry are held (None: every camera moves).  Returns ``(cost (2, V) or None, status (V,) of CAM_* bits or
        None)`` as ``want_cost`` / ``want_status`` ask."""
        v = self.info(INFO_N_CAMS)
        mask = _cam_mask(mask, v)
        cost = np.zeros((2, v)) if want_cost else None
        status = np.zeros(v, dtype=np.int32) if want_status else None
        check(self._lib.sfm_ba_refine_cameras(self._h, float(lam), int(iters), int(quirks), int(use_loss),
                                              _u8ptr(mask), dptr(cost), iptr(status)))
        return cost, status

    def covariance(self, lam, quirks=QUIRKS_REFERENCE, use_loss=False, mask=None, group=0, want_cameras=True, want_points=True):
        """Covariance blocks of the resident scene at its current state (sfm_ba_covariance), the cameras with a zero
        ``mask`` entry held (None: every camera free, which needs ``lam > 0`` and says little: hold at least two).
        Returns a namespace: ``cam_cov`` (V, 7, 7) or None, ``pt_cov`` (N, 6) packed (xx, xy, xz, yy, yz, zz) or None
        (``sym3`` expands it), ``cam_status`` (V,) of ``COV_CAM_*`` bits, ``pt_status`` (N,) of ``COV_PT_*`` bits,
        ``sigma0_sq``, and ``pivot_camera``: None, or the camera at which the free cameras' system turned out not to be
        positive definite -- then the covariances are None and ``sigma0_sq`` is NaN.  Nothing is scaled by ``sigma0_sq``."""
        v, n = self.info(INFO_N_CAMS), self.info(INFO_N_PTS)
        group, mask = _check_group(group), _cam_mask(mask, v)
        out = SimpleNamespace(cam_cov=np.zeros((v, 7, 7)) if want_cameras else None,
                              pt_cov=np.zeros((n, 6)) if want_points else None,
                              cam_status=np.zeros(v, dtype=np.int32), pt_status=np.zeros(n, dtype=np.int32),
                              sigma0_sq=float("nan"), pivot_camera=None)
        s0 = ctypes.c_double(float("nan"))
        st = self._lib.sfm_ba_covariance(self._h, float(lam), int(quirks), int(bool(use_loss)),
                                         _u8ptr(mask),
                                         group, dptr(out.cam_cov), dptr(out.pt_cov), iptr(out.cam_status), iptr(out.pt_status),
                                         ctypes.byref(s0))
        if st == E_SINGULAR:
            out.pivot_camera = int(np.flatnonzero(out.cam_status & COV_CAM_PIVOT)[0])
            out.cam_cov = out.pt_cov = None
            return out
        check(st)
        out.sigma0_sq = s0.value
        return out

    def covariance_times(self):
        """Device milliseconds of the last ``covariance`` call's phases (terms, S, inverse, points) when an ``OPT_TIMING``
        bit was set during it (sfm_ba_covariance_times); zeros otherwise."""
        ms = np.zeros(4)
        check(self._lib.sfm_ba_covariance_times(self._h, dptr(ms)))
        return ms

    def iterate_pcg(self, lam, iters, quirks=QUIRKS_REFERENCE, mask=None, tol=1e-10, max_cg=0, group=0):
        """``iters`` bundle-adjustment iterations with the reduced camera system solved matrix-free by block-Jacobi PCG
        (sfm_ba_iterate_pcg); cameras with a zero ``mask`` entry are held (None: every camera moves).  ``tol`` is the
        relative tolerance on the preconditioned residual, ``max_cg`` the CG iteration limit (0: min(7 V_free, 1000)).
        Returns a namespace: ``iters_done``, and per outer iteration ``cost``, ``cg_iters``, ``cg_rel``, ``cg_status``
        (``PCG_CONVERGED`` / ``PCG_MAX_ITERS`` / ``PCG_BREAKDOWN``).  Raises ``SfmSingularError`` (``.camera``) when a free
        camera's diagonal block does not factor; the state is then as it was."""
        lam, iters, mask, tol, max_cg, group = check_pcg(self.info(INFO_N_CAMS), lam, iters, mask, tol, max_cg, group)
        n = max(iters, 1)
        cost, rel = np.zeros(n), np.zeros(n)
        cg, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        done, bad = ctypes.c_int(0), ctypes.c_int(-1)
        st = self._lib.sfm_ba_iterate_pcg(self._h, lam, iters, int(quirks),
                                          _u8ptr(mask),
                                          tol, max_cg, group, ctypes.byref(done), dptr(cost), iptr(cg), dptr(rel), iptr(status),
                                          ctypes.byref(bad))
        if st == E_SINGULAR:
            raise SfmSingularError(last_error(), int(bad.value))
        check(st)
        k = int(done.value)
        return SimpleNamespace(iters_done=k, cost=cost[:k].copy(), cg_iters=cg[:k].copy(), cg_rel=rel[:k].copy(),
                               cg_status=status[:k].copy())

    def cost(self, quirks=QUIRKS_REFERENCE, group=0):
        """The minimised cost at the current state, computed on the device from residuals alone (sfm_ba_cost): the robust
        cost while a loss is set.  Changes nothing on the problem."""
        out = ctypes.c_double(0.0)
        check(self._lib.sfm_ba_cost(self._h, int(quirks), _check_group(group), ctypes.byref(out)))
        return float(out.value)

    def minimize_pcg(self, mask=None, **options):
        """Levenberg-Marquardt minimisation on the matrix-free route (sfm_ba_minimize_pcg): every trial is one outer
        iteration of ``iterate_pcg`` whose step stands only if it lowered the cost by more than ``LM_MIN_GAIN`` of what the
        linear model predicted; the damping adapts and the call stops by itself.  ``options`` are the fields of
        ``LmOptions`` (``LM_DEFAULTS``); cameras with a zero ``mask`` entry are held.  Returns a namespace: ``trials``,
        ``accepted``, ``stop`` (``LM_STOP_*``), ``lam`` (the damping the next trial would use), ``cost`` (of the state the
        problem is left in: the last accepted one), ``bad_camera`` (``LM_STOP_SINGULAR``) and ``log``, a structured array
        with the fields of ``LmTrial``, one row per trial."""
        opt, mask = check_lm(self.info(INFO_N_CAMS), mask, **options)
        log = (LmTrial * max(opt.max_trials, 1))()
        trials, accepted, stop, bad = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(-1)
        lam, cost = ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(self._lib.sfm_ba_minimize_pcg(self._h, ctypes.byref(opt), _u8ptr(mask), log, ctypes.byref(trials),
                                            ctypes.byref(accepted), ctypes.byref(stop), ctypes.byref(lam), ctypes.byref(cost),
                                            ctypes.byref(bad)))
        rows = np.frombuffer(log, dtype=LM_TRIAL_DTYPE)[:trials.value].copy()
        return SimpleNamespace(trials=int(trials.value), accepted=int(accepted.value), stop=int(stop.value), lam=float(lam.value),
                               cost=float(cost.value), bad_camera=int(bad.value), log=rows)

    def pcg_times(self):
        """Milliseconds of the last ``iterate_pcg`` call, summed over its outer iterations: (linearise, camera blocks, CG
        loop, back substitution, whole call).  The first four are device times and zeros unless an ``OPT_TIMING`` bit was
        set during the call; the last is the host's clock (sfm_ba_pcg_times)."""
        ms = np.zeros(5)
        check(self._lib.sfm_ba_pcg_times(self._h, dptr(ms)))
        return ms

    def _screen(self, name, max_err2, cos_min_angle, min_obs, cam_scale, want_outputs, group):
        max_err2, cos_min_angle, min_obs, cam_scale, group = check_screen(self.n_cams, max_err2, cos_min_angle, min_obs,
                                                                          cam_scale, group)
        n, m = self.info(INFO_N_PTS), self.info(INFO_N_OBS)
        summary = np.zeros(8, dtype=np.int64)
        out = SimpleNamespace(err2=None, depth=None, obs_flags=None, min_cos=None, pt_flags=None, summary=summary)
        if want_outputs:
            out.err2, out.depth, out.obs_flags = np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.uint8)
            out.min_cos, out.pt_flags = np.ones(n), np.zeros(n, dtype=np.int32)
        check(getattr(self._lib, name)(self._h, max_err2, cos_min_angle, min_obs, group,
                                         dptr(cam_scale), dptr(out.err2), dptr(out.depth), _u8ptr(out.obs_flags),
                                         dptr(out.min_cos), iptr(out.pt_flags), _lptr(summary)))
        return out

    def screen(self, max_err2=float("inf"), cos_min_angle=1.0, min_obs=2, cam_scale=None, want_outputs=True, group=0):
        """Judge every observation and point of the resident scene at its current state (sfm_ba_screen) without changing
        anything: returns a namespace with ``err2`` (M,), ``depth`` (M,), ``obs_flags`` (M,) uint8 of ``OBS_*`` bits,
        ``min_cos`` (N,), ``pt_flags`` (N,) of ``PT_*`` bits and ``summary`` (8,) int64 in the order of ``SCREEN_SUMMARY``.
        ``cam_scale`` (V,) multiplies a camera's residuals (None: 1); ``want_outputs=False`` downloads the summary only."""
        return self._screen("sfm_ba_screen", max_err2, cos_min_angle, min_obs, cam_scale, want_outputs, group)

    def cull(self, max_err2=float("inf"), cos_min_angle=1.0, min_obs=2, cam_scale=None, want_outputs=True, group=0):
        """``screen``, then remove what failed from the resident scene on the device (sfm_ba_cull): the report describes the
        scene before the cull, ``obs_flags == 0`` marks what remains.  Cameras, points and their indices are unchanged."""
        out = self._screen("sfm_ba_cull", max_err2, cos_min_angle, min_obs, cam_scale, want_outputs, group)
        self.n_obs = self.info(INFO_N_OBS)
        return out

    def points_ptr(self):
        """Device pointers (px, py, pz) of the resident points and their count (sfm_ba_points_ptr)."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        n = ctypes.c_int()
        check(self._lib.sfm_ba_points_ptr(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(n)))
        return a.value, b.value, c.value, n.value

    def stream_ptr(self):
        """The HIP stream this problem runs on (hipStream_t as an integer; sfm_ba_stream)."""
        s = ctypes.c_void_p()
        check(self._lib.sfm_ba_stream(self._h, ctypes.byref(s)))
        return s.value or 0

    def reduced_buffer(self):
        ptr = ctypes.c_void_p(); n = ctypes.c_int64(); ld = ctypes.c_int()
        check(self._lib.sfm_ba_reduced_buffer(self._h, ctypes.byref(ptr), ctypes.byref(n), ctypes.byref(ld)))
        return ptr.value, n.value, ld.value

    def bind_reduced_buffer(self, device_ptr, n_doubles):
        check(self._lib.sfm_ba_bind_reduced_buffer(self._h, ctypes.c_void_p(device_ptr), int(n_doubles)))

    def kernel_time(self, kernel_id):
        ms = ctypes.c_double(); n = ctypes.c_int()
        check(self._lib.sfm_ba_kernel_time(self._h, kernel_id, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def event_overhead(self, n=20):
        """Average hipEvent bracket (ms) around an empty kernel on this problem's stream (sfm_ba_event_overhead)."""
        ms = ctypes.c_double()
        check(self._lib.sfm_ba_event_overhead(self._h, int(n), ctypes.byref(ms)))
        return ms.value

    def reset_timing(self):
        check(self._lib.sfm_ba_reset_timing(self._h))

    def debug_stamps(self, n=1024):
        out = np.zeros(n, dtype=np.uint64)
        check(self._lib.sfm_ba_debug_stamps(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n))
        return out


# ---- descriptor matching (KeyTracker.__extend_list, key_tracker.py:213-317) ------------------------------------
class DescriptorSet:
    """Device-resident descriptor rows of one view (sfm_desc_create ... sfm_desc_destroy).

    ``metric`` is MATCH_L2 or MATCH_HAMMING; ``descriptors`` an (n, dim) array: uint8 (either metric) or float32 (L2),
    or ``None`` / no rows for an empty set.  Integer-valued L2 rows in [0, 255] take the exact bf16-MFMA path
    (``exact``)."""

    def __init__(self, metric, descriptors):
        self._lib = load()
        self._h = None
        d = np.zeros((0, 1), dtype=np.uint8) if descriptors is None else np.asarray(descriptors)
        if d.size == 0 and d.ndim != 2:
            d = d.reshape(0, 1)
        if d.ndim != 2:
            raise ValueError("descriptors must be (n, dim), got shape %s" % (d.shape,))
        if d.dtype == np.uint8:
            dtype = DESC_U8
        elif metric == MATCH_L2:
            d = d.astype(np.float32, copy=False); dtype = DESC_F32
        else:
            raise ValueError("Hamming matching needs uint8 descriptors, got %s" % d.dtype)
        d = np.ascontiguousarray(d)
        self.metric = int(metric)
        self.n, self.dim = int(d.shape[0]), int(d.shape[1])
        h = ctypes.c_void_p()
        check(self._lib.sfm_desc_create(self.metric, self.n, self.dim, dtype, d.ctypes.data_as(ctypes.c_void_p) if self.n else None,
                                        ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sfm_desc_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self, what):
        v = ctypes.c_int64()
        check(self._lib.sfm_desc_info(self._h, int(what), ctypes.byref(v)))
        return int(v.value)

    @property
    def exact(self):
        return bool(self.info(DESC_INFO_EXACT))

    @property
    def upload_bytes(self):
        return self.info(DESC_INFO_UPLOAD_BYTES)


def match(query, refs, mode=MATCH_KNN2):
    """Brute-force matching of ``query`` (a DescriptorSet) against every set of ``refs`` in one device call.

    Returns (best_idx, best_dist, second_idx, second_dist, mutual), each (len(refs), query.n): int32 / float32 /
    int32 / float32 / bool.  Order (distance, train index); a missing neighbour is index -1, distance inf; ``mutual``
    is only computed in MATCH_MUTUAL (all False otherwise)."""
    refs = list(refs)
    nr, nq = len(refs), query.n
    bi = np.empty((nr, nq), dtype=np.int32); si = np.empty((nr, nq), dtype=np.int32)
    bd = np.empty((nr, nq), dtype=np.float32); sd = np.empty((nr, nq), dtype=np.float32)
    mu = np.zeros((nr, nq), dtype=np.uint8)
    handles = (ctypes.c_void_p * max(nr, 1))(*[r._h for r in refs])
    check(load().sfm_match(query._h, nr, handles, int(mode), iptr(bi), bd.ctypes.data_as(fp), iptr(si), sd.ctypes.data_as(fp),
                           mu.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    return bi, bd, si, sd, mu.astype(bool)


def match_dev(query, refs, mode, d_best_idx, d_best_dist, d_second_idx, d_second_dist, d_mutual, stream=0):
    """Stream-ordered form of ``match``: outputs are device pointers (integers) of (len(refs), query.n) arrays."""
    refs = list(refs)
    handles = (ctypes.c_void_p * max(len(refs), 1))(*[r._h for r in refs])
    check(load().sfm_match_dev(query._h, len(refs), handles, int(mode), _vp(d_best_idx), _vp(d_best_dist), _vp(d_second_idx),
                               _vp(d_second_dist), _vp(d_mutual), _vp(stream)))


# ---- view pairs: which pairs of views to match (sfm_vocab_*, sfm_view_describe*, sfm_view_pairs*; no reference counterpart) ----
def _set_facts(s):
    """``(n, dim, metric, exact)`` of a DescriptorSet, or of a tuple that stands for one where there is no device."""
    if isinstance(s, (tuple, list)):
        n, dim, metric, exact = s
        return int(n), int(dim), int(metric), bool(exact)
    return int(s.n), int(s.dim), int(s.metric), bool(s.exact)


def _check_retrieve_sets(what, sets):
    sets = list(sets)
    if not 1 <= len(sets) <= RETRIEVE_MAX_VIEWS:
        raise ValueError("%d %ss (1 .. %d)" % (len(sets), what, RETRIEVE_MAX_VIEWS))
    dim0, total = None, 0
    for i, s in enumerate(sets):
        if s is None:
            raise ValueError("%s %d is null" % (what, i))
        n, dim, metric, exact = _set_facts(s)
        if metric != MATCH_L2 or not exact:
            raise ValueError("%s %d is not an exact L2 set (Hamming and non-integer float sets are not described)" % (what, i))
        dim0 = dim if dim0 is None else dim0
        if dim != dim0:
            raise ValueError("%s %d has dim %d, %s 0 has %d" % (what, i, dim, what, dim0))
        if n > RETRIEVE_MAX_VIEW_KEYS:
            raise ValueError("%s %d has %d keys (at most 2^22)" % (what, i, n))
        total += n
    return sets, dim0, total


def _check_retrieve_words(K, D):
    if not 1 <= K <= RETRIEVE_MAX_WORDS:
        raise ValueError("K = %d words (1 .. %d)" % (K, RETRIEVE_MAX_WORDS))
    if not 1 <= D <= RETRIEVE_MAX_DIM:
        raise ValueError("dim %d (1 .. %d)" % (D, RETRIEVE_MAX_DIM))
    if K * D > RETRIEVE_MAX_LEN:
        raise ValueError("K * D = %d exceeds %d" % (K * D, RETRIEVE_MAX_LEN))


def check_vocab_train(sets, K, iters=4, seed=1, train_cap=0):
    """The arguments of a ``vocab_train`` call, without a device: ``(sets, K, iters, seed, train_cap, D, N, T)`` converted or
    ValueError -- everything sfm_vocab_train refuses, in its order and with its messages.  A set is a DescriptorSet or, where
    there is no device, a tuple ``(n, dim, metric, exact)``; ``T`` is the number of training rows."""
    K, iters, train_cap = _integer("K", K), _integer("iters", iters), _integer("train_cap", train_cap)
    seed = _integer("seed", seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1, got %d" % seed)
    if not 1 <= K <= RETRIEVE_MAX_WORDS:
        raise ValueError("K = %d words (1 .. %d)" % (K, RETRIEVE_MAX_WORDS))
    if not 0 <= iters <= RETRIEVE_MAX_ITERS:
        raise ValueError("iters = %d (0 .. %d)" % (iters, RETRIEVE_MAX_ITERS))
    if not 0 <= train_cap <= RETRIEVE_CAP_MAX:
        raise ValueError("train_cap = %d (0 = 2^20, at most 2^22)" % train_cap)
    sets, D, N = _check_retrieve_sets("set", sets)
    _check_retrieve_words(K, D)
    T = min(N, train_cap if train_cap else RETRIEVE_CAP_DEFAULT)
    if T < K:
        raise ValueError("T = %d training rows for K = %d words" % (T, K))
    return sets, K, iters, seed, train_cap, D, N, T


def check_view_describe(vocab, views):
    """The arguments of a ``view_describe`` call, without a device: ``(views, K, D, N)`` or ValueError, as sfm_view_describe."""
    if vocab is None:
        raise ValueError("the vocabulary is null")
    _, D, K = _check_retrieve_sets("vocabulary", [vocab])
    _check_retrieve_words(K, D)
    views, Dv, N = _check_retrieve_sets("view", views)
    if Dv != D:
        raise ValueError("the views have dim %d, the vocabulary %d" % (Dv, D))
    if N >= 2 ** 31:
        raise ValueError("%d keys in all (fewer than 2^31)" % N)
    return views, K, D, N


def check_view_pairs(n_views, length, k=8, min_score=-np.inf, mutual=False, sequential=0, cap=0):
    """The scalar arguments of a ``view_pairs`` call, without a device: ``(V, len, k, min_score, mutual, sequential, cap)``
    converted or ValueError -- what sfm_view_pairs refuses, in its order and with its messages."""
    V, length, k, sequential, cap = (_integer("n_views", n_views), _integer("len", length), _integer("k", k),
                                     _integer("sequential", sequential), _integer("cap", cap))
    mutual = int(mutual) if isinstance(mutual, (bool, np.bool_)) else _integer("mutual", mutual)
    min_score = float(min_score)
    if not 1 <= V <= RETRIEVE_MAX_VIEWS:
        raise ValueError("V = %d views (1 .. %d)" % (V, RETRIEVE_MAX_VIEWS))
    if not 1 <= length <= RETRIEVE_MAX_LEN:
        raise ValueError("len = %d (1 .. %d)" % (length, RETRIEVE_MAX_LEN))
    if not 1 <= k <= RETRIEVE_MAX_K:
        raise ValueError("k = %d neighbours (1 .. %d)" % (k, RETRIEVE_MAX_K))
    if min_score != min_score:
        raise ValueError("min_score is NaN")
    if mutual not in (0, 1):
        raise ValueError("mutual = %d must be 0 or 1" % mutual)
    if sequential < 0:
        raise ValueError("sequential = %d must be >= 0" % sequential)
    if cap < 0:
        raise ValueError("cap = %d must be >= 0" % cap)
    if V * (2 * k + min(sequential, V)) >= 2 ** 31:
        raise ValueError("V (2 k + sequential) reaches 2^31 pairs")
    return V, length, k, min_score, mutual, min(sequential, 2 ** 31 - 1), cap


def _set_handles(sets):
    return (ctypes.c_void_p * max(len(sets), 1))(*[s._h for s in sets])


def view_score(dot, norm2_a, norm2_b):
    """``dot / sqrt(norm2_a * norm2_b)`` in the library's three fp64 operations (sfm_view_score; host only): the kernel's bits."""
    out = np.zeros(1)
    check(load().sfm_view_score(int(dot), int(norm2_a), int(norm2_b), dptr(out)))
    return float(out[0])


def vocab_init_rows(n_rows, K, seed=1, train_cap=0):
    """The rows of the concatenation of ``n_rows`` descriptors that ``vocab_train`` starts its ``K`` words from
    (sfm_vocab_init_rows; host only), int64 (K,)."""
    rows = np.zeros(max(int(K), 1), dtype=np.int64)
    check(load().sfm_vocab_init_rows(int(n_rows), int(K), ctypes.c_uint64(int(seed) % 2 ** 64), int(train_cap), _lptr(rows)))
    return rows[:int(K)]


def vocab_train(sets, K, iters=4, seed=1, train_cap=0):
    """A vocabulary of ``K`` words from resident exact L2 DescriptorSets by ``iters`` rounds of integer k-means
    (sfm_vocab_train).  Returns ``words`` uint8 (K, D) and ``log`` int64 (iters + 1, 3): inertia, words without a row, words
    changed, per round under the words it started with; the last row under the final words."""
    sets, K, iters, seed, train_cap, D, N, T = check_vocab_train(sets, K, iters, seed, train_cap)
    words = np.zeros((K, D), dtype=np.uint8)
    log = np.zeros((iters + 1, 3), dtype=np.int64)
    check(load().sfm_vocab_train(len(sets), _set_handles(sets), K, iters, ctypes.c_uint64(seed), train_cap, _u8ptr(words), _lptr(log)))
    return words, log


def view_describe(vocab, views, outputs=DESCRIBE_OUTPUTS):
    """One VLAD descriptor per view (sfm_view_describe): ``vocab`` a DescriptorSet of the K words, ``views`` DescriptorSets.
    Returns a dict of ``desc`` int8 (V, K * D), ``norm2`` int64 (V,), ``word_count`` int32 (V, K), ``assign`` int32 (keys of all
    views,), ``residual`` int32 (V, K * D); an output not named in ``outputs`` is not computed and comes back as None."""
    views, K, D, N = check_view_describe(vocab, views)
    unknown = set(outputs) - set(DESCRIBE_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (DESCRIBE_OUTPUTS, sorted(unknown)))
    V = len(views)
    o = {"desc": np.zeros((V, K * D), dtype=np.int8), "norm2": np.zeros(V, dtype=np.int64), "word_count": np.zeros((V, K), dtype=np.int32),
         "assign": np.zeros(N, dtype=np.int32), "residual": np.zeros((V, K * D), dtype=np.int32)}
    w = {name: (o[name] if name in outputs else None) for name in DESCRIBE_OUTPUTS}
    desc_p = w["desc"].ctypes.data_as(ctypes.POINTER(ctypes.c_int8)) if w["desc"] is not None else None
    check(load().sfm_view_describe(vocab._h, V, _set_handles(views), desc_p, _lptr(w["norm2"]), iptr(w["word_count"]), iptr(w["assign"]),
                                   iptr(w["residual"])))
    return w


def view_describe_dev(vocab, views, d_desc=0, d_norm2=0, d_word_count=0, d_assign=0, d_residual=0, stream=0):
    """``view_describe`` with the outputs as device pointers (0 = not wanted) and a caller's stream (sfm_view_describe_dev)."""
    views = list(views)
    check(load().sfm_view_describe_dev(vocab._h, len(views), _set_handles(views), _vp(d_desc), _vp(d_norm2), _vp(d_word_count),
                                       _vp(d_assign), _vp(d_residual), _vp(stream)))


def view_pairs(desc, norm2, k=8, min_score=-np.inf, mutual=False, sequential=0, cap=None, outputs=PAIRS_OUTPUTS[:5]):
    """The pairs of views to match (sfm_view_pairs): ``desc`` int8 (V, len), ``norm2`` int64 (V,).  Every view keeps its first
    ``k`` candidates by (score descending, index ascending); the pair a < b is listed iff one lists the other (``mutual``:
    both do) or ``b - a <= sequential``.  ``cap`` bounds the rows of ``pairs`` that are written (default: every pair that can
    be listed).  Returns a dict of ``nbr`` int32 (V, k), ``nbr_score`` (V, k), ``pairs`` int32 (min(n_pairs, cap), 2), ``how``
    int32, ``pair_score``, ``dot`` int32 (V, V) -- None where not in ``outputs`` -- and ``n_pairs``, the true count."""
    desc = np.ascontiguousarray(desc, dtype=np.int8)
    norm2 = np.ascontiguousarray(norm2, dtype=np.int64).reshape(-1)
    if desc.ndim != 2 or norm2.shape[0] != desc.shape[0]:
        raise ValueError("desc must be (V, len) and norm2 (V,), got %r and %r" % (desc.shape, norm2.shape))
    V, length = desc.shape
    if cap is None:
        cap = min(V * (V - 1) // 2, V * (2 * int(k) + min(int(sequential), V)))
    V, length, k, min_score, mutual, sequential, cap = check_view_pairs(V, length, k, min_score, mutual, sequential, cap)
    unknown = set(outputs) - set(PAIRS_OUTPUTS)
    if unknown:
        raise ValueError("outputs must be among %r, got %r" % (PAIRS_OUTPUTS, sorted(unknown)))
    o = {"nbr": np.zeros((V, k), dtype=np.int32), "nbr_score": np.zeros((V, k)), "pairs": np.zeros((cap, 2), dtype=np.int32),
         "how": np.zeros(cap, dtype=np.int32), "pair_score": np.zeros(cap), "dot": None}
    if "dot" in outputs:
        o["dot"] = np.zeros((V, V), dtype=np.int32)
    w = {name: (o[name] if name in outputs else None) for name in PAIRS_OUTPUTS}
    if w["pairs"] is None and (w["how"] is not None or w["pair_score"] is not None):
        raise ValueError("how and pair_score come with pairs")
    n_pairs = np.zeros(1, dtype=np.int64)
    check(load().sfm_view_pairs(V, length, desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), _lptr(norm2), k, min_score, mutual, sequential,
                                cap, iptr(w["nbr"]), dptr(w["nbr_score"]), iptr(w["pairs"]), iptr(w["how"]), dptr(w["pair_score"]),
                                iptr(w["dot"]), _lptr(n_pairs)))
    written = min(int(n_pairs[0]), cap)
    for name in ("pairs", "how", "pair_score"):
        if w[name] is not None:
            w[name] = w[name][:written].copy()
    w["n_pairs"] = int(n_pairs[0])
    return w


def view_pairs_dev(n_views, length, d_desc, d_norm2, k=8, min_score=-np.inf, mutual=False, sequential=0, cap=0, d_nbr=0, d_nbr_score=0,
                   d_pairs=0, d_how=0, d_pair_score=0, d_dot=0, stream=0):
    """``view_pairs`` with every array as a device pointer (0 = not wanted) and a caller's stream (sfm_view_pairs_dev).  Returns
    ``n_pairs``, the true count; the first ``min(n_pairs, cap)`` rows of ``d_pairs``, ``d_how``, ``d_pair_score`` are written."""
    n_pairs = np.zeros(1, dtype=np.int64)
    check(load().sfm_view_pairs_dev(int(n_views), int(length), _vp(d_desc), _vp(d_norm2), int(k), float(min_score), int(mutual),
                                    int(sequential), int(cap), _vp(d_nbr), _vp(d_nbr_score), _vp(d_pairs), _vp(d_how), _vp(d_pair_score),
                                    _vp(d_dot), _lptr(n_pairs), _vp(stream)))
    return int(n_pairs[0])


# ---- guided matching (sfm_match_guided*; no reference counterpart) ---------------------------------------------------
GUIDE_NAMES = {"none": GUIDE_NONE, "fundamental": GUIDE_FUNDAMENTAL, "homography": GUIDE_HOMOGRAPHY}
GUIDED_OUTPUTS = ("best_idx", "best_dist", "second_idx", "second_dist", "mutual", "n_admitted")
_GUIDED_DTYPES = (np.int32, np.float32, np.int32, np.float32, np.uint8, np.int32)


def homography_adjugate(H):
    """adj H by the cofactor formula of include/sfm_hip.h ('guided matching'), as a (3, 3) array; runs on the host."""
    H = f64(H).reshape(9)
    G = np.zeros(9)
    check(load().sfm_homography_adjugate(dptr(H), dptr(G)))
    return G.reshape(3, 3)


def check_guided(n_refs, kinds, models, max_err2):
    """The arguments of a guided match as the library takes them: ``(kind (n_refs,) int32, model (n_refs, 9) float64,
    max_err2)``.  ``kinds`` holds GUIDE_* values or their names; ``models`` one (3, 3) matrix per reference (``None`` for
    an ungated one).  ValueError for what the library would answer with SFM_E_SHAPE."""
    kinds, models = list(kinds), list(models)
    if len(kinds) != n_refs or len(models) != n_refs:
        raise ValueError("guided match: %d references, %d kinds, %d models" % (n_refs, len(kinds), len(models)))
    max_err2 = float(max_err2)
    if not max_err2 >= 0.0:
        raise ValueError("guided match: max_err2 must be >= 0, got %r" % max_err2)
    kind = np.zeros(max(n_refs, 1), dtype=np.int32)
    model = np.zeros((max(n_refs, 1), 9))
    for r in range(n_refs):
        k = GUIDE_NAMES.get(kinds[r], kinds[r]) if isinstance(kinds[r], str) else kinds[r]
        if k not in (GUIDE_NONE, GUIDE_FUNDAMENTAL, GUIDE_HOMOGRAPHY):
            raise ValueError("guided match: reference %d has the unknown gate %r" % (r, kinds[r]))
        kind[r] = k
        if k == GUIDE_NONE:
            continue
        m = np.asarray(models[r], dtype=np.float64)
        if m.size != 9 or not np.all(np.isfinite(m)):
            raise ValueError("guided match: the model of reference %d must be a finite 3x3 matrix" % r)
        model[r] = m.reshape(9)
    return kind, model, max_err2


def _key_xy(xy, n, who):
    xy = np.asarray(xy, dtype=np.float64)
    if xy.shape != (n, 2):
        raise ValueError("%s: key coordinates of shape %s for %d descriptors" % (who, xy.shape, n))
    return np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


def match_guided(query, query_xy, refs, ref_xy, kinds, models, max_err2, outputs=GUIDED_OUTPUTS):
    """``match`` with the candidates of every query restricted to the train keys its pair's model admits
    (sfm_match_guided; the rule is in include/sfm_hip.h, 'guided matching').

    ``query_xy`` is (query.n, 2); ``ref_xy[r]`` (refs[r].n, 2), or ``None`` for an ungated reference; ``kinds`` /
    ``models`` as ``check_guided`` takes them; the reference key is left, the query key right.  Returns a dict of the
    ``outputs`` asked for, each (len(refs), query.n): ``best_idx`` / ``second_idx`` int32, ``best_dist`` / ``second_dist``
    float32, ``mutual`` bool, ``n_admitted`` int32.  What is not asked for is not computed."""
    refs, ref_xy = list(refs), list(ref_xy)
    nr, nq = len(refs), query.n
    unknown = [o for o in outputs if o not in GUIDED_OUTPUTS]
    if unknown:
        raise ValueError("guided match: unknown outputs %s" % unknown)
    if len(ref_xy) != nr:
        raise ValueError("guided match: %d references, %d coordinate arrays" % (nr, len(ref_xy)))
    kind, model, max_err2 = check_guided(nr, kinds, models, max_err2)
    qx, qy = _key_xy(query_xy, nq, "guided match (query)")
    keep = [qx, qy]
    rx, ry = (_dp * max(nr, 1))(), (_dp * max(nr, 1))()
    for r in range(nr):
        if ref_xy[r] is None:
            if kind[r] != GUIDE_NONE:
                raise ValueError("guided match: reference %d has a gate and no coordinates" % r)
            continue
        x, y = _key_xy(ref_xy[r], refs[r].n, "guided match (reference %d)" % r)
        keep += [x, y]
        rx[r], ry[r] = dptr(x), dptr(y)
    out = {name: np.zeros((nr, nq), dtype=dt) for name, dt in zip(GUIDED_OUTPUTS, _GUIDED_DTYPES) if name in outputs}
    ptrs = [out[name].ctypes.data_as(vp) if name in out else None for name in GUIDED_OUTPUTS]
    handles = (vp * max(nr, 1))(*[r._h for r in refs])
    check(load().sfm_match_guided(query._h, dptr(qx), dptr(qy), nr, handles, ctypes.cast(rx, _pp), ctypes.cast(ry, _pp), iptr(kind),
                                  dptr(model), max_err2, *ptrs))
    if "mutual" in out:
        out["mutual"] = out["mutual"].astype(bool)
    return out


def match_guided_dev(query, d_query_xy, refs, d_ref_xy, kinds, models, max_err2, d_best_idx=0, d_best_dist=0, d_second_idx=0,
                     d_second_dist=0, d_mutual=0, d_n_admitted=0, stream=0):
    """Stream-ordered form of ``match_guided``: ``d_query_xy`` = (d_x, d_y) and ``d_ref_xy[r]`` = (d_x, d_y) or ``None``
    are device pointers (integers) of float64 arrays, the outputs device pointers of (len(refs), query.n) arrays; 0 = not
    wanted."""
    refs, d_ref_xy = list(refs), list(d_ref_xy)
    nr = len(refs)
    if len(d_ref_xy) != nr:
        raise ValueError("guided match: %d references, %d coordinate arrays" % (nr, len(d_ref_xy)))
    kind, model, max_err2 = check_guided(nr, kinds, models, max_err2)
    rx, ry = (vp * max(nr, 1))(), (vp * max(nr, 1))()
    for r in range(nr):
        if d_ref_xy[r] is not None:
            rx[r], ry[r] = int(d_ref_xy[r][0]), int(d_ref_xy[r][1])
    handles = (vp * max(nr, 1))(*[r._h for r in refs])
    check(load().sfm_match_guided_dev(query._h, _vp(d_query_xy[0]), _vp(d_query_xy[1]), nr, handles, rx, ry, iptr(kind), dptr(model),
                                      max_err2, _vp(d_best_idx), _vp(d_best_dist), _vp(d_second_idx), _vp(d_second_dist),
                                      _vp(d_mutual), _vp(d_n_admitted), _vp(stream)))


# ---- SIFT detection (ViewProcessor.__extract_keys, view_processor.py:199-202) ------------------------------------
def _sift_image(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.size == 0 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("SIFT input must be a non-empty (H, W) or (H, W, 3) uint8 image, got %s %s" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


class SiftResult:
    """One sfm_sift_detect result (a context manager).  ``arrays()`` gives the keypoints and descriptors; the
    debug reads (``level``, ``pre``) need ``keep_pyramid=True`` for the pyramid levels."""

    def __init__(self, img, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6,
                 keep_pyramid=False, stream=0):
        self._lib = load()
        self._h = None
        a = _sift_image(img)
        prm = SiftParams(int(n_octave_layers), float(contrast_threshold), float(edge_threshold), float(sigma),
                         int(bool(keep_pyramid)), ctypes.c_void_p(stream) if stream else None)
        h = ctypes.c_void_p()
        ch = 1 if a.ndim == 2 else 3
        check(self._lib.sfm_sift_detect(a.ctypes.data_as(ctypes.c_void_p), a.shape[0], a.shape[1], ch, a.strides[0],
                                        ctypes.byref(prm), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sfm_sift_result_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self, what):
        v = ctypes.c_int64()
        check(self._lib.sfm_sift_result_info(self._h, int(what), ctypes.byref(v)))
        return int(v.value)

    @property
    def n(self):
        return self.info(SIFT_INFO_N)

    @property
    def n_octaves(self):
        return self.info(SIFT_INFO_N_OCTAVES)

    @property
    def n_layers(self):
        return self.info(SIFT_INFO_N_LAYERS)

    def level_shape(self, octave):
        h, w = ctypes.c_int(), ctypes.c_int()
        check(self._lib.sfm_sift_result_level_shape(self._h, int(octave), ctypes.byref(h), ctypes.byref(w)))
        return h.value, w.value

    def arrays(self):
        """dict of x, y, size, angle, response (float32), octave (int32) and descriptors ((n, 128) float32)."""
        n = self.n
        out = {k: np.zeros(n, dtype=np.float32) for k in ("x", "y", "size", "angle", "response")}
        out["octave"] = np.zeros(n, dtype=np.int32)
        out["descriptors"] = np.zeros((n, 128), dtype=np.float32)
        check(self._lib.sfm_sift_result_copy(self._h, *[out[k].ctypes.data_as(fp) for k in ("x", "y", "size", "angle", "response")],
                                              iptr(out["octave"]), out["descriptors"].ctypes.data_as(fp)))
        return out

    def pre(self):
        """The refined keypoints before orientation (pyramid coordinates, octave field before the fixup)."""
        n = self.info(SIFT_INFO_N_PRE)
        out = {k: np.zeros(n, dtype=np.float32) for k in ("x", "y", "size", "response")}
        out["octave"] = np.zeros(n, dtype=np.int32)
        check(self._lib.sfm_sift_result_copy_pre(self._h, *[out[k].ctypes.data_as(fp) for k in ("x", "y", "size", "response")],
                                                 iptr(out["octave"])))
        return out

    def level(self, kind, octave, level):
        """One Gaussian (kind SIFT_LEVEL_GAUSS) or DoG (SIFT_LEVEL_DOG) level as an (h, w) float32 array."""
        h, w = self.level_shape(octave)
        out = np.zeros((h, w), dtype=np.float32)
        check(self._lib.sfm_sift_result_copy_level(self._h, int(kind), int(octave), int(level),
                                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out


def sift_detect(img, **params):
    """detectAndCompute(img, None) on the GPU: a dict of x, y, size, angle, response, octave and (n, 128) float32
    descriptors, in the contract's order (INTEGRATION.md 'SIFT detection').  ``params``: n_octave_layers,
    contrast_threshold, edge_threshold, sigma, stream."""
    with SiftResult(img, **params) as r:
        return r.arrays()


def sift_blur_kernel(sigma):
    """The float32 Gaussian weights the library blurs with for ``sigma``."""
    lib = load()
    k = ctypes.c_int()
    check(lib.sfm_sift_blur_kernel(float(sigma), 0, None, ctypes.byref(k)))
    w = np.zeros(k.value, dtype=np.float32)
    check(lib.sfm_sift_blur_kernel(float(sigma), k.value, w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(k)))
    return w


# ---- device-resident key tracks (KeyTrack / KeyTracker, key_tracker.py:14-59, 132-181, 213-317) -------------------
class TrackStore:
    """The key coordinates and ``KeyTrack.table`` of every view of one KeyTracker on the device (sfm_track_create ...
    sfm_track_destroy).  Tables come back as int32 arrays, -1 = invalid match / not used.  ``upload_bytes`` and
    ``download_bytes`` count the traffic of the store itself (descriptors are counted by their ``DescriptorSet``)."""

    def __init__(self):
        self._lib = load()
        self._h = None
        h = ctypes.c_void_p()
        check(self._lib.sfm_track_create(ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sfm_track_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self, what, view=0):
        v = ctypes.c_int64()
        check(self._lib.sfm_track_info(self._h, int(what), int(view), ctypes.byref(v)))
        return int(v.value)

    @property
    def n_views(self):
        return self.info(TRACK_INFO_N_VIEWS)

    def n_keys(self, view):
        return self.info(TRACK_INFO_N_KEYS, view)

    def n_rows(self, view):
        return self.info(TRACK_INFO_N_ROWS, view)

    @property
    def upload_bytes(self):
        return self.info(TRACK_INFO_UPLOAD_BYTES)

    @property
    def download_bytes(self):
        return self.info(TRACK_INFO_DOWNLOAD_BYTES)

    def add_view(self, xy):
        """Add a view whose keys sit at the rows of ``xy`` ((n, 2)); returns its index."""
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
        out = ctypes.c_int()
        check(self._lib.sfm_track_add_view(self._h, xy.shape[0], dptr(x), dptr(y), ctypes.byref(out)))
        return out.value

    def drop_last_view(self):
        check(self._lib.sfm_track_drop_last_view(self._h))

    def match_dedup_dev(self, new_view, n_refs, mode, d_best_idx, d_best_dist, d_second_idx, d_second_dist, d_mutual, stream=0):
        """Filter + duplicate removal from DEVICE neighbour arrays ((n_refs, n_query), pointers as integers)."""
        check(self._lib.sfm_track_match_dedup_dev(self._h, int(new_view), int(n_refs), int(mode), _vp(d_best_idx), _vp(d_best_dist),
                                                  _vp(d_second_idx), _vp(d_second_dist), _vp(d_mutual), _vp(stream)))

    def extend_dev(self, new_view, n_refs, mode, d_best_idx, d_best_dist, d_second_idx, d_second_dist, d_mutual, stream=0):
        """Filter + duplicate removal + table writes in one call."""
        check(self._lib.sfm_track_extend_dev(self._h, int(new_view), int(n_refs), int(mode), _vp(d_best_idx), _vp(d_best_dist),
                                             _vp(d_second_idx), _vp(d_second_dist), _vp(d_mutual), _vp(stream)))

    def match_views(self, new_view, query, refs, mode, write=True, stream=0):
        """``sfm_match_dev`` of ``query`` against ``refs`` (DescriptorSets of the views 0 .. len(refs)-1) into the store's
        own buffers, then the extend (``write``) or only filter + duplicate removal."""
        refs = list(refs)
        handles = (ctypes.c_void_p * max(len(refs), 1))(*[r._h for r in refs])
        check(self._lib.sfm_track_match_views(self._h, int(new_view), query._h, len(refs), handles, int(mode), int(bool(write)),
                                              _vp(stream)))

    def extend_status(self, n_refs):
        """(status, first offending query, kept length) per reference view of the last extend, as int32 arrays."""
        st, bad, kept = (np.zeros(max(n_refs, 1), dtype=np.int32) for _ in range(3))
        check(self._lib.sfm_track_extend_status(self._h, int(n_refs), iptr(st), iptr(bad), iptr(kept)))
        return st[:n_refs], bad[:n_refs], kept[:n_refs]

    def kept(self, ref, n_kept):
        """The kept (query, train) lists of reference view ``ref`` (``n_kept`` from ``extend_status``)."""
        q, t = np.zeros(max(n_kept, 1), dtype=np.int32), np.zeros(max(n_kept, 1), dtype=np.int32)
        check(self._lib.sfm_track_kept_copy(self._h, int(ref), iptr(q), iptr(t)))
        return q[:n_kept], t[:n_kept]

    def write_kept(self, ref, n=-1, stream=0):
        check(self._lib.sfm_track_write_kept(self._h, int(ref), int(n), _vp(stream)))

    def pairs(self, ref, que):
        """generate_matched_pairs: (r_idx (n,), q_idx (n,), ref_pts (3, n), que_pts (3, n))."""
        cap = max(self.n_keys(ref), 1)
        n = ctypes.c_int()
        r, q = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        rp, qp = np.zeros(3 * cap), np.zeros(3 * cap)
        check(self._lib.sfm_track_pairs(self._h, int(ref), int(que), ctypes.byref(n), iptr(r), iptr(q), dptr(rp), dptr(qp)))
        n = n.value
        return r[:n], q[:n], rp[:3 * n].reshape(3, n), qp[:3 * n].reshape(3, n)

    def verify_pairs(self, ref, que, max_err2, max_hyp=0, iters=2):
        """The pairs of ``pairs(ref, que)`` verified on the device (sfm_twoview_verify_pairs): ``(r_idx (n,), q_idx (n,),
        inlier (n,) uint8, F (3, 3), best_hyp, status)``; the coordinates are not downloaded."""
        max_err2, max_hyp, iters = check_twoview(max_err2, max_hyp, iters)
        cap = max(self.n_keys(ref), 1)
        n, best, status = ctypes.c_int(), ctypes.c_int(-1), ctypes.c_int(0)
        r, q, inl = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint8)
        F = np.zeros((3, 3))
        check(self._lib.sfm_twoview_verify_pairs(self._h, int(ref), int(que), max_err2, max_hyp, iters, ctypes.byref(n), iptr(r),
                                               iptr(q), _u8ptr(inl), dptr(F), ctypes.byref(best), ctypes.byref(status)))
        n = n.value
        return r[:n], q[:n], inl[:n], F, int(best.value), int(status.value)

    def pose_pairs(self, ref, que, model, kind, K_left, K_right, cos2_min, min_parallax=1, inlier=None):
        """The pairs of ``pairs(ref, que)`` posed on the device as one set (sfm_twoview_pose_pairs): a dict with ``r_idx``,
        ``q_idx`` (n,), and ``R``, ``t``, ``normal``, ``cand_front``, ``n_front``, ``n_parallax``, ``best_cand``, ``status``,
        ``obs_front`` (n,), ``X`` (3, n) of ``twoview_pose`` for that set.  ``inlier`` (n,) is the optional mask of the matches
        that vote; the coordinates are not downloaded and nothing goes up but the model, the intrinsics and that mask."""
        model, kind, kl, kr, cos2_min, min_parallax = check_pose(1, [model], [kind], K_left, K_right, cos2_min, min_parallax)
        cap = max(self.n_keys(ref), 1)
        if inlier is not None:
            inlier = np.ascontiguousarray(np.asarray(inlier) != 0, dtype=np.uint8).reshape(-1)
            if inlier.shape[0] > cap:
                raise ValueError("pose_pairs: %d mask entries for at most %d pairs" % (inlier.shape[0], cap))
            inlier = np.concatenate((inlier, np.zeros(cap - inlier.shape[0], dtype=np.uint8)))
        n = ctypes.c_int()
        ints = {name: ctypes.c_int(0) for name in ("n_front", "n_parallax", "best_cand", "status")}
        r, q, front = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint8)
        R, t, normal, cand, X = np.zeros((3, 3)), np.zeros(3), np.zeros(3), np.zeros(4, dtype=np.int32), np.zeros(3 * cap)
        check(self._lib.sfm_twoview_pose_pairs(self._h, int(ref), int(que), _u8ptr(inlier), dptr(model), int(kind[0]), dptr(kl), dptr(kr),
                                               cos2_min, min_parallax, ctypes.byref(n), iptr(r), iptr(q), dptr(R), dptr(t),
                                               dptr(normal), iptr(cand), ctypes.byref(ints["n_front"]),
                                               ctypes.byref(ints["n_parallax"]), ctypes.byref(ints["best_cand"]),
                                               ctypes.byref(ints["status"]), _u8ptr(front), dptr(X)))
        n = n.value
        out = {"r_idx": r[:n], "q_idx": q[:n], "R": R, "t": t, "normal": normal, "cand_front": cand, "obs_front": front[:n],
               "X": X[:3 * n].reshape(3, n)}
        out.update({name: int(v.value) for name, v in ints.items()})
        return out

    def refine_pairs(self, ref, que, R_in, t_in, K_left, K_right, lam=0.0, iters=6, max_err2=4.0, cos2_min=1.0, inlier=None):
        """The pairs of ``pairs(ref, que)`` and the refinement of their pose on the device as one set
        (sfm_twoview_refine_pairs): a dict with ``r_idx``, ``q_idx`` (n,), and ``R``, ``t``, ``F``, ``cost`` (2,), ``info`` (15,),
        ``n_used``, ``status``, ``obs_res``, ``obs_inlier``, ``obs_front`` (n,), ``X`` (3, n), ``n_inliers``, ``n_front``,
        ``n_parallax`` of ``twoview_refine`` for that set.  ``inlier`` (n,) is the optional mask of the matches that count; the
        coordinates are not downloaded and nothing goes up but the pose, the intrinsics and that mask."""
        R, t, kl, kr, lam, iters, max_err2, cos2_min = check_refine(1, [R_in], [t_in], K_left, K_right, lam, iters, max_err2, cos2_min)
        cap = max(self.n_keys(ref), 1)
        if inlier is not None:
            inlier = np.ascontiguousarray(np.asarray(inlier) != 0, dtype=np.uint8).reshape(-1)
            if inlier.shape[0] > cap:
                raise ValueError("refine_pairs: %d mask entries for at most %d pairs" % (inlier.shape[0], cap))
            inlier = np.concatenate((inlier, np.zeros(cap - inlier.shape[0], dtype=np.uint8)))
        n = ctypes.c_int()
        ints = {name: ctypes.c_int(0) for name in ("n_used", "status", "n_inliers", "n_front", "n_parallax")}
        r, q = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        inl, front, res = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8), np.zeros(cap)
        Ro, to, F, cost, info, X = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3)), np.zeros(2), np.zeros(15), np.zeros(3 * cap)
        check(self._lib.sfm_twoview_refine_pairs(self._h, int(ref), int(que), _u8ptr(inlier), dptr(R), dptr(t), dptr(kl), dptr(kr), lam, iters,
                                                 max_err2, cos2_min, ctypes.byref(n), iptr(r), iptr(q), dptr(Ro), dptr(to), dptr(F),
                                                 dptr(cost), dptr(info), ctypes.byref(ints["n_used"]), ctypes.byref(ints["status"]),
                                                 dptr(res), _u8ptr(inl), _u8ptr(front), dptr(X), ctypes.byref(ints["n_inliers"]),
                                                 ctypes.byref(ints["n_front"]), ctypes.byref(ints["n_parallax"])))
        n = n.value
        out = {"r_idx": r[:n], "q_idx": q[:n], "R": Ro, "t": to, "F": F, "cost": cost, "info": info, "obs_res": res[:n],
               "obs_inlier": inl[:n], "obs_front": front[:n], "X": X[:3 * n].reshape(3, n)}
        out.update({name: int(v.value) for name, v in ints.items()})
        return out

    def match_guided(self, que_view, query, ref_views, refs, kinds, models, max_err2, d_best_idx=0, d_best_dist=0, d_second_idx=0,
                     d_second_dist=0, d_mutual=0, d_n_admitted=0, stream=0):
        """``match_guided_dev`` with the key coordinates the store holds (sfm_match_guided_track): ``query`` is the
        DescriptorSet of view ``que_view``, ``refs[r]`` that of view ``ref_views[r]``; nothing is uploaded.  Outputs are
        device pointers (integers) of (len(refs), query.n) arrays, 0 = not wanted."""
        refs = list(refs)
        views = i32(ref_views).reshape(-1)
        if views.shape[0] != len(refs):
            raise ValueError("guided match: %d reference views, %d descriptor sets" % (views.shape[0], len(refs)))
        kind, model, max_err2 = check_guided(len(refs), kinds, models, max_err2)
        handles = (vp * max(len(refs), 1))(*[r._h for r in refs])
        check(self._lib.sfm_match_guided_track(self._h, int(que_view), query._h, len(refs), iptr(views), handles, iptr(kind),
                                               dptr(model), max_err2, _vp(d_best_idx), _vp(d_best_dist), _vp(d_second_idx),
                                               _vp(d_second_dist), _vp(d_mutual), _vp(d_n_admitted), _vp(stream)))

    def set_pairs(self, ref, que, r_idx, q_idx):
        """Replace the matches between the views ``ref`` and ``que`` by the pairs (r_idx[k], q_idx[k])
        (sfm_match_guided_set_pairs); a bad or repeated index raises ValueError and writes nothing."""
        r_idx, q_idx = i32(r_idx).reshape(-1), i32(q_idx).reshape(-1)
        if r_idx.shape != q_idx.shape:
            raise ValueError("set_pairs: %d reference keys, %d query keys" % (r_idx.shape[0], q_idx.shape[0]))
        check(self._lib.sfm_match_guided_set_pairs(self._h, int(ref), int(que), r_idx.shape[0], iptr(r_idx), iptr(q_idx)))

    def pairs_dev(self, ref, que, d_count, d_r_idx, d_q_idx, d_ref_pts, d_que_pts, stream=0):
        check(self._lib.sfm_track_pairs_dev(self._h, int(ref), int(que), _vp(d_count), _vp(d_r_idx), _vp(d_q_idx), _vp(d_ref_pts),
                                            _vp(d_que_pts), _vp(stream)))

    def update_usage(self, view, keys, tri):
        keys, tri = i32(keys).reshape(-1), i32(tri).reshape(-1)
        if keys.shape != tri.shape:
            raise ValueError("update_usage: %d keys, %d point indices" % (keys.shape[0], tri.shape[0]))
        check(self._lib.sfm_track_update_usage(self._h, int(view), keys.shape[0], iptr(keys), iptr(tri)))

    def constructed(self, view):
        cap = max(self.n_keys(view), 1)
        n = ctypes.c_int()
        k, t = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        check(self._lib.sfm_track_constructed(self._h, int(view), ctypes.byref(n), iptr(k), iptr(t)))
        return k[:n.value], t[:n.value]

    def unconstructed(self, view):
        cap = max(self.n_keys(view), 1)
        n = ctypes.c_int()
        k = np.zeros(cap, dtype=np.int32)
        check(self._lib.sfm_track_unconstructed(self._h, int(view), ctypes.byref(n), iptr(k)))
        return k[:n.value]

    def table(self, view):
        out = np.zeros((self.n_rows(view), self.n_keys(view)), dtype=np.int32)
        check(self._lib.sfm_track_copy_table(self._h, int(view), iptr(out) if out.size else None))
        return out

    def row(self, view, row):
        out = np.zeros(self.n_keys(view), dtype=np.int32)
        check(self._lib.sfm_track_copy_row(self._h, int(view), int(row), iptr(out) if out.size else None))
        return out

    def set_normalised(self, view, uv):
        """The normalised coordinates ((2, n): ``geometry.normalise_pixels`` of ALL keys) the observation list gathers
        from (sfm_obs_set_normalised); again whenever the view's intrinsic matrix changes."""
        uv = np.asarray(uv, dtype=np.float64).reshape(2, -1)
        u, v = np.ascontiguousarray(uv[0]), np.ascontiguousarray(uv[1])
        check(self._lib.sfm_obs_set_normalised(self._h, int(view), u.shape[0], dptr(u) if u.size else None, dptr(v) if v.size else None))

    def build_observations(self, n_views, n_pts):
        """Build the bundle adjustment's observation list of the first ``n_views`` views and ``n_pts`` points on the device
        (sfm_obs_build: ``observations.build_observations`` of the views' own rows); returns M."""
        m = ctypes.c_int64()
        check(self._lib.sfm_obs_build(self._h, int(n_views), int(n_pts), ctypes.byref(m)))
        return int(m.value)

    def link(self, pairs, key_mask=None, min_len=2, d_key_track=0):
        """Link the matches of ``pairs`` ((P, 2) of (ref, que): the entries ``table[ref][que, r] > 0``, read where they lie) into
        multi-view tracks and make them the store's observation list (sfm_link_tracks_views).  ``key_mask``: one byte per key
        of each pair's reference view, concatenated in pair order (a match is used iff the byte of its reference key is
        non-zero) -- the only upload.  ``d_key_track``: a device pointer for the per-key verdicts (all keys of the store), or 0.
        Returns ``summary (8,) int64`` in the order of ``LINK_SUMMARY``; ``observations()`` and ``BaProblem.from_tracks`` then
        see the tracks."""
        pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
        if key_mask is not None:
            key_mask = np.ascontiguousarray(np.asarray(key_mask).reshape(-1) != 0, dtype=np.uint8)
            want = sum(self.n_keys(int(r)) for r in pairs[:, 0] if 0 <= r < self.n_views)
            if key_mask.size != want:
                raise ValueError("link: key_mask holds %d bytes, the reference views of the pairs %d keys" % (key_mask.size, want))
        summary = np.zeros(8, dtype=np.int64)
        check(self._lib.sfm_link_tracks_views(self._h, pairs.shape[0], iptr(pairs), _u8ptr(key_mask), int(min_len), _vp(d_key_track),
                                             _lptr(summary)))
        return summary

    def observations(self):
        """(pt_ptr (N+1,), cam_idx (M,), key_idx (M,), uv (2, M)) of the last ``build_observations`` or ``link``."""
        n, m = self.info(TRACK_INFO_OBS_PTS), self.info(TRACK_INFO_N_OBS)
        pt_ptr, cam, key = np.zeros(n + 1, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        uv = np.zeros((2, m))
        check(self._lib.sfm_obs_copy(self._h, iptr(pt_ptr), iptr(cam) if m else None, iptr(key) if m else None,
                                                    dptr(uv) if m else None))
        return pt_ptr, cam, key, uv
