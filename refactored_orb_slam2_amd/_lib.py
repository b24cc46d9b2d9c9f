"""ctypes loader of the in-tree liborbfe.so (HIP, gfx950).  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "liborbfe.so")

OK, ERR_INVALID, ERR_CAPACITY, ERR_NO_DEVICE, ERR_HIP, ERR_EMPTY = 0, -1, -2, -3, -4, -5
MAX_LEVELS = 16
STAGES = ("pyramid", "fast", "octree", "blur", "describe")

KP_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")]
)
QUERY_DTYPE = np.dtype(
    [("u", "<f4"), ("v", "<f4"), ("u_r", "<f4"), ("radius", "<f4"), ("min_level", "<i4"),
     ("max_level", "<i4"), ("valid", "<i4"), ("blocks", "<i4"), ("angle", "<f4"), ("desc", "u1", (32,))]
)
CAND_DTYPE = np.dtype([("idx", "<i4"), ("dist", "<i4")])
# orbfe_frustum / orbfe_map_point / orbfe_track (include/orbfe.h)
FRUSTUM_DTYPE = np.dtype(
    [("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
     ("cy", "<f4"), ("mbf", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"),
     ("log_scale_factor", "<f4"), ("n_levels", "<i4"), ("scale_factors", "<f4", (16,))]
)
MAP_POINT_DTYPE = np.dtype(
    [("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("skip", "<i4"),
     ("observed", "<i4"), ("desc", "u1", (32,))]
)
TRACK_DTYPE = np.dtype(
    [("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("level", "<i4"), ("view_cos", "<f4")]
)
EPIPOLAR_DTYPE = np.dtype([("F12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4"), ("scale_factors", "<f4", (16,)), ("level_sigma2", "<f4", (16,))])
UNPROJECT_CAM_DTYPE = np.dtype([("Rwc", "<f4", (9,)), ("Ow", "<f4", (3,)), ("cx", "<f4"), ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4")])
LAST_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("valid", "<i4"), ("observed", "<i4"), ("octave", "<i4"), ("angle", "<f4"), ("desc", "u1", (32,))])
TRACK_POSE_DTYPE = np.dtype(
    [("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"),
     ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"), ("forward", "<i4"), ("backward", "<i4"),
     ("th", "<f4"), ("scale_factors", "<f4", (16,))]
)
assert UNPROJECT_CAM_DTYPE.itemsize == 64 and LAST_POINT_DTYPE.itemsize == 60 and TRACK_POSE_DTYPE.itemsize == 160
assert FRUSTUM_DTYPE.itemsize == 168 and MAP_POINT_DTYPE.itemsize == 72 and TRACK_DTYPE.itemsize == 24
BF_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i4"), ("second_dist", "<i4")])
# orbfe_kf_camera / orbfe_kf_point / orbfe_kf_result: the whole-function keyframe-rate searches (orbfe_kf_search)
KF_CAMERA_DTYPE = np.dtype(
    [("R", "<f4", (9,)), ("t", "<f4", (3,)), ("R2", "<f4", (9,)), ("t2", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"),
     ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"),
     ("log_scale_factor", "<f4"), ("n_levels", "<i4"), ("th", "<f4"), ("scale_factors", "<f4", (16,))]
)
KF_POINT_DTYPE = np.dtype(
    [("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("skip", "<i4"),
     ("angle", "<f4"), ("desc", "u1", (32,))]
)
KF_RESULT_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i4"), ("level", "<i4"), ("u", "<f4"), ("v", "<f4"), ("u_r", "<f4")])
assert KF_CAMERA_DTYPE.itemsize == 220 and KF_POINT_DTYPE.itemsize == 72 and KF_RESULT_DTYPE.itemsize == 24
KF_FUSE, KF_FUSE_SIM3, KF_SIM3, KF_LOOP, KF_RELOC = 1, 2, 3, 4, 5


class OrbfeError(RuntimeError):
    def __init__(self, code: int, where: str, text: str):
        super().__init__(f"{where} failed with code {code}: {text}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class FeatVecNode(C.Structure):
    _fields_ = [("node_id", C.c_int32), ("start", C.c_int32), ("count", C.c_int32)]


class Calibration(C.Structure):
    """orbfe_calibration (include/orbfe.h): mK, mDistCoef, mbf, mDepthMapFactor; 48 bytes"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float),
                ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float), ("mbf", C.c_float), ("depth_factor", C.c_float),
                ("reserved", C.c_int32)]


class VocabTrainConfig(C.Structure):
    """orbfe_vocab_train_config (include/orbfe.h); 32 bytes"""
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("seed", C.c_uint64),
                ("max_iterations", C.c_int32), ("wide_min", C.c_int32)]


# orbfe_vocab_train_stats (include/orbfe.h)
VOCAB_TRAIN_STATS_DTYPE = np.dtype([("n_nodes", "<i4"), ("n_words", "<i4"), ("n_kmeans_nodes", "<i4"), ("n_trivial_nodes", "<i4"),
                                    ("n_short_seedings", "<i4"), ("n_empty_clusters", "<i4"), ("n_capped_nodes", "<i4"),
                                    ("max_rounds", "<i4"), ("nodes_per_level", "<i4", (11,))])
assert C.sizeof(VocabTrainConfig) == 32 and VOCAB_TRAIN_STATS_DTYPE.itemsize == 76
VOCAB_TRAIN_MAX_ITERATIONS = 1000
VOCAB_TRAIN_CHUNK = 1024   # positions per workgroup of the wide form; the most the narrow form holds (csrc/vocab_train_internal.h)

DEPTH_NONE, DEPTH_U16, DEPTH_F32 = 0, 1, 2
# orbfe_pose_camera / orbfe_pose_result (Optimizer::PoseOptimization, include/orbfe.h)
POSE_CAMERA_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("n_levels", "<i4"),
                              ("inv_level_sigma2", "<f4", (16,))])
POSE_RESULT_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("n_initial", "<i4"), ("n_bad", "<i4"), ("n_inliers", "<i4"), ("rounds", "<i4"),
                              ("iterations", "<i4")])
assert POSE_CAMERA_DTYPE.itemsize == 88 and POSE_RESULT_DTYPE.itemsize == 68
POSE_DISCARD = 1
POSE_MAX_ROWS = 9500
# orbfe_tri_view / orbfe_new_point / orbfe_tri_neighbor (LocalMapping::CreateNewMapPoints, include/orbfe.h)
TRI_VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                           ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"), ("n_levels", "<i4"),
                           ("scale_factors", "<f4", (16,)), ("level_sigma2", "<f4", (16,))])
NEW_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                            ("idx2", "<i4"), ("code", "<i4"), ("path", "<i4")])
TRI_NEIGHBOR_DTYPE = np.dtype([("keys", "<u8"), ("desc", "<u8"), ("u_right", "<u8"), ("depth", "<u8"), ("has_mp", "<u8"), ("nodes", "<u8"),
                               ("idx", "<u8"), ("n", "<i4"), ("n_nodes", "<i4"), ("view", TRI_VIEW_DTYPE), ("ep", EPIPOLAR_DTYPE),
                               ("median_depth", "<f4")])
assert TRI_VIEW_DTYPE.itemsize == 224 and NEW_POINT_DTYPE.itemsize == 44 and TRI_NEIGHBOR_DTYPE.itemsize == 464
(TRI_OK, TRI_NO_MATCH, TRI_W_ZERO, TRI_LOW_PARALLAX, TRI_BEHIND1, TRI_BEHIND2, TRI_REPROJ1, TRI_REPROJ2, TRI_DIST_ZERO,
 TRI_SCALE) = range(10)
TRI_PATH_NONE, TRI_PATH_LINEAR, TRI_PATH_UNPROJECT1, TRI_PATH_UNPROJECT2 = range(4)
TRI_MAX_ROWS = 65535
# orbfe_sim3_view / orbfe_sim3_pair / orbfe_sim3_hypothesis / orbfe_sim3_result (Sim3Solver, include/orbfe.h)
SIM3_VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
SIM3_PAIR_DTYPE = np.dtype([("Xw1", "<f4", (3,)), ("Xw2", "<f4", (3,)), ("max_err1", "<f4"), ("max_err2", "<f4")])
SIM3_HYPOTHESIS_DTYPE = np.dtype([("s", "<f4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("n_inliers", "<i4"), ("reserved", "<i4", (2,))])
SIM3_RESULT_DTYPE = np.dtype([("returned", "<i4"), ("n_inliers", "<i4"), ("best", "<i4"), ("best_inliers", "<i4"), ("T12", "<f4", (12,)),
                              ("s", "<f4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("reserved", "<i4", (3,))])
assert SIM3_VIEW_DTYPE.itemsize == 64 and SIM3_PAIR_DTYPE.itemsize == 32 and SIM3_HYPOTHESIS_DTYPE.itemsize == 64
assert SIM3_RESULT_DTYPE.itemsize == 128
SIM3_MAX_PAIRS, SIM3_MAX_HYPOTHESES, SIM3_MAX_PROBLEMS = 1024, 4096, 65535
SIM3_WAVES = 4   # hypotheses per workgroup of sim3_hypotheses_kernel (csrc/sim3_internal.h)
# orbfe_pnp_point / orbfe_pnp_camera / orbfe_pnp_hypothesis / orbfe_pnp_refine / orbfe_pnp_result / orbfe_pnp_diag (PnPsolver, include/orbfe.h)
PNP_POINT_DTYPE = np.dtype([("Xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("max_err", "<f4")])
PNP_CAMERA_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
PNP_HYPOTHESIS_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_inliers", "<i4"), ("winner", "<i4"), ("refine", "<i4"),
                                 ("reserved", "<i4")])
PNP_REFINE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_inliers", "<i4"), ("success", "<i4"), ("winner", "<i4"),
                             ("n_used", "<i4")])
PNP_RESULT_DTYPE = np.dtype([("returned", "<i4"), ("refined", "<i4"), ("n_inliers", "<i4"), ("best", "<i4"), ("best_inliers", "<i4"),
                             ("reserved", "<i4", (3,)), ("Tcw", "<f4", (12,))])
PNP_DIAG_DTYPE = np.dtype([("cws", "<f8", (12,)), ("V", "<f8", (48,)), ("eig", "<f8", (5,)), ("betas", "<f8", (12,)),
                           ("rep_errors", "<f8", (3,))])
assert PNP_POINT_DTYPE.itemsize == 24 and PNP_CAMERA_DTYPE.itemsize == 16 and PNP_HYPOTHESIS_DTYPE.itemsize == 112
assert PNP_REFINE_DTYPE.itemsize == 112 and PNP_RESULT_DTYPE.itemsize == 80 and PNP_DIAG_DTYPE.itemsize == 640
PNP_MAX_POINTS, PNP_MAX_HYPOTHESES, PNP_MAX_PROBLEMS = 1024, 4096, 65535
PNP_WAVES = 4   # hypotheses per workgroup of pnp_hypotheses_kernel (csrc/pnp_internal.h)
# orbfe_init_params / orbfe_init_hypothesis / orbfe_init_candidate / orbfe_init_result (Initializer, include/orbfe.h)
INIT_PARAMS_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("sigma", "<f4"), ("min_parallax", "<f4"),
                              ("min_triangulated", "<i4"), ("reserved", "<i4")])
INIT_HYPOTHESIS_DTYPE = np.dtype([("M", "<f4", (9,)), ("score", "<f4"), ("n_inliers", "<i4"), ("status", "<i4"), ("reserved", "<i4", (4,))])
INIT_CANDIDATE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("n_good", "<i4"), ("parallax", "<f4"), ("reserved", "<i4", (2,))])
INIT_RESULT_DTYPE = np.dtype([("model", "<i4"), ("success", "<i4"), ("reason", "<i4"), ("best_h", "<i4"), ("best_f", "<i4"), ("score_h", "<f4"),
                              ("score_f", "<f4"), ("rh", "<f4"), ("n_matches", "<i4"), ("n_inliers", "<i4"), ("n_candidates", "<i4"),
                              ("best_candidate", "<i4"), ("n_good", "<i4"), ("second_good_or_n_similar", "<i4"), ("parallax", "<f4"),
                              ("n_triangulated", "<i4"), ("H21", "<f4", (9,)), ("F21", "<f4", (9,)), ("R21", "<f4", (9,)), ("t21", "<f4", (3,)),
                              ("norm1", "<f4", (4,)), ("norm2", "<f4", (4,)), ("reserved", "<i4", (2,))])
assert INIT_PARAMS_DTYPE.itemsize == 32 and INIT_HYPOTHESIS_DTYPE.itemsize == 64 and INIT_CANDIDATE_DTYPE.itemsize == 64
assert INIT_RESULT_DTYPE.itemsize == 224
INIT_MAX_MATCHES, INIT_MAX_HYPOTHESES, INIT_MAX_PROBLEMS = 4096, 1024, 65535
INIT_WAVES = 4   # hypotheses per workgroup of initz_hypotheses_kernel (csrc/initializer_internal.h)
(INIT_FEW_MATCHES, INIT_NO_MODEL, INIT_H_DEGENERATE, INIT_F_FEW_GOOD, INIT_F_SIMILAR, INIT_F_PARALLAX, INIT_H_SECOND, INIT_H_PARALLAX,
 INIT_H_MIN_TRIANGULATED, INIT_H_FEW_GOOD) = (1 << k for k in range(10))
# orbfe_optsim3_pair / orbfe_optsim3_result (Optimizer::OptimizeSim3, include/orbfe.h)
OPTSIM3_PAIR_DTYPE = np.dtype([("Xw1", "<f4", (3,)), ("Xw2", "<f4", (3,)), ("obs1", "<f4", (2,)), ("obs2", "<f4", (2,)),
                               ("inv_sigma2_1", "<f4"), ("inv_sigma2_2", "<f4")])
OPTSIM3_RESULT_DTYPE = np.dtype([("s", "<f4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("n_pairs", "<i4"), ("n_bad", "<i4"),
                                 ("n_inliers", "<i4"), ("iterations", "<i4", (2,)), ("reserved", "<i4", (2,))])
assert OPTSIM3_PAIR_DTYPE.itemsize == 48 and OPTSIM3_RESULT_DTYPE.itemsize == 80
OPTSIM3_MAX_PAIRS, OPTSIM3_MAX_PROBLEMS = 9500, 65535
# orbfe_lba_edge / orbfe_lba_problem / orbfe_lba_result and the ORBFE_LBA_* limits (Optimizer::LocalBundleAdjustment, include/orbfe.h)
LBA_EDGE_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("u_right", "<f4"), ("inv_sigma2", "<f4")])
LBA_PROBLEM_DTYPE = np.dtype([("kf_offset", "<i4"), ("n_kf", "<i4"), ("point_offset", "<i4"), ("n_points", "<i4"), ("edge_offset", "<i4"),
                              ("n_edges", "<i4")])
LBA_RESULT_DTYPE = np.dtype([("rounds", "<i4"), ("n_free", "<i4"), ("n_edges", "<i4"), ("iterations", "<i4", (2,)), ("trials", "<i4", (2,)),
                             ("n_dropped", "<i4"), ("n_erase", "<i4"), ("reserved", "<i4"), ("chi2_first", "<f8", (2,)),
                             ("chi2_final", "<f8", (2,))])
assert LBA_EDGE_DTYPE.itemsize == 24 and LBA_PROBLEM_DTYPE.itemsize == 24 and LBA_RESULT_DTYPE.itemsize == 72
LBA_MAX_FREE, LBA_MAX_KEYFRAMES, LBA_MAX_POINTS, LBA_MAX_EDGES, LBA_MAX_PROBLEMS = 64, 256, 65535, 262140, 65535
LBA_FIRST_ROUND_ONLY = 1
LBA_ERASE, LBA_DROPPED = 1, 2
# orbfe_ba_result and the ORBFE_BA_* constants (Optimizer::BundleAdjustment, include/orbfe.h)
BA_RESULT_DTYPE = np.dtype([("rounds", "<i4"), ("n_free", "<i4"), ("n_edges", "<i4"), ("iterations", "<i4"), ("trials", "<i4"),
                            ("reserved", "<i4"), ("chi2_first", "<f8"), ("chi2_final", "<f8")])
assert BA_RESULT_DTYPE.itemsize == 40
BA_MAX_ITERATIONS = 20
BA_ROBUST = 1
# the ORBFE_GBA_* constants (the global bundle adjustment across the device, include/orbfe.h); the tile is no limit
GBA_MAX_KEYFRAMES, GBA_MAX_POINTS, GBA_MAX_EDGES = 2048, 1048575, 8388600
GBA_TILE_KEYFRAMES = 8
# orbfe_gba_map_keyframe / orbfe_gba_map_result and the ORBFE_GBA_MAP_* constants (the map update behind the global bundle adjustment,
# LoopClosing::RunGlobalBundleAdjustment, include/orbfe.h)
GBA_MAP_KEYFRAME_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Twc", "<f4", (12,)), ("Cw", "<f4", (3,)), ("status", "<i4")])
GBA_MAP_RESULT_DTYPE = np.dtype([("n_optimised", "<i4"), ("n_propagated", "<i4"), ("n_unreached", "<i4"), ("n_taken", "<i4"),
                                 ("n_moved", "<i4"), ("n_left", "<i4"), ("rounds", "<i4"), ("reserved", "<i4")])
assert GBA_MAP_KEYFRAME_DTYPE.itemsize == 112 and GBA_MAP_RESULT_DTYPE.itemsize == 32
GBA_MAP_MAX_KEYFRAMES, GBA_MAP_MAX_POINTS = 65536, 16777216
GBA_MAP_KF_OPTIMISED, GBA_MAP_KF_PROPAGATED, GBA_MAP_KF_UNREACHED = 0, 1, 2
# orbfe_initial_map_result and the ORBFE_IMAP_* reason bits (Tracking::CreateInitialMapMonocular, include/orbfe.h)
INITIAL_MAP_RESULT_DTYPE = np.dtype([("n_points", "<i4"), ("tracked", "<i4"), ("median_depth", "<f4"), ("success", "<i4"), ("reason", "<i4"),
                                     ("reserved", "<i4", (3,)), ("ba", BA_RESULT_DTYPE)])
assert INITIAL_MAP_RESULT_DTYPE.itemsize == 72
IMAP_MEDIAN_NEGATIVE, IMAP_FEW_POINTS, IMAP_NO_POINTS, IMAP_REFUSED = 1, 2, 4, 8
# orbfe_kfdb_query_info and the ORBFE_KFDB_* limits (KeyFrameDatabase, include/orbfe.h)
KFDB_INFO_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common_words", "<i4"), ("min_common_words", "<i4"), ("n_scored", "<i4"),
                            ("n_matches", "<i4"), ("best_acc_score", "<f4"), ("min_score_to_retain", "<f4"), ("n_candidates", "<i4")])
assert KFDB_INFO_DTYPE.itemsize == 32
KFDB_MAX_WORDS, KFDB_NEIGHBOURS, KFDB_MAX_QUERIES, KFDB_MAX_SLOTS, KFDB_MAX_CELLS = 4096, 10, 65535, 4194304, 67108864
KFDB_SCORE_UNKNOWN = -1.0
KFDB_L1_NORM, KFDB_L2_NORM = 0, 1
KFDB_STRIP = 64   # slots per workgroup of the common and score passes (csrc/kfdb_internal.h)
# orbfe_mp_keyframe / orbfe_mp_obs / orbfe_mp_point / orbfe_mp_update and the ORBFE_MP_* limits (MapPoint::ComputeDistinctiveDescriptors,
# MapPoint::UpdateNormalAndDepth, include/orbfe.h)
MP_KEYFRAME_DTYPE = np.dtype([("desc", "<u8"), ("n_keys", "<i4"), ("bad", "<i4"), ("Ow", "<f4", (3,)), ("reserved", "<i4")])
MP_OBS_DTYPE = np.dtype([("kf", "<i4"), ("idx", "<i4")])
MP_POINT_DTYPE = np.dtype([("obs_offset", "<i4"), ("n_obs", "<i4"), ("ref", "<i4"), ("ref_octave", "<i4")])
MP_UPDATE_DTYPE = np.dtype([("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("best", "<i4"), ("n_live", "<i4"),
                            ("status", "<i4"), ("desc", "u1", (32,))])
assert MP_KEYFRAME_DTYPE.itemsize == 32 and MP_OBS_DTYPE.itemsize == 8 and MP_POINT_DTYPE.itemsize == 16 and MP_UPDATE_DTYPE.itemsize == 64
MP_MAX_OBS, MP_MAX_POINTS, MP_MAX_TOTAL_OBS, MP_MAX_KEYFRAMES = 1024, 1048576, 16777216, 1048576
MP_DESCRIPTOR, MP_NORMAL_DEPTH = 1, 2
MP_UPDATED, MP_UNCHANGED, MP_REFUSED = 0, 1, 2
MP_SMALL_OBS = 64   # observations up to which a point is one wave's (csrc/mappoint_internal.h)
# orbfe_cov_subject / orbfe_cov_header / orbfe_cov_entry / orbfe_cov_keyframe / orbfe_cov_problem / orbfe_cov_verdict and the ORBFE_COV_*
# limits (KeyFrame::UpdateConnections, Tracking::UpdateLocalKeyFrames, LocalMapping::KeyFrameCulling, include/orbfe.h)
COV_SUBJECT_DTYPE = np.dtype([("slot_offset", "<i4"), ("n_slots", "<i4"), ("self", "<i4"), ("mode", "<i4")])
COV_HEADER_DTYPE = np.dtype([("n_counted", "<i4"), ("n_ordered", "<i4"), ("kf_max", "<i4"), ("w_max", "<i4"), ("status", "<i4"),
                             ("n_written", "<i4"), ("single", "<i4"), ("reserved", "<i4")])
COV_ENTRY_DTYPE = np.dtype([("kf", "<i4"), ("weight", "<i4")])
COV_KEYFRAME_DTYPE = np.dtype([("keys_un", "<u8"), ("u_right", "<u8"), ("depth", "<u8"), ("slots", "<u8"), ("n_keys", "<i4"),
                               ("th_depth", "<f4"), ("flags", "<i4"), ("reserved", "<i4")])
COV_PROBLEM_DTYPE = np.dtype([("local_offset", "<i4"), ("n_local", "<i4"), ("monocular", "<i4"), ("reserved", "<i4")])
COV_VERDICT_DTYPE = np.dtype([("n_mps", "<i4"), ("n_redundant", "<i4"), ("verdict", "<i4"), ("reserved", "<i4")])
assert COV_SUBJECT_DTYPE.itemsize == 16 and COV_HEADER_DTYPE.itemsize == 32 and COV_ENTRY_DTYPE.itemsize == 8
assert COV_KEYFRAME_DTYPE.itemsize == 48 and COV_PROBLEM_DTYPE.itemsize == 16 and COV_VERDICT_DTYPE.itemsize == 16
(COV_MAX_KEYFRAMES, COV_MAX_CONN, COV_MAX_POINTS, COV_MAX_TOTAL_OBS, COV_MAX_TOTAL_SLOTS, COV_MAX_SUBJECTS, COV_MAX_PROBLEMS,
 COV_MAX_TOTAL_LOCAL, COV_MAX_KEYS) = 32768, 2048, 1048576, 16777216, 16777216, 65535, 65535, 1048576, 65535
COV_MAX_TOTAL_KEYS, COV_MAX_TOTAL_ENTRIES = 4194304, 4194304
COV_TH = 15
COV_CONNECTIONS, COV_VOTES = 0, 1
COV_OK, COV_EMPTY, COV_OVERFLOW, COV_REFUSED = 0, 1, 2, 3
COV_KEPT, COV_CULLED, COV_MARKED, COV_SKIPPED_ID0, COV_ROW_REFUSED = 0, 1, 2, 3, 4
COV_IS_ID0, COV_NOT_ERASE = 1, 2
# orbfe_lm_graph / orbfe_lm_frame / orbfe_lm_header and the ORBFE_LM_* constants (include/orbfe.h)
LM_GRAPH_DTYPE = np.dtype([("parent", "<i4"), ("child_offset", "<i4"), ("n_children", "<i4"), ("n_best", "<i4"), ("best", "<i4", (10,))])
LM_FRAME_DTYPE = np.dtype([("seen_offset", "<i4"), ("n_seen", "<i4")])
LM_HEADER_DTYPE = np.dtype([("n_voted", "<i4"), ("n_local_kf", "<i4"), ("n_local_points", "<i4"), ("ref_kf", "<i4"), ("stop", "<i4"),
                            ("status", "<i4"), ("reserved", "<i4", (2,))])
assert LM_GRAPH_DTYPE.itemsize == 56 and LM_FRAME_DTYPE.itemsize == 8 and LM_HEADER_DTYPE.itemsize == 32
(LM_MAX_FRAMES, LM_MAX_KEYFRAMES, LM_MAX_POINTS, LM_MAX_TOTAL_SLOTS, LM_MAX_TOTAL_CHILDREN, LM_MAX_TOTAL_SEEN, LM_MAX_KF_CAP, LM_MAX_P_CAP,
 LM_MAX_TOTAL_RECORDS) = 65535, 32768, 1048576, 16777216, 32768, 16777216, 2051, 1048576, 4194304
LM_BEST, LM_SIZE = 10, 80
LM_OK, LM_EMPTY, LM_OVERFLOW, LM_REFUSED = 0, 1, 2, 3
LM_STOP_EXHAUSTED, LM_STOP_SIZE, LM_STOP_PARENT = 0, 1, 2
# orbfe_kf_decision_in / orbfe_kf_scales / orbfe_kf_header / orbfe_kf_call and the ORBFE_KF_* constants of the keyframe decision and the
# close stereo points (Tracking::NeedNewKeyFrame, CreateNewKeyFrame, UpdateLastFrame, StereoInitialization, include/orbfe.h)
KF_DECISION_DTYPE = np.dtype([("frame_id", "<u8"), ("last_reloc_frame_id", "<u4"), ("last_keyframe_id", "<u4"), ("max_frames", "<i4"),
                              ("min_frames", "<i4"), ("sensor", "<i4"), ("only_tracking", "<i4"), ("mapper_stopped", "<i4"),
                              ("accept_keyframes", "<i4"), ("keyframes_in_queue", "<i4"), ("n_kfs", "<i4"), ("reserved", "<i4", (2,))])
KF_SCALES_DTYPE = np.dtype([("n_levels", "<i4"), ("th_depth", "<f4"), ("scale_factors", "<f4", (16,))])
KF_HEADER_DTYPE = np.dtype([("n_matches_inliers", "<i4"), ("track_ok", "<i4"), ("n_tracked_close", "<i4"), ("n_non_tracked_close", "<i4"),
                            ("n_ref_matches", "<i4"), ("early", "<i4"), ("conditions", "<i4"), ("need", "<i4"), ("interrupt_ba", "<i4"),
                            ("M", "<i4"), ("c", "<i4"), ("L", "<i4"), ("n_created", "<i4"), ("n_cleared", "<i4"), ("status", "<i4"),
                            ("reserved", "<i4")])
assert KF_DECISION_DTYPE.itemsize == 56 and KF_SCALES_DTYPE.itemsize == 72 and KF_HEADER_DTYPE.itemsize == 64
KF_MAX_FRAMES, KF_MAX_CAP, KF_MAX_TOTAL_ROWS = 65535, 9500, 4194304
KF_STATISTICS, KF_DECISION, KF_CREATE = 1, 2, 4
KF_MODE_KEYFRAME, KF_MODE_LAST_FRAME, KF_MODE_STEREO_INIT = 0, 1, 2
KF_SENSOR_MONOCULAR, KF_SENSOR_STEREO, KF_SENSOR_RGBD = 0, 1, 2
KF_OK, KF_OVERFLOW, KF_REFUSED = 0, 2, 3
KF_EARLY_NONE, KF_EARLY_ONLY_TRACKING, KF_EARLY_STOPPED, KF_EARLY_RELOCALISED = 0, 1, 2, 3
KF_C1A, KF_C1B, KF_C1C, KF_C2 = 1, 2, 4, 8
KF_CLOSE_POINTS, KF_INIT_MIN_KEYS = 100, 500
KF_CALL_POINTERS = ("keys_un", "desc", "depth", "n", "cam", "assigned", "points", "n_points", "outlier", "decision", "ref_kf", "keyframes",
                    "point_bad", "point_observations", "n_points_base", "headers", "new_points", "new_index", "n_new", "depth_selected")
KF_CALL_COUNTS = ("S", "cap", "new_cap", "p_cap", "frame_shift", "point_stride", "observed_offset", "ref_kf_stride", "n_kf", "n_map_points",
                  "mode", "flags")


class KfCall(C.Structure):
    """orbfe_kf_call (include/orbfe.h): the arrays and counts of one orbfe_keyframe_insertion* call; 208 bytes"""
    _fields_ = [(k, C.c_void_p) for k in KF_CALL_POINTERS] + [(k, C.c_int32) for k in KF_CALL_COUNTS]


assert C.sizeof(KfCall) == 208
# orbfe_eg_sim3 / orbfe_eg_vertex / orbfe_eg_edge / orbfe_eg_problem / orbfe_eg_result and the ORBFE_EG_* limits
# (Optimizer::OptimizeEssentialGraph and the map correction behind it, include/orbfe.h)
EG_SIM3_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
EG_VERTEX_DTYPE = np.dtype([("Scw", EG_SIM3_DTYPE), ("Snc", EG_SIM3_DTYPE), ("fixed", "<u4"), ("reserved", "<u4")])
EG_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("kind", "<u4")])
EG_PROBLEM_DTYPE = np.dtype([("kf_offset", "<i4"), ("n_kf", "<i4"), ("edge_offset", "<i4"), ("n_edges", "<i4")])
EG_RESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("trials", "<i4"), ("n_free", "<i4"), ("n_edges", "<i4"),
                            ("envelope_blocks", "<i4"), ("chi2_first", "<f8"), ("chi2_last", "<f8"), ("lambda", "<f8")])
assert EG_SIM3_DTYPE.itemsize == 64 and EG_VERTEX_DTYPE.itemsize == 136 and EG_EDGE_DTYPE.itemsize == 12
assert EG_PROBLEM_DTYPE.itemsize == 16 and EG_RESULT_DTYPE.itemsize == 48
EG_MAX_KEYFRAMES, EG_MAX_EDGES, EG_MAX_ENVELOPE_BLOCKS, EG_MAX_PROBLEMS, EG_MAX_POINTS = 32768, 262144, 131072, 65535, 16777216
EG_FIX_SCALE = 1
EG_NORMAL, EG_LOOP_CONNECTION = 0, 1
EG_DONE, EG_FACTOR_FAILED, EG_REFUSED = 0, 1, -1
# the ORBFE_EGRID_* constants (one graph across the device, include/orbfe.h); EGRID_PHASES: the floats of orbfe_debug_egrid_phases
EGRID_MAX_KEYFRAMES, EGRID_MAX_EDGES, EGRID_MAX_ENVELOPE_BLOCKS = 32768, 262144, 4194304
EGRID_PHASES = ("prepare", "plan", "linearise", "build", "factor", "solve", "update", "control", "levels")


class RectifyCamera(C.Structure):
    """orbfe_rectify_camera (include/orbfe.h): LEFT. / RIGHT. K, D, R, P of a stereo settings file, row-major doubles; 296 bytes"""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 5), ("R", C.c_double * 9), ("P", C.c_double * 12),
                ("src_width", C.c_int32), ("src_height", C.c_int32), ("dst_width", C.c_int32), ("dst_height", C.c_int32)]


assert C.sizeof(RectifyCamera) == 296


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("desc", C.c_void_p), ("u_right", C.c_void_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


# every symbol include/orbfe.h declares (tests check the .so exports all of them)
EXPORTS = [
    "orbfe_last_error", "orbfe_device_count", "orbfe_set_device", "orbfe_device_malloc", "orbfe_device_free", "orbfe_device_upload",
    "orbfe_device_download", "orbfe_thread_release", "orbfe_extractor_prepare", "orbfe_frontend_prepare",
    "orbfe_shard_range", "orbfe_gather_unique_id", "orbfe_gather_create", "orbfe_gather_create_all", "orbfe_gather_destroy",
    "orbfe_gather_rank", "orbfe_gather_records", "orbfe_gather_sync", "orbfe_extractor_create", "orbfe_extractor_destroy",
    "orbfe_extractor_levels", "orbfe_extractor_scale_factors", "orbfe_extractor_inv_scale_factors",
    "orbfe_extractor_sigma2", "orbfe_extractor_inv_sigma2", "orbfe_extractor_features_per_level",
    "orbfe_extractor_max_keypoints", "orbfe_extract", "orbfe_pyramid_level", "orbfe_pyramid_level_size", "orbfe_pyramid_levels",
    "orbfe_extract_batch", "orbfe_extract_batch_device", "orbfe_device_pyramid", "orbfe_device_pyramid_layout", "orbfe_sync",
    "orbfe_device_status", "orbfe_debug_candidates", "orbfe_debug_blurred", "orbfe_debug_blur_kernel", "orbfe_debug_pyramid",
    "orbfe_debug_level_keypoints", "orbfe_profile_enable", "orbfe_stage_times", "orbfe_stage_intervals",
    "orbfe_matcher_create", "orbfe_matcher_destroy", "orbfe_matcher_sync", "orbfe_proj_match_batch_device",
    "orbfe_hamming_matrix_device", "orbfe_hamming_bf_device", "orbfe_proj_candidates",
    "orbfe_search_by_projection_points", "orbfe_search_by_projection_frame", "orbfe_stereo_match_device", "orbfe_stereo_match",
    "orbfe_search_for_initialization", "orbfe_search_by_bow", "orbfe_search_by_bow_kf", "orbfe_search_for_triangulation", "orbfe_proj_best", "orbfe_kf_search", "orbfe_search_by_projection_keyframe", "orbfe_search_local_points",
    "orbfe_search_local_points_batch_device", "orbfe_unproject_stereo_device", "orbfe_track_queries_device", "orbfe_track_queries_stereo_device",
    "orbfe_vocabulary_create", "orbfe_vocabulary_load_text", "orbfe_vocabulary_load_binary", "orbfe_vocabulary_destroy", "orbfe_vocabulary_info",
    "orbfe_bow_transform_device", "orbfe_compute_bow", "orbfe_png_info", "orbfe_png_info2", "orbfe_png_read_gray", "orbfe_png_read_gray2", "orbfe_png_read_gray16",
    "orbfe_pipeline_create", "orbfe_pipeline_destroy", "orbfe_pipeline_input", "orbfe_pipeline_submit", "orbfe_pipeline_wait",
    "orbfe_pipeline_output", "orbfe_pipeline_device_records", "orbfe_pipeline_stream", "orbfe_pipeline_gather", "orbfe_pipeline_gather_wait",
    "orbfe_pipeline_device_input", "orbfe_pipeline_submit_resident", "orbfe_debug_pipeline_streams",
    "orbfe_image_bounds", "orbfe_undistort_points", "orbfe_undistort_frames_device",
    "orbfe_rectifier_create", "orbfe_rectifier_destroy", "orbfe_rectifier_info", "orbfe_rectifier_maps", "orbfe_rectifier_coverage",
    "orbfe_rectify_image", "orbfe_rectify_batch_device", "orbfe_pipeline_set_rectifiers",
    "orbfe_pose_optimization", "orbfe_pose_optimization_batch_device",
    "orbfe_triangulate_matches", "orbfe_triangulate_matches_batch_device", "orbfe_create_new_map_points",
    "orbfe_sim3_ransac_iterations", "orbfe_sim3_solve", "orbfe_sim3_solve_batch_device",
    "orbfe_optimize_sim3", "orbfe_optimize_sim3_batch_device",
    "orbfe_local_bundle_adjustment", "orbfe_lba_workspace_bytes", "orbfe_local_bundle_adjustment_batch_device",
    "orbfe_bundle_adjustment", "orbfe_bundle_adjustment_batch_device",
    "orbfe_global_bundle_adjustment", "orbfe_gba_workspace_bytes", "orbfe_global_bundle_adjustment_device", "orbfe_debug_gba_phases",
    "orbfe_gba_update_map", "orbfe_gba_update_map_device",
    "orbfe_kfdb_create", "orbfe_kfdb_destroy", "orbfe_kfdb_clear", "orbfe_kfdb_size", "orbfe_kfdb_slots", "orbfe_kfdb_add", "orbfe_kfdb_erase",
    "orbfe_kfdb_set_covisibles", "orbfe_kfdb_score", "orbfe_kfdb_detect_relocalization", "orbfe_kfdb_detect_loop",
    "orbfe_kfdb_detect_relocalization_device", "orbfe_kfdb_detect_loop_device", "orbfe_debug_kfdb_arrangement",
    "orbfe_refresh_map_points", "orbfe_refresh_map_points_batch_device",
    "orbfe_covis_count", "orbfe_covis_count_batch_device", "orbfe_covis_cull_keyframes", "orbfe_covis_cull_keyframes_batch_device",
    "orbfe_local_map", "orbfe_local_map_batch_device",
    "orbfe_keyframe_insertion", "orbfe_keyframe_insertion_batch_device",
    "orbfe_initializer_initialize", "orbfe_initializer_workspace_bytes", "orbfe_initializer_initialize_batch_device",
    "orbfe_create_initial_map", "orbfe_initial_map_workspace_bytes", "orbfe_create_initial_map_batch_device",
    "orbfe_essential_graph_envelope_blocks", "orbfe_essential_graph", "orbfe_essential_graph_workspace_bytes",
    "orbfe_essential_graph_batch_device", "orbfe_sim3_correct_points", "orbfe_sim3_correct_points_device",
    "orbfe_essential_graph_grid", "orbfe_essential_graph_grid_workspace_bytes", "orbfe_essential_graph_grid_device",
    "orbfe_debug_egrid_phases", "orbfe_debug_egrid_level_plan",
    "orbfe_pnp_ransac_parameters", "orbfe_pnp_solve", "orbfe_pnp_solve_batch_device",
    "orbfe_vocabulary_nodes", "orbfe_vocabulary_write_text", "orbfe_vocabulary_write_binary", "orbfe_vocabulary_save_text",
    "orbfe_vocabulary_save_binary", "orbfe_vocabulary_training_draw", "orbfe_vocabulary_train_workspace_bytes", "orbfe_vocabulary_train",
    "orbfe_vocabulary_train_device", "orbfe_debug_vocabulary_train_levels",
    "orbfe_fuse_batch_create", "orbfe_fuse_batch_create_device", "orbfe_fuse_batch_destroy", "orbfe_fuse_batch_search",
    "orbfe_fuse_batch_search_device",
]


def build(force: bool = False) -> str:
    """Compile liborbfe.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC]
    if force:
        args.append("-B")
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building liborbfe.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


_lib = None


def lib():
    """Loads liborbfe.so.  Raises if it is missing -- the product path has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same soname as /opt/rocm's).  Whichever is
    # loaded first serves both; torch cannot find the GPU if the system copy got there first, so when torch is
    # installed let it load its runtime before liborbfe.so pulls in libamdhip64.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, ci, cf, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    pi = C.POINTER(ci)
    L.orbfe_last_error.restype = C.c_char_p
    L.orbfe_device_count.argtypes = [pi]
    L.orbfe_extractor_create.argtypes = [C.POINTER(Params), ci, C.POINTER(vp)]
    L.orbfe_extractor_destroy.argtypes = [vp]
    L.orbfe_extractor_levels.argtypes = [vp, pi]
    for n in ("scale_factors", "inv_scale_factors", "sigma2", "inv_sigma2", "features_per_level"):
        getattr(L, "orbfe_extractor_" + n).argtypes = [vp, vp]
    L.orbfe_extractor_max_keypoints.argtypes = [vp, ci, ci, pi]
    L.orbfe_extract.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, pi]
    L.orbfe_pyramid_level.argtypes = [vp, ci, vp, ci, pi, pi]
    L.orbfe_pyramid_level_size.argtypes = [vp, ci, ci, ci, pi, pi]
    L.orbfe_pyramid_levels.argtypes = [vp, vp, vp]
    L.orbfe_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, vp]
    L.orbfe_extract_batch_device.argtypes = [vp, vp, ci, ci, ci, ci, sz, vp, vp, ci, vp, vp]
    L.orbfe_device_pyramid.argtypes = [vp, ci, ci, C.POINTER(vp), pi, pi, pi]
    L.orbfe_sync.argtypes = [vp]
    L.orbfe_device_status.argtypes = [vp]
    L.orbfe_debug_candidates.argtypes = [vp, ci, ci, vp, vp, vp, ci, pi]
    L.orbfe_debug_blurred.argtypes = [vp, ci, ci, vp, ci]
    L.orbfe_debug_pyramid.argtypes = [vp, ci, ci, vp, ci]
    L.orbfe_debug_level_keypoints.argtypes = [vp, ci, ci, vp, vp, vp, ci, pi]
    L.orbfe_profile_enable.argtypes = [vp, ci]
    L.orbfe_stage_times.argtypes = [vp, vp, vp, ci]
    L.orbfe_stage_intervals.argtypes = [vp, vp, vp, vp, vp, ci, vp]
    L.orbfe_hamming_matrix_device.argtypes = [vp, ci, vp, ci, vp, vp]
    L.orbfe_hamming_bf_device.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp]
    L.orbfe_matcher_create.argtypes = [ci, C.POINTER(vp)]
    L.orbfe_matcher_destroy.argtypes = [vp]
    L.orbfe_matcher_sync.argtypes = [vp]
    L.orbfe_proj_match_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, ci, cf, cf, cf, cf, vp, vp, ci, ci, cf, ci,
                                                vp, vp, vp, vp]
    L.orbfe_proj_candidates.argtypes = [C.POINTER(FrameView), vp, ci, vp, vp, ci]
    L.orbfe_search_by_projection_points.argtypes = [C.POINTER(FrameView), vp, ci, cf, vp, vp, pi]
    L.orbfe_search_by_projection_frame.argtypes = [C.POINTER(FrameView), vp, ci, ci, vp, vp, pi]
    L.orbfe_unproject_stereo_device.argtypes = [ci, vp, vp, vp, vp, ci, vp, ci, vp, vp]
    L.orbfe_track_queries_device.argtypes = [ci, vp, vp, vp, ci, ci, vp, vp, vp]
    L.orbfe_track_queries_stereo_device.argtypes = [ci, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp]
    L.orbfe_search_local_points.argtypes = [C.POINTER(FrameView), vp, vp, ci, cf, cf, vp, vp, vp, pi, pi]
    L.orbfe_search_local_points_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, ci, cf, cf, cf, cf, vp, vp, vp, ci, cf, cf,
                                                         vp, vp, vp, vp, vp, vp]
    L.orbfe_search_by_projection_keyframe.argtypes = [C.POINTER(FrameView), vp, ci, ci, ci, vp, vp, pi]
    L.orbfe_vocabulary_create.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, C.POINTER(vp)]
    L.orbfe_vocabulary_load_text.argtypes = [C.c_char_p, ci, C.POINTER(vp)]
    L.orbfe_vocabulary_load_binary.argtypes = [C.c_char_p, ci, C.POINTER(vp)]
    L.orbfe_vocabulary_destroy.argtypes = [vp]
    L.orbfe_vocabulary_info.argtypes = [vp, pi, pi, pi, pi]
    L.orbfe_bow_transform_device.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_compute_bow.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, pi, vp, vp, pi]
    L.orbfe_proj_best.argtypes = [C.POINTER(FrameView), vp, ci, ci, vp, ci, vp, vp]
    L.orbfe_kf_search.argtypes = [C.POINTER(FrameView), vp, vp, vp, ci, ci, ci, ci, vp, vp, pi]
    L.orbfe_fuse_batch_create.argtypes = [ci, vp, vp, vp, ci, C.POINTER(vp)]
    L.orbfe_fuse_batch_create_device.argtypes = [ci, vp, vp, vp, vp, ci, cf, cf, cf, cf, vp, vp, ci, vp, C.POINTER(vp)]
    L.orbfe_fuse_batch_destroy.argtypes = [vp]
    L.orbfe_fuse_batch_search.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp]
    L.orbfe_fuse_batch_search_device.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp]
    L.orbfe_search_for_triangulation.argtypes = [vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, ci, ci, vp, pi]
    L.orbfe_search_by_bow_kf.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, ci, vp, cf, ci, vp, pi]
    L.orbfe_search_by_bow.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, ci, vp, ci, vp, cf, ci, vp, pi]
    L.orbfe_search_for_initialization.argtypes = [C.POINTER(FrameView), C.POINTER(FrameView), vp, ci, cf, ci, vp, pi]
    L.orbfe_stereo_match_device.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, vp, vp, vp]
    L.orbfe_stereo_match.argtypes = [vp, vp, vp, vp, ci, vp, vp, ci, cf, cf, vp, vp, pi]
    pcal, pf = C.POINTER(Calibration), C.POINTER(cf)
    L.orbfe_image_bounds.argtypes = [pcal, ci, ci, pf, pf, pf, pf]
    L.orbfe_undistort_points.argtypes = [pcal, vp, ci, vp]
    L.orbfe_undistort_frames_device.argtypes = [ci, vp, vp, ci, pcal, ci, vp, ci, ci, ci, sz, vp, vp, vp, vp, vp]
    prc, pi32 = C.POINTER(RectifyCamera), C.POINTER(C.c_int32)
    L.orbfe_rectifier_create.argtypes = [prc, ci, C.POINTER(vp)]
    L.orbfe_rectifier_destroy.argtypes = [vp]
    L.orbfe_rectifier_info.argtypes = [vp, prc, pi]
    L.orbfe_rectifier_maps.argtypes = [vp, vp, vp]
    L.orbfe_rectifier_coverage.argtypes = [vp, pi32, pi32, pi32]
    L.orbfe_rectify_image.argtypes = [vp, vp, ci, vp, ci]
    L.orbfe_rectify_batch_device.argtypes = [vp, vp, ci, ci, sz, vp, ci, sz, vp]
    L.orbfe_pipeline_set_rectifiers.argtypes = [vp, vp, vp]
    L.orbfe_pose_optimization.argtypes = [C.POINTER(FrameView), vp, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_pose_optimization_batch_device.argtypes = [ci, vp, vp, vp, ci, vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, ci, vp]
    L.orbfe_triangulate_matches.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, pi]
    L.orbfe_triangulate_matches_batch_device.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_create_new_map_points.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]
    L.orbfe_sim3_ransac_iterations.argtypes = [ci, C.c_double, ci, ci]
    L.orbfe_sim3_solve.argtypes = [vp, vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp]
    L.orbfe_sim3_solve_batch_device.argtypes = [ci, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_optimize_sim3.argtypes = [vp, vp, vp, ci, vp, cf, ci, vp, vp]
    L.orbfe_optimize_sim3_batch_device.argtypes = [ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_local_bundle_adjustment.argtypes = [vp, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_lba_workspace_bytes.argtypes = [ci, ci, ci, ci, C.POINTER(sz)]
    L.orbfe_local_bundle_adjustment_batch_device.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]
    L.orbfe_bundle_adjustment.argtypes = [vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp]
    L.orbfe_bundle_adjustment_batch_device.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]
    L.orbfe_global_bundle_adjustment.argtypes = [vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp]
    L.orbfe_gba_workspace_bytes.argtypes = [ci, ci, ci, C.POINTER(sz)]
    L.orbfe_debug_gba_phases.argtypes = [ci, vp]
    L.orbfe_global_bundle_adjustment_device.argtypes = [vp, vp, vp, ci, vp, ci, ci, vp, ci, ci, ci, vp, vp, vp, vp, sz, vp]
    L.orbfe_gba_update_map.argtypes = [vp, vp, vp, ci, vp, ci, cf, vp, vp, vp, ci, vp, ci, vp, vp, vp]
    L.orbfe_gba_update_map_device.argtypes = [vp, vp, vp, ci, vp, ci, cf, vp, ci, vp, vp, ci, vp, ci, vp, vp, vp, vp]
    i64 = C.c_int64
    L.orbfe_kfdb_create.argtypes = [ci, ci, ci, C.POINTER(vp)]
    L.orbfe_debug_kfdb_arrangement.argtypes = [ci]
    L.orbfe_kfdb_destroy.argtypes = [vp]
    L.orbfe_kfdb_clear.argtypes = [vp]
    L.orbfe_kfdb_size.argtypes = [vp, pi, pi]
    L.orbfe_kfdb_slots.argtypes = [vp, vp, ci, pi]
    L.orbfe_kfdb_add.argtypes = [vp, i64, vp, vp, ci]
    L.orbfe_kfdb_erase.argtypes = [vp, i64]
    L.orbfe_kfdb_set_covisibles.argtypes = [vp, ci, vp, vp]
    L.orbfe_kfdb_score.argtypes = [vp, vp, vp, ci, vp, ci, vp]
    L.orbfe_kfdb_detect_relocalization.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_kfdb_detect_loop.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_kfdb_detect_relocalization_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_kfdb_detect_loop_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_refresh_map_points.argtypes = [vp, ci, vp, ci, vp, vp, ci, vp, ci, ci, vp]
    L.orbfe_refresh_map_points_batch_device.argtypes = [ci, vp, ci, vp, ci, vp, vp, ci, vp, ci, ci, vp, vp]
    L.orbfe_covis_count.argtypes = [vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp]
    L.orbfe_covis_count_batch_device.argtypes = [ci, vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp]
    L.orbfe_covis_cull_keyframes.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, ci, vp]
    L.orbfe_covis_cull_keyframes_batch_device.argtypes = [ci, vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp]
    L.orbfe_local_map_batch_device.argtypes = [ci, vp, vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, ci, vp, ci, ci, vp, vp, vp, vp,
                                               vp, vp]
    L.orbfe_local_map.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.orbfe_keyframe_insertion_batch_device.argtypes = [C.POINTER(KfCall), vp, vp]
    L.orbfe_keyframe_insertion.argtypes = [C.POINTER(KfCall), vp]
    L.orbfe_initializer_initialize.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_initializer_workspace_bytes.argtypes = [ci, ci, C.POINTER(sz)]
    L.orbfe_initializer_initialize_batch_device.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.orbfe_create_initial_map.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_initial_map_workspace_bytes.argtypes = [ci, ci, C.POINTER(sz)]
    L.orbfe_create_initial_map_batch_device.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp,
                                                        vp, vp, sz, vp]
    L.orbfe_essential_graph_envelope_blocks.argtypes = [ci, vp, vp, ci, C.POINTER(i64)]
    L.orbfe_essential_graph.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp]
    L.orbfe_essential_graph_workspace_bytes.argtypes = [ci, ci, ci, ci, C.POINTER(sz)]
    L.orbfe_essential_graph_batch_device.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]
    L.orbfe_essential_graph_grid.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp]
    L.orbfe_essential_graph_grid_workspace_bytes.argtypes = [ci, ci, i64, C.POINTER(sz)]
    L.orbfe_essential_graph_grid_device.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp, sz, vp]
    L.orbfe_debug_egrid_phases.argtypes = [ci, vp]
    L.orbfe_debug_egrid_level_plan.argtypes = [vp, ci, vp, vp]
    L.orbfe_sim3_correct_points.argtypes = [vp, ci, vp, vp, vp, ci, vp]
    L.orbfe_sim3_correct_points_device.argtypes = [vp, ci, vp, vp, ci, vp, ci, vp, vp]
    L.orbfe_pnp_ransac_parameters.argtypes = [ci, C.c_double, ci, ci, ci, cf, vp, vp, vp]
    L.orbfe_pnp_solve.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_pnp_solve_batch_device.argtypes = [ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    ptc = C.POINTER(VocabTrainConfig)
    L.orbfe_vocabulary_nodes.argtypes = [vp, vp, vp, vp, vp]
    L.orbfe_vocabulary_write_text.argtypes = [C.c_char_p, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    L.orbfe_vocabulary_write_binary.argtypes = [C.c_char_p, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    L.orbfe_vocabulary_save_text.argtypes = [vp, C.c_char_p]
    L.orbfe_vocabulary_save_binary.argtypes = [vp, C.c_char_p]
    L.orbfe_vocabulary_training_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32]
    L.orbfe_vocabulary_train_workspace_bytes.argtypes = [ptc, i64, ci, C.POINTER(sz)]
    L.orbfe_vocabulary_train.argtypes = [ptc, vp, vp, ci, ci, vp, vp, C.POINTER(vp)]
    L.orbfe_vocabulary_train_device.argtypes = [ptc, vp, vp, ci, ci, vp, sz, vp, vp, vp, C.POINTER(vp)]
    L.orbfe_debug_vocabulary_train_levels.argtypes = [ci, vp, vp, vp, vp, vp, pi]
    for name in EXPORTS:
        if name != "orbfe_last_error":
            getattr(L, name).restype = ci
    L.orbfe_vocabulary_training_draw.restype = C.c_uint32
    _lib = L
    return L


def check(rc: int, where: str):
    if rc != OK:
        raise OrbfeError(rc, where, lib().orbfe_last_error().decode(errors="replace"))


def stream_handle(stream) -> C.c_void_p:
    """torch stream -> hipStream_t.  None selects the handle's own stream.  torch's default stream is the NULL
    stream, which the C ABI also reads as "the handle's own stream" -- refuse it instead of racing silently."""
    if stream is None:
        return C.c_void_p(None)
    h = int(stream.cuda_stream)
    if h == 0:
        raise ValueError("pass an explicit torch.cuda.Stream (or None for the handle's own stream), not the default stream")
    return C.c_void_p(h)


def ptr(a) -> C.c_void_p:
    """Host numpy array or torch tensor -> void*."""
    if a is None:
        return C.c_void_p(None)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())
