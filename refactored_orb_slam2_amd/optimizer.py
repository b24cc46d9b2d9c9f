"""Optimizer::PoseOptimization, Optimizer::OptimizeSim3, Optimizer::LocalBundleAdjustment and Optimizer::BundleAdjustment over the C
ABI of liborbfe.so (L/src/Optimizer.cc:233-435, :1381-1573, :437-760, :43-231, L/ = Source/Libraries/ORB_SLAM2/): the pose of a frame
from its keypoint <-> map-point pairs, and which pairs were wrong; the similarity between two keyframes of a loop candidate from their
matched map points, and which matches were wrong; the poses of the local keyframes and the points they see, and which observations to
erase; the poses of all keyframes of a map and all its points.

pose_optimization is the per-frame call of Tracking on host arrays; pose_optimization_batch optimises every frame of a batch in one
launch on device tensors (pose_kernels.hip, one workgroup per frame) and reads the `assigned` array of the batched projection
searches unchanged.  Both run the same kernel; there is no CPU path.

optimize_sim3 is the per-candidate call of LoopClosing::ComputeSim3 on host arrays; optimize_sim3_batch optimises every candidate of
a batch in one launch on device tensors (optsim3_kernels.hip, one workgroup per candidate).

local_bundle_adjustment is the call of LocalMapping::Run on host arrays; local_bundle_adjustment_batch optimises ragged problems that
lie in device tensors in one launch (lba_kernels.hip, one workgroup per problem) with a workspace of lba_workspace_bytes(...) bytes.

bundle_adjustment is the call of Tracking::CreateInitialMapMonocular (20 iterations, robust) and of
LoopClosing::RunGlobalBundleAdjustment (10, not robust) on host arrays; bundle_adjustment_batch takes the same ragged device tensors
and the same workspace as local_bundle_adjustment_batch (ba_kernels.hip: one optimize() call, no classification, no erase list).

essential_graph is the call of LoopClosing::CorrectLoop on host arrays (Optimizer::OptimizeEssentialGraph, :1366: the Sim3 form, or
the SE3 form with fix_scale); essential_graph_batch optimises ragged graphs that lie in device tensors in one launch
(egraph_kernels.hip, one workgroup per graph) with a workspace of essential_graph_workspace_bytes(...) bytes, whose env_cap
essential_graph_envelope_blocks(...) states per graph.  The vertex order is the elimination order: list keyframes by ascending mnId.
essential_graph_grid is the same call for ONE graph across the whole device (egraph_grid_kernels.hip: every phase of a trial a
launch, the factorisation level by level with a workgroup per block): the same bytes for a graph both take, envelopes 32 times as
large, and the form a loop closure wants -- it has one graph.  essential_graph_grid_device takes device tensors and a workspace of
essential_graph_grid_workspace_bytes(...) bytes; both are synchronous.
The map correction behind it is sim3.correct_points.

gba_update_map is what LoopClosing::RunGlobalBundleAdjustment does with the adjustment's result (L/src/LoopClosing.cc:648-703): the
correction of every keyframe the adjustment did not see through the spanning tree, SetPose's Twc and Cw of every keyframe, and every
map point either replaced or moved with its reference keyframe (gba_map_kernels.hip).  gba_update_map_device takes device tensors --
the two output tables of global_bundle_adjustment_device as they lie -- and is asynchronous on its stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import BA_MAX_ITERATIONS, BA_RESULT_DTYPE, BA_ROBUST
from ._lib import GBA_MAX_EDGES, GBA_MAX_KEYFRAMES, GBA_MAX_POINTS, GBA_TILE_KEYFRAMES
from ._lib import (GBA_MAP_KEYFRAME_DTYPE, GBA_MAP_KF_OPTIMISED, GBA_MAP_KF_PROPAGATED, GBA_MAP_KF_UNREACHED, GBA_MAP_MAX_KEYFRAMES,
                   GBA_MAP_MAX_POINTS, GBA_MAP_RESULT_DTYPE)
from ._lib import (LBA_DROPPED, LBA_EDGE_DTYPE, LBA_ERASE, LBA_FIRST_ROUND_ONLY, LBA_PROBLEM_DTYPE, LBA_RESULT_DTYPE)
from ._lib import (EG_DONE, EG_EDGE_DTYPE, EG_FACTOR_FAILED, EG_FIX_SCALE, EG_LOOP_CONNECTION, EG_NORMAL, EG_PROBLEM_DTYPE, EG_REFUSED,
                   EG_RESULT_DTYPE, EG_SIM3_DTYPE, EG_VERTEX_DTYPE)
from ._lib import EGRID_MAX_EDGES, EGRID_MAX_ENVELOPE_BLOCKS, EGRID_MAX_KEYFRAMES
from ._lib import OPTSIM3_PAIR_DTYPE, OPTSIM3_RESULT_DTYPE, POSE_CAMERA_DTYPE, POSE_DISCARD, POSE_RESULT_DTYPE, SIM3_VIEW_DTYPE

__all__ = ["POSE_CAMERA_DTYPE", "POSE_RESULT_DTYPE", "POSE_DISCARD", "pose_camera", "pose_optimization", "pose_optimization_batch",
           "OPTSIM3_PAIR_DTYPE", "OPTSIM3_RESULT_DTYPE", "sim3_view", "optimize_sim3", "optimize_sim3_batch",
           "LBA_EDGE_DTYPE", "LBA_PROBLEM_DTYPE", "LBA_RESULT_DTYPE", "LBA_FIRST_ROUND_ONLY", "LBA_ERASE", "LBA_DROPPED",
           "local_bundle_adjustment", "local_bundle_adjustment_batch", "lba_workspace_bytes",
           "BA_RESULT_DTYPE", "BA_ROBUST", "BA_MAX_ITERATIONS", "bundle_adjustment", "bundle_adjustment_batch",
           "GBA_MAX_KEYFRAMES", "GBA_MAX_POINTS", "GBA_MAX_EDGES", "GBA_TILE_KEYFRAMES", "global_bundle_adjustment",
           "global_bundle_adjustment_device", "gba_workspace_bytes",
           "GBA_MAP_KEYFRAME_DTYPE", "GBA_MAP_RESULT_DTYPE", "GBA_MAP_MAX_KEYFRAMES", "GBA_MAP_MAX_POINTS", "GBA_MAP_KF_OPTIMISED",
           "GBA_MAP_KF_PROPAGATED", "GBA_MAP_KF_UNREACHED", "gba_update_map", "gba_update_map_device",
           "EG_SIM3_DTYPE", "EG_VERTEX_DTYPE", "EG_EDGE_DTYPE", "EG_PROBLEM_DTYPE", "EG_RESULT_DTYPE", "EG_FIX_SCALE", "EG_NORMAL",
           "EG_LOOP_CONNECTION", "EG_DONE", "EG_FACTOR_FAILED", "EG_REFUSED", "essential_graph", "essential_graph_batch",
           "essential_graph_envelope_blocks", "essential_graph_workspace_bytes",
           "EGRID_MAX_KEYFRAMES", "EGRID_MAX_EDGES", "EGRID_MAX_ENVELOPE_BLOCKS", "essential_graph_grid", "essential_graph_grid_device",
           "essential_graph_grid_workspace_bytes"]


def pose_camera(fx, fy, cx, cy, mbf, inv_level_sigma2) -> np.ndarray:
    """One orbfe_pose_camera record: the Frame's fx, fy, cx, cy, mbf and mvInvLevelSigma2 (its length is n_levels)."""
    sig = np.asarray(inv_level_sigma2, np.float32).reshape(-1)
    cam = np.zeros(1, POSE_CAMERA_DTYPE)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"] = fx, fy, cx, cy, mbf
    cam["n_levels"] = len(sig)
    cam["inv_level_sigma2"][0, :min(len(sig), _lib.MAX_LEVELS)] = sig[:_lib.MAX_LEVELS]
    return cam


def pose_optimization(keys_un, u_right, assigned, points, camera, Tcw):
    """Optimizer::PoseOptimization of one frame.  keys_un: KP_DTYPE (n) = mvKeysUn; u_right: (n) float32 = mvuRight or None (every
    edge monocular); assigned: (n) int32, >= 0 <=> mvpMapPoints[i] != NULL, an index into points; points: a structured array whose
    first three floats are the world position (MAP_POINT_DTYPE, LAST_POINT_DTYPE) or an (m, 3) float32 array; camera: pose_camera(...);
    Tcw: 12 or 3 x 4 / 4 x 4 floats.  Returns (result, outlier): one POSE_RESULT_DTYPE record and mvbOutlier as (n) uint8."""
    keys_un = np.ascontiguousarray(keys_un, _lib.KP_DTYPE)
    n = len(keys_un)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    assigned = np.ascontiguousarray(assigned, np.int32)
    if len(assigned) != n or (ur is not None and len(ur) != n):
        raise ValueError("keys_un, u_right and assigned must have one entry per keypoint")
    points = np.ascontiguousarray(points)
    if points.dtype.fields is None:
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        stride = 12
    else:
        stride = points.dtype.itemsize
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
    cam = np.ascontiguousarray(camera, POSE_CAMERA_DTYPE).reshape(1)
    fv = _lib.FrameView(n, keys_un.ctypes.data if n else None, None, ur.ctypes.data if ur is not None and n else None, 0, 0, 0, 0)
    res = np.zeros(1, POSE_RESULT_DTYPE)
    outlier = np.zeros(n, np.uint8)
    _lib.check(_lib.lib().orbfe_pose_optimization(C.byref(fv), _lib.ptr(assigned), _lib.ptr(points), stride, len(points), _lib.ptr(cam),
                                                  _lib.ptr(T), _lib.ptr(res), _lib.ptr(outlier)), "orbfe_pose_optimization")
    return res[0], outlier


def pose_optimization_batch(keys_un, u_right, n, assigned, points, n_points, camera, Tcw_in, result, outlier, frame_shift: int = 0,
                            flags: int = 0, stream=None):
    """orbfe_pose_optimization_batch_device on torch CUDA tensors: keys_un (F,cap,28) u8, u_right (F,cap) f32 or None, n (F) i32,
    assigned (F,cap) i32 (written only with POSE_DISCARD), points (F,p_cap,stride) u8 whose records start with the position, n_points
    (F) i32, camera (88) u8 = one POSE_CAMERA_DTYPE record, Tcw_in (F,12) f32, result (F,68) u8 = POSE_RESULT_DTYPE, outlier (F,cap) u8.
    The points of frame f are those of frame (f - frame_shift) mod F.  stream: a torch.cuda.Stream, or None for the NULL stream."""
    F, cap = int(keys_un.shape[0]), int(keys_un.shape[1])
    p_cap, stride = int(points.shape[1]), int(points.shape[2])
    _lib.check(_lib.lib().orbfe_pose_optimization_batch_device(F, _lib.ptr(keys_un), _lib.ptr(u_right), _lib.ptr(n), cap,
                                                               _lib.ptr(assigned), _lib.ptr(points), stride, _lib.ptr(n_points), p_cap,
                                                               int(frame_shift), _lib.ptr(camera), _lib.ptr(Tcw_in), _lib.ptr(result),
                                                               _lib.ptr(outlier), int(flags), _lib.stream_handle(stream)),
               "orbfe_pose_optimization_batch_device")


def sim3_view(Rcw, tcw, fx, fy, cx, cy) -> np.ndarray:
    """One orbfe_sim3_view record: GetRotation() (row-major), GetTranslation() and mK of a KeyFrame."""
    v = np.zeros(1, SIM3_VIEW_DTYPE)
    v["Rcw"][0] = np.asarray(Rcw, np.float32).reshape(9)
    v["tcw"][0] = np.asarray(tcw, np.float32).reshape(3)
    v["fx"], v["fy"], v["cx"], v["cy"] = fx, fy, cx, cy
    return v


def optimize_sim3(view1, view2, pairs, s_R_t_in, th2, fix_scale):
    """Optimizer::OptimizeSim3 of one loop candidate.  view1 / view2: sim3_view(...) of pKF1 / pKF2; pairs: OPTSIM3_PAIR_DTYPE (n), the
    correspondences that passed the filters of Optimizer.cc:1436-1468; s_R_t_in: g2oS12 as 13 floats (scale, rotation row-major,
    translation); th2: the chi-square bound.  Returns (result, bad): one OPTSIM3_RESULT_DTYPE record -- n_inliers is the reference's
    return value, s / R / t are the input's bits when it is 0 by the fewer-than-10 rule -- and (n) uint8, 1 where the vpMatches1 entry
    is nulled."""
    v1 = np.ascontiguousarray(view1, SIM3_VIEW_DTYPE).reshape(1)
    v2 = np.ascontiguousarray(view2, SIM3_VIEW_DTYPE).reshape(1)
    pairs = np.ascontiguousarray(pairs, OPTSIM3_PAIR_DTYPE).reshape(-1)
    n = len(pairs)
    sRt = np.ascontiguousarray(np.asarray(s_R_t_in, np.float32).reshape(13))
    res = np.zeros(1, OPTSIM3_RESULT_DTYPE)
    bad = np.zeros(n, np.uint8)
    _lib.check(_lib.lib().orbfe_optimize_sim3(_lib.ptr(v1), _lib.ptr(v2), _lib.ptr(pairs) if n else None, n, _lib.ptr(sRt), float(th2),
                                              1 if fix_scale else 0, _lib.ptr(res), _lib.ptr(bad) if n else None), "orbfe_optimize_sim3")
    return res[0], bad


def optimize_sim3_batch(view1, view2, pairs, n, s_R_t_in, th2, fix_scale, result, bad, stream=None):
    """orbfe_optimize_sim3_batch_device on torch CUDA tensors: view1, view2 (P,64) u8 = SIM3_VIEW_DTYPE, pairs (P,cap,48) u8 =
    OPTSIM3_PAIR_DTYPE, n (P) i32, s_R_t_in (P,13) f32, th2 (P) f32, fix_scale (P) i32, result (P,80) u8 = OPTSIM3_RESULT_DTYPE, bad
    (P,cap) u8.  Rows behind n[p] are neither read nor written.  stream: a torch.cuda.Stream, or None for the NULL stream."""
    P, cap = int(pairs.shape[0]), int(pairs.shape[1])
    _lib.check(_lib.lib().orbfe_optimize_sim3_batch_device(P, _lib.ptr(view1), _lib.ptr(view2), _lib.ptr(pairs), _lib.ptr(n), cap,
                                                           _lib.ptr(s_R_t_in), _lib.ptr(th2), _lib.ptr(fix_scale), _lib.ptr(result),
                                                           _lib.ptr(bad), _lib.stream_handle(stream)),
               "orbfe_optimize_sim3_batch_device")


def local_bundle_adjustment(camera, poses, fixed, points, edges, flags: int = 0):
    """Optimizer::LocalBundleAdjustment of one window from its edge list on.  camera: pose_camera(...) (fx fy cx cy mbf are read);
    poses: (n_kf, 12) float32, rows of [R | t]; fixed: (n_kf) uint8, != 0 for a keyframe of lFixedCameras or with mnId == 0; points:
    (n_points, 3) float32; edges: LBA_EDGE_DTYPE (n_edges) in any order; flags: LBA_FIRST_ROUND_ONLY.  Returns (poses_out, points_out,
    erase, result): erase holds the LBA_ERASE / LBA_DROPPED bits per edge, result is one LBA_RESULT_DTYPE record."""
    cam = np.ascontiguousarray(camera, POSE_CAMERA_DTYPE).reshape(1)
    poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    edges = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    if len(fixed) != len(poses):
        raise ValueError("poses and fixed must have one entry per keyframe")
    poses_out, points_out = np.zeros_like(poses), np.zeros_like(points)
    erase = np.zeros(len(edges), np.uint8)
    res = np.zeros(1, LBA_RESULT_DTYPE)
    opt = lambda a: _lib.ptr(a) if len(a) else None
    _lib.check(_lib.lib().orbfe_local_bundle_adjustment(_lib.ptr(cam), opt(poses), opt(fixed), len(poses), opt(points), len(points),
                                                        opt(edges), len(edges), int(flags), opt(poses_out), opt(points_out), opt(erase),
                                                        _lib.ptr(res)), "orbfe_local_bundle_adjustment")
    return poses_out, points_out, erase, res[0]


def lba_workspace_bytes(P: int, kf_cap: int, point_cap: int, edge_cap: int) -> int:
    """orbfe_lba_workspace_bytes: the workspace of a batch of P problems of at most kf_cap keyframes, point_cap points and edge_cap
    edges each."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().orbfe_lba_workspace_bytes(int(P), int(kf_cap), int(point_cap), int(edge_cap), C.byref(n)),
               "orbfe_lba_workspace_bytes")
    return int(n.value)


def local_bundle_adjustment_batch(camera, problems, poses, fixed, points, edges, kf_cap, point_cap, edge_cap, poses_out, points_out,
                                  erase, result, workspace, flags: int = 0, stream=None):
    """orbfe_local_bundle_adjustment_batch_device on torch CUDA tensors: camera (88) u8 = one POSE_CAMERA_DTYPE record, problems (P,24)
    u8 = LBA_PROBLEM_DTYPE, poses (K,12) f32, fixed (K) u8, points (M,stride) u8 whose records start with the position (or (M,3) f32),
    edges (E,24) u8 = LBA_EDGE_DTYPE, listed point by point with keyframes ascending; poses_out (K,12) f32, points_out (M,3) f32, erase
    (E) u8, result (P,72) u8 = LBA_RESULT_DTYPE, workspace: u8 of at least lba_workspace_bytes(P, kf_cap, point_cap, edge_cap) bytes.
    Rows no problem names are not written.  stream: a torch.cuda.Stream, or None for the NULL stream."""
    P = int(problems.shape[0])
    stride = int(points.shape[1]) * int(points.element_size()) if points.dim() == 2 else 12
    _lib.check(_lib.lib().orbfe_local_bundle_adjustment_batch_device(
        P, _lib.ptr(camera), _lib.ptr(problems), _lib.ptr(poses), _lib.ptr(fixed), _lib.ptr(points), stride, _lib.ptr(edges), int(kf_cap),
        int(point_cap), int(edge_cap), int(flags), _lib.ptr(poses_out), _lib.ptr(points_out), _lib.ptr(erase), _lib.ptr(result),
        _lib.ptr(workspace), int(workspace.numel()) * int(workspace.element_size()), _lib.stream_handle(stream)),
        "orbfe_local_bundle_adjustment_batch_device")


def bundle_adjustment(camera, poses, fixed, points, edges, n_iterations: int = 5, robust: bool = True):
    """Optimizer::BundleAdjustment of one map from its edge list on: ONE optimize(n_iterations), a Huber kernel on every edge iff
    `robust`.  Arguments as local_bundle_adjustment's; fixed: != 0 for the keyframe with mnId == 0.  Returns (poses_out, points_out,
    result): result is one BA_RESULT_DTYPE record.  A point without an edge keeps its bytes."""
    cam = np.ascontiguousarray(camera, POSE_CAMERA_DTYPE).reshape(1)
    poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    edges = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    if len(fixed) != len(poses):
        raise ValueError("poses and fixed must have one entry per keyframe")
    poses_out, points_out = np.zeros_like(poses), np.zeros_like(points)
    res = np.zeros(1, BA_RESULT_DTYPE)
    opt = lambda a: _lib.ptr(a) if len(a) else None
    _lib.check(_lib.lib().orbfe_bundle_adjustment(_lib.ptr(cam), opt(poses), opt(fixed), len(poses), opt(points), len(points), opt(edges),
                                                  len(edges), int(n_iterations), BA_ROBUST if robust else 0, opt(poses_out),
                                                  opt(points_out), _lib.ptr(res)), "orbfe_bundle_adjustment")
    return poses_out, points_out, res[0]


def bundle_adjustment_batch(camera, problems, poses, fixed, points, edges, kf_cap, point_cap, edge_cap, poses_out, points_out, result,
                            workspace, n_iterations: int = 5, robust: bool = True, stream=None):
    """orbfe_bundle_adjustment_batch_device on torch CUDA tensors, laid out as local_bundle_adjustment_batch's; result (P,40) u8 =
    BA_RESULT_DTYPE, workspace: u8 of at least lba_workspace_bytes(P, kf_cap, point_cap, edge_cap) bytes.  n_iterations and robust
    hold for every problem.  Rows no problem names are not written."""
    P = int(problems.shape[0])
    stride = int(points.shape[1]) * int(points.element_size()) if points.dim() == 2 else 12
    _lib.check(_lib.lib().orbfe_bundle_adjustment_batch_device(
        P, _lib.ptr(camera), _lib.ptr(problems), _lib.ptr(poses), _lib.ptr(fixed), _lib.ptr(points), stride, _lib.ptr(edges), int(kf_cap),
        int(point_cap), int(edge_cap), int(n_iterations), BA_ROBUST if robust else 0, _lib.ptr(poses_out), _lib.ptr(points_out),
        _lib.ptr(result), _lib.ptr(workspace), int(workspace.numel()) * int(workspace.element_size()), _lib.stream_handle(stream)),
        "orbfe_bundle_adjustment_batch_device")


def global_bundle_adjustment(camera, poses, fixed, points, edges, n_iterations: int = 5, robust: bool = True):
    """orbfe_global_bundle_adjustment: bundle_adjustment for ONE map of up to GBA_MAX_KEYFRAMES keyframes, any number of them free,
    across the whole device.  Arguments and return value as bundle_adjustment's; a problem both take gives the same bytes."""
    cam = np.ascontiguousarray(camera, POSE_CAMERA_DTYPE).reshape(1)
    poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    edges = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    if len(fixed) != len(poses):
        raise ValueError("poses and fixed must have one entry per keyframe")
    poses_out, points_out = np.zeros_like(poses), np.zeros_like(points)
    res = np.zeros(1, BA_RESULT_DTYPE)
    opt = lambda a: _lib.ptr(a) if len(a) else None
    _lib.check(_lib.lib().orbfe_global_bundle_adjustment(_lib.ptr(cam), opt(poses), opt(fixed), len(poses), opt(points), len(points),
                                                         opt(edges), len(edges), int(n_iterations), BA_ROBUST if robust else 0,
                                                         opt(poses_out), opt(points_out), _lib.ptr(res)), "orbfe_global_bundle_adjustment")
    return poses_out, points_out, res[0]


def gba_workspace_bytes(kf_cap: int, point_cap: int, edge_cap: int) -> int:
    """orbfe_gba_workspace_bytes: the workspace of one problem of at most kf_cap keyframes, point_cap points and edge_cap edges."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().orbfe_gba_workspace_bytes(int(kf_cap), int(point_cap), int(edge_cap), C.byref(n)), "orbfe_gba_workspace_bytes")
    return int(n.value)


def global_bundle_adjustment_device(camera, poses, fixed, points, edges, poses_out, points_out, result, workspace, n_iterations: int = 5,
                                    robust: bool = True, stream=None):
    """orbfe_global_bundle_adjustment_device on torch CUDA tensors: camera (88) u8 = one POSE_CAMERA_DTYPE record, poses (K,12) f32,
    fixed (K) u8, points (M,stride) u8 whose records start with the position (or (M,3) f32), edges (E,24) u8 = LBA_EDGE_DTYPE, listed
    point by point with keyframes ascending; poses_out (K,12) f32, points_out (M,3) f32, result (40) u8 = one BA_RESULT_DTYPE record,
    workspace: u8 of at least gba_workspace_bytes(K, M, E) bytes.  Synchronous on `stream` (a torch.cuda.Stream, or None for the NULL
    stream): the host reads one control record per trial."""
    stride = int(points.shape[1]) * int(points.element_size()) if points.dim() == 2 else 12
    _lib.check(_lib.lib().orbfe_global_bundle_adjustment_device(
        _lib.ptr(camera), _lib.ptr(poses), _lib.ptr(fixed), int(poses.shape[0]), _lib.ptr(points), stride, int(points.shape[0]),
        _lib.ptr(edges), int(edges.shape[0]), int(n_iterations), BA_ROBUST if robust else 0, _lib.ptr(poses_out), _lib.ptr(points_out),
        _lib.ptr(result), _lib.ptr(workspace), int(workspace.numel()) * int(workspace.element_size()), _lib.stream_handle(stream)),
        "orbfe_global_bundle_adjustment_device")


def essential_graph_envelope_blocks(n_kf: int, fixed, edges) -> int:
    """orbfe_essential_graph_envelope_blocks: the blocks of the row envelope of a graph of n_kf vertices in their order; fixed:
    (n_kf) uint8 or None, edges: EG_EDGE_DTYPE."""
    edges = np.ascontiguousarray(edges, EG_EDGE_DTYPE).reshape(-1)
    fixed = None if fixed is None else np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    if fixed is not None and len(fixed) != int(n_kf):
        raise ValueError("fixed must have one entry per vertex")
    n = C.c_int64(0)
    _lib.check(_lib.lib().orbfe_essential_graph_envelope_blocks(int(n_kf), _lib.ptr(fixed) if fixed is not None and len(fixed) else None,
                                                                _lib.ptr(edges) if len(edges) else None, len(edges), C.byref(n)),
               "orbfe_essential_graph_envelope_blocks")
    return int(n.value)


def essential_graph_workspace_bytes(P: int, kf_cap: int, edge_cap: int, env_cap: int) -> int:
    """orbfe_essential_graph_workspace_bytes: the workspace of a batch of P graphs of at most kf_cap vertices, edge_cap edges and
    env_cap envelope blocks each."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().orbfe_essential_graph_workspace_bytes(int(P), int(kf_cap), int(edge_cap), int(env_cap), C.byref(n)),
               "orbfe_essential_graph_workspace_bytes")
    return int(n.value)


def essential_graph(vertices, edges, fix_scale: bool = False):
    """Optimizer::OptimizeEssentialGraph of one graph from its vertex and edge lists on.  vertices: EG_VERTEX_DTYPE (n_kf), ascending
    by mnId; edges: EG_EDGE_DTYPE (n_edges); fix_scale: the SE3 form.  Returns (sim3_out, poses_out, result): EG_SIM3_DTYPE (n_kf), the
    corrected Siw; (n_kf, 12) float32, rows of [R | t / s]; one EG_RESULT_DTYPE record."""
    vertices = np.ascontiguousarray(vertices, EG_VERTEX_DTYPE).reshape(-1)
    edges = np.ascontiguousarray(edges, EG_EDGE_DTYPE).reshape(-1)
    sim3_out = np.zeros(len(vertices), EG_SIM3_DTYPE)
    poses_out = np.zeros((len(vertices), 12), np.float32)
    res = np.zeros(1, EG_RESULT_DTYPE)
    opt = lambda a: _lib.ptr(a) if len(a) else None
    _lib.check(_lib.lib().orbfe_essential_graph(opt(vertices), len(vertices), opt(edges), len(edges), EG_FIX_SCALE if fix_scale else 0,
                                                opt(sim3_out), opt(poses_out), _lib.ptr(res)), "orbfe_essential_graph")
    return sim3_out, poses_out, res[0]


def essential_graph_batch(problems, vertices, edges, kf_cap, edge_cap, env_cap, sim3_out, poses_out, result, workspace,
                          fix_scale: bool = False, stream=None):
    """orbfe_essential_graph_batch_device on torch CUDA tensors: problems (P,16) u8 = EG_PROBLEM_DTYPE, vertices (K,136) u8 =
    EG_VERTEX_DTYPE, edges (E,12) u8 = EG_EDGE_DTYPE; sim3_out (K,8) f64 = EG_SIM3_DTYPE, poses_out (K,12) f32, result (P,48) u8 =
    EG_RESULT_DTYPE, workspace: u8 of at least essential_graph_workspace_bytes(P, kf_cap, edge_cap, env_cap) bytes.  fix_scale holds for
    every problem.  Rows no problem names are not written.  stream: a torch.cuda.Stream, or None for the NULL stream."""
    P = int(problems.shape[0])
    _lib.check(_lib.lib().orbfe_essential_graph_batch_device(
        P, _lib.ptr(problems), _lib.ptr(vertices), _lib.ptr(edges), int(kf_cap), int(edge_cap), int(env_cap),
        EG_FIX_SCALE if fix_scale else 0, _lib.ptr(sim3_out), _lib.ptr(poses_out), _lib.ptr(result), _lib.ptr(workspace),
        int(workspace.numel()) * int(workspace.element_size()), _lib.stream_handle(stream)), "orbfe_essential_graph_batch_device")


def essential_graph_grid(vertices, edges, fix_scale: bool = False):
    """orbfe_essential_graph_grid: essential_graph for ONE graph across the whole device, with envelopes of up to
    EGRID_MAX_ENVELOPE_BLOCKS blocks.  Arguments and return value as essential_graph's; a graph both take gives the same bytes."""
    vertices = np.ascontiguousarray(vertices, EG_VERTEX_DTYPE).reshape(-1)
    edges = np.ascontiguousarray(edges, EG_EDGE_DTYPE).reshape(-1)
    sim3_out = np.zeros(len(vertices), EG_SIM3_DTYPE)
    poses_out = np.zeros((len(vertices), 12), np.float32)
    res = np.zeros(1, EG_RESULT_DTYPE)
    opt = lambda a: _lib.ptr(a) if len(a) else None
    _lib.check(_lib.lib().orbfe_essential_graph_grid(opt(vertices), len(vertices), opt(edges), len(edges), EG_FIX_SCALE if fix_scale else 0,
                                                     opt(sim3_out), opt(poses_out), _lib.ptr(res)), "orbfe_essential_graph_grid")
    return sim3_out, poses_out, res[0]


def essential_graph_grid_workspace_bytes(kf_cap: int, edge_cap: int, env_cap: int) -> int:
    """orbfe_essential_graph_grid_workspace_bytes: the workspace of one graph of at most kf_cap vertices, edge_cap edges and env_cap
    envelope blocks (essential_graph_envelope_blocks states a graph's)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().orbfe_essential_graph_grid_workspace_bytes(int(kf_cap), int(edge_cap), int(env_cap), C.byref(n)),
               "orbfe_essential_graph_grid_workspace_bytes")
    return int(n.value)


def essential_graph_grid_device(vertices, edges, sim3_out, poses_out, result, workspace, fix_scale: bool = False, stream=None):
    """orbfe_essential_graph_grid_device on torch CUDA tensors: vertices (K,136) u8 = EG_VERTEX_DTYPE, edges (E,12) u8 = EG_EDGE_DTYPE;
    sim3_out (K,8) f64 = EG_SIM3_DTYPE, poses_out (K,12) f32, result (48) u8 = one EG_RESULT_DTYPE record, workspace: u8 of at least
    essential_graph_grid_workspace_bytes(K, E, blocks) bytes for a graph of `blocks` envelope blocks -- a graph it does not hold comes
    back with status EG_REFUSED.  Synchronous on `stream` (a torch.cuda.Stream, or None for the NULL stream): the host reads one
    control record per trial."""
    _lib.check(_lib.lib().orbfe_essential_graph_grid_device(
        _lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(edges), int(edges.shape[0]), EG_FIX_SCALE if fix_scale else 0,
        _lib.ptr(sim3_out), _lib.ptr(poses_out), _lib.ptr(result), _lib.ptr(workspace),
        int(workspace.numel()) * int(workspace.element_size()), _lib.stream_handle(stream)), "orbfe_essential_graph_grid_device")


def gba_update_map(poses, parent, kf_gba_row, gba_poses, half_baseline, points, point_gba_row, ref, gba_points):
    """orbfe_gba_update_map: the map update of LoopClosing::RunGlobalBundleAdjustment (L/src/LoopClosing.cc:648-703) behind
    global_bundle_adjustment.  poses: (n_kf, 12) float32, the current Tcw; parent: (n_kf) int32, the row of the spanning-tree parent or -1
    for an origin; kf_gba_row: (n_kf) int32, the row of gba_poses (m, 12) of an optimised keyframe or -1; half_baseline: mHalfBaseline;
    points: (n, 3) float32; point_gba_row: (n) int32, the row of gba_points (q, 3) of an optimised point or -1; ref: (n) int32, the row of
    the reference keyframe or -1 for a point that stays.  Returns (keyframes, points_out, result): GBA_MAP_KEYFRAME_DTYPE (n_kf) with
    the new Tcw, SetPose's Twc and Cw and a GBA_MAP_KF_* status; (n, 3) float32; one GBA_MAP_RESULT_DTYPE record."""
    poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    kf_gba_row = np.ascontiguousarray(kf_gba_row, np.int32).reshape(-1)
    gba_poses = np.ascontiguousarray(np.asarray(gba_poses, np.float32).reshape(-1, 12))
    points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    point_gba_row = np.ascontiguousarray(point_gba_row, np.int32).reshape(-1)
    ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
    gba_points = np.ascontiguousarray(np.asarray(gba_points, np.float32).reshape(-1, 3))
    if len(parent) != len(poses) or len(kf_gba_row) != len(poses):
        raise ValueError("poses, parent and kf_gba_row must have one entry per keyframe")
    if len(point_gba_row) != len(points) or len(ref) != len(points):
        raise ValueError("points, point_gba_row and ref must have one entry per point")
    kf_out = np.zeros(len(poses), GBA_MAP_KEYFRAME_DTYPE)
    points_out = np.zeros_like(points)
    res = np.zeros(1, GBA_MAP_RESULT_DTYPE)
    opt = lambda a: _lib.ptr(a) if len(a) else None
    _lib.check(_lib.lib().orbfe_gba_update_map(opt(poses), opt(parent), opt(kf_gba_row), len(poses), opt(gba_poses), len(gba_poses),
                                               float(half_baseline), opt(points), opt(point_gba_row), opt(ref), len(points),
                                               opt(gba_points), len(gba_points), opt(kf_out), opt(points_out), _lib.ptr(res)),
               "orbfe_gba_update_map")
    return kf_out, points_out, res[0]


def gba_update_map_device(poses, parent, kf_gba_row, gba_poses, half_baseline, points, point_gba_row, ref, gba_points, kf_out,
                          points_out, result, stream=None):
    """orbfe_gba_update_map_device on torch CUDA tensors: poses (K,12) f32, parent (K) i32, kf_gba_row (K) i32, gba_poses (G,12) f32 --
    the poses_out of global_bundle_adjustment_device as it lies --, points (M,stride) u8 whose records start with the position (or
    (M,3) f32), point_gba_row (M) i32, ref (M) i32, gba_points (Q,3) f32 -- its points_out --; kf_out (K,112) u8 =
    GBA_MAP_KEYFRAME_DTYPE, points_out (M,3) f32, result (32) u8 = one GBA_MAP_RESULT_DTYPE record.  Asynchronous on `stream` (a
    torch.cuda.Stream, or None for the NULL stream)."""
    stride = int(points.shape[1]) * int(points.element_size()) if points.dim() == 2 else 12
    _lib.check(_lib.lib().orbfe_gba_update_map_device(
        _lib.ptr(poses), _lib.ptr(parent), _lib.ptr(kf_gba_row), int(poses.shape[0]), _lib.ptr(gba_poses), int(gba_poses.shape[0]),
        float(half_baseline), _lib.ptr(points), stride, _lib.ptr(point_gba_row), _lib.ptr(ref), int(points.shape[0]), _lib.ptr(gba_points),
        int(gba_points.shape[0]), _lib.ptr(kf_out), _lib.ptr(points_out), _lib.ptr(result), _lib.stream_handle(stream)),
        "orbfe_gba_update_map_device")
