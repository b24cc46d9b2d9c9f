"""Initializer::Initialize over the C ABI of liborbfe.so (L/src/Initializer.cc, L/ = Source/Libraries/ORB_SLAM2/): the two-view
geometry between search_for_initialization and a first monocular map.

initialize evaluates H homography and H fundamental hypotheses of one problem on host arrays, initialize_batch P problems in one
set of launches on device tensors; both run initializer_kernels.hip, there is no CPU path.  The caller draws the sets of eight
(draw_sets) and owns the random state.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import INIT_CANDIDATE_DTYPE, INIT_HYPOTHESIS_DTYPE, INIT_PARAMS_DTYPE, INIT_RESULT_DTYPE
from ._lib import INITIAL_MAP_RESULT_DTYPE, POSE_CAMERA_DTYPE

__all__ = ["INIT_PARAMS_DTYPE", "INIT_HYPOTHESIS_DTYPE", "INIT_CANDIDATE_DTYPE", "INIT_RESULT_DTYPE", "init_params", "draw_sets",
           "initialize", "initialize_batch", "workspace_bytes", "bits",
           "INITIAL_MAP_RESULT_DTYPE", "create_initial_map", "create_initial_map_batch", "initial_map_workspace_bytes"]


def init_params(fx, fy, cx, cy, sigma=1.0, min_parallax=1.0, min_triangulated=50) -> np.ndarray:
    """One orbfe_init_params record; the defaults are Tracking's (Initializer(frame, 1.0, 200)) and Initialize's (1.0, 50)."""
    p = np.zeros(1, INIT_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = fx, fy, cx, cy
    p["sigma"], p["min_parallax"], p["min_triangulated"] = sigma, min_parallax, min_triangulated
    return p


def draw_sets(N, H, rng) -> np.ndarray:
    """H sets of eight match indices as Initialize draws them (:80-93): eight times an index r = RandomInt(0, len - 1) into the list
    of available indices, whose entry r is then replaced by the last one.  rng: a callable k -> integer in [0, k) (for the
    reference's stream: lambda k: int(rand() / (RAND_MAX + 1.0) * k)), or a numpy Generator.  Returns int32 (H, 8)."""
    if N < 8:
        raise ValueError("a set needs eight matches")
    below = (lambda k: int(rng.integers(k))) if hasattr(rng, "integers") else rng
    out = np.empty((H, 8), np.int32)
    for h in range(H):
        avail = list(range(N))
        for j in range(8):
            r = below(len(avail))
            if not 0 <= r < len(avail):
                raise ValueError(f"the generator returned {r} for a list of {len(avail)}")
            out[h, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def bits(words, n) -> np.ndarray:
    """uint64 (..., >= ceil(n / 64)) words -> bool (..., n)"""
    w = np.ascontiguousarray(words, np.uint64)
    b = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return b[..., :n].astype(bool)


def initialize(params, keys1, keys2, matches12, sets, want_hypotheses=False, want_words=False, want_candidates=True) -> dict:
    """orbfe_initializer_initialize.  params: init_params(...); keys1 (n1, 2) / keys2 (n2, 2): mvKeysUn points of the reference and
    the current frame; matches12 (n1): index into keys2 or -1; sets: int32 (H, 8) into the match list.  Returns a dict: result (one
    INIT_RESULT_DTYPE record), P3D (n1, 3) float32, triangulated (n1) bool, inliers (N) bool over the match list, and -- when wanted,
    else None -- hyps_h / hyps_f (H) INIT_HYPOTHESIS_DTYPE, words_h / words_f (H, ceil(n1 / 64)) uint64, candidates (8)."""
    par = np.ascontiguousarray(params, INIT_PARAMS_DTYPE).reshape(1)
    k1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
    m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    if len(m12) != len(k1):
        raise ValueError("matches12 has one entry per keypoint of the reference frame")
    n1, n2, H = len(k1), len(k2), len(sets)
    nw = (n1 + 63) // 64
    result = np.zeros(1, INIT_RESULT_DTYPE)
    P3D, tri, inl = np.zeros((n1, 3), np.float32), np.zeros(max(nw, 1), np.uint64), np.zeros(max(nw, 1), np.uint64)
    hh = np.zeros(H, INIT_HYPOTHESIS_DTYPE) if want_hypotheses else None
    hf = np.zeros(H, INIT_HYPOTHESIS_DTYPE) if want_hypotheses else None
    wh = np.zeros((H, nw), np.uint64) if want_words else None
    wf = np.zeros((H, nw), np.uint64) if want_words else None
    cands = np.zeros(8, INIT_CANDIDATE_DTYPE) if want_candidates else None
    _lib.check(_lib.lib().orbfe_initializer_initialize(_lib.ptr(par), _lib.ptr(k1), n1, _lib.ptr(k2), n2, _lib.ptr(m12), _lib.ptr(sets), H,
                                                       _lib.ptr(result), _lib.ptr(P3D), _lib.ptr(tri), _lib.ptr(inl), _lib.ptr(hh), _lib.ptr(hf),
                                                       _lib.ptr(wh), _lib.ptr(wf), _lib.ptr(cands)), "orbfe_initializer_initialize")
    N = int(result["n_matches"][0])
    return {"result": result[0], "P3D": P3D, "triangulated": bits(tri, n1), "inliers": bits(inl, N), "hyps_h": hh, "hyps_f": hf,
            "words_h": wh, "words_f": wf, "candidates": cands, "triangulated_words": tri[:nw], "inlier_words": inl[:nw]}


def workspace_bytes(P, cap) -> int:
    """orbfe_initializer_workspace_bytes"""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().orbfe_initializer_workspace_bytes(int(P), int(cap), C.byref(n)), "orbfe_initializer_workspace_bytes")
    return int(n.value)


def initialize_batch(params, keys1, n1, keys2, n2, matches12, sets, H, result, P3D, triangulated, inlier_words, hyps, words, candidates,
                     workspace, stream=None):
    """orbfe_initializer_initialize_batch_device on torch CUDA tensors: params (P,32) u8 = INIT_PARAMS_DTYPE, keys1 / keys2 (P,cap,2)
    f32, n1 / n2 (P) i32, matches12 (P,cap) i32, sets (P,h_cap,8) i32, H (P) i32, result (P,224) u8, P3D (P,cap,3) f32, triangulated /
    inlier_words (P,ceil(cap/64)) i64, hyps (P,2,h_cap,64) u8, words (P,2,h_cap,ceil(cap/64)) i64, candidates (P,8,64) u8, workspace
    (>= workspace_bytes(P, cap)) u8.  stream: a torch.cuda.Stream, or None for the NULL stream."""
    P, cap, h_cap = int(keys1.shape[0]), int(keys1.shape[1]), int(sets.shape[1])
    _lib.check(_lib.lib().orbfe_initializer_initialize_batch_device(
        P, _lib.ptr(params), _lib.ptr(keys1), _lib.ptr(n1), _lib.ptr(keys2), _lib.ptr(n2), cap, _lib.ptr(matches12), _lib.ptr(sets),
        _lib.ptr(H), h_cap, _lib.ptr(result), _lib.ptr(P3D), _lib.ptr(triangulated), _lib.ptr(inlier_words), _lib.ptr(hyps), _lib.ptr(words),
        _lib.ptr(candidates), _lib.ptr(workspace), int(workspace.numel() * workspace.element_size()), _lib.stream_handle(stream)),
        "orbfe_initializer_initialize_batch_device")


def create_initial_map(camera, keys1, keys2, matches12, P3D, triangulated, init_result, octaves1, octaves2, pose1=None, n_iterations=20,
                       q=2, min_points=100, want_unscaled=False) -> dict:
    """orbfe_create_initial_map: Tracking::CreateInitialMapMonocular from what initialize() returned.  camera: optimizer.pose_camera(...)
    with the pyramid's inv_level_sigma2; keys1 / keys2 / matches12 as given to initialize(); P3D (n1, 3), triangulated (n1) bool or the
    uint64 words, init_result: initialize()'s result record; octaves1 (n1) / octaves2 (n2): the octave of every keypoint; pose1: the
    initial keyframe's (12) [R | t], None for the identity.  Returns a dict: result (one INITIAL_MAP_RESULT_DTYPE record), poses (2, 12),
    points (n1, 3) in match-index order with zero rows where there is no point, index (n_points) the matches that became points, and --
    when want_unscaled -- poses_ba / points_ba, the same before the rescale."""
    cam = np.ascontiguousarray(camera, POSE_CAMERA_DTYPE).reshape(1)
    k1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
    n1, n2 = len(k1), len(k2)
    m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    p3d = np.ascontiguousarray(np.asarray(P3D, np.float32).reshape(-1, 3))
    o1, o2 = np.ascontiguousarray(octaves1, np.int32).reshape(-1), np.ascontiguousarray(octaves2, np.int32).reshape(-1)
    if len(m12) != n1 or len(p3d) != n1 or len(o1) != n1 or len(o2) != n2:
        raise ValueError("matches12, P3D and octaves1 have one entry per keypoint of the initial frame, octaves2 one per keypoint of the current")
    tri = np.asarray(triangulated)
    if tri.dtype != np.uint64:
        b = np.zeros(((n1 + 63) // 64) * 64, np.uint8)
        b[:n1] = tri.astype(bool).reshape(-1)
        tri = np.packbits(b.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64) if n1 else np.zeros(0, np.uint64)
    words = np.zeros(max((n1 + 63) // 64, 1), np.uint64)
    words[:(n1 + 63) // 64] = tri[:(n1 + 63) // 64]
    init = np.ascontiguousarray(init_result, _lib.INIT_RESULT_DTYPE).reshape(1)
    p1 = None if pose1 is None else np.ascontiguousarray(np.asarray(pose1, np.float32).reshape(12))
    result = np.zeros(1, INITIAL_MAP_RESULT_DTYPE)
    poses, points, index = np.zeros((2, 12), np.float32), np.zeros((n1, 3), np.float32), np.full(n1, -1, np.int32)
    poses_ba = np.zeros((2, 12), np.float32) if want_unscaled else None
    points_ba = np.zeros((n1, 3), np.float32) if want_unscaled else None
    opt = lambda a: _lib.ptr(a) if a is not None and len(a) else None
    _lib.check(_lib.lib().orbfe_create_initial_map(_lib.ptr(cam), opt(k1), n1, opt(k2), n2, opt(m12), opt(p3d), _lib.ptr(words), _lib.ptr(init),
                                                   opt(o1), opt(o2), _lib.ptr(p1), int(n_iterations), int(q), int(min_points),
                                                   _lib.ptr(poses), opt(points), opt(index), _lib.ptr(poses_ba), opt(points_ba),
                                                   _lib.ptr(result)), "orbfe_create_initial_map")
    return {"result": result[0], "poses": poses, "points": points, "index": index[:int(result["n_points"][0])], "poses_ba": poses_ba,
            "points_ba": points_ba}


def initial_map_workspace_bytes(P, cap) -> int:
    """orbfe_initial_map_workspace_bytes"""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().orbfe_initial_map_workspace_bytes(int(P), int(cap), C.byref(n)), "orbfe_initial_map_workspace_bytes")
    return int(n.value)


def create_initial_map_batch(camera, keys1, n1, keys2, n2, matches12, P3D, triangulated, init_result, octaves1, octaves2, poses, points,
                             index, result, workspace, pose1=None, poses_ba=None, points_ba=None, n_iterations=20, q=2, min_points=100,
                             stream=None):
    """orbfe_create_initial_map_batch_device on torch CUDA tensors: camera (88) u8 = one POSE_CAMERA_DTYPE record; keys1 / keys2
    (P,cap,2) f32, n1 / n2 (P) i32, matches12 (P,cap) i32, P3D (P,cap,3) f32, triangulated (P,ceil(cap/64)) i64 words and init_result
    (P,224) u8 exactly as initialize_batch reads and writes them; octaves1 / octaves2 (P,cap) i32; pose1 (P,12) f32 or None.  Outputs:
    poses (P,2,12) f32, points (P,cap,3) f32, index (P,cap) i32, poses_ba / points_ba the same or None, result (P,72) u8 =
    INITIAL_MAP_RESULT_DTYPE; workspace: u8 of at least initial_map_workspace_bytes(P, cap) bytes."""
    P, cap = int(keys1.shape[0]), int(keys1.shape[1])
    _lib.check(_lib.lib().orbfe_create_initial_map_batch_device(
        P, _lib.ptr(camera), _lib.ptr(keys1), _lib.ptr(n1), _lib.ptr(keys2), _lib.ptr(n2), cap, _lib.ptr(matches12), _lib.ptr(P3D),
        _lib.ptr(triangulated), _lib.ptr(init_result), _lib.ptr(octaves1), _lib.ptr(octaves2), _lib.ptr(pose1), int(n_iterations), int(q),
        int(min_points), _lib.ptr(poses), _lib.ptr(points), _lib.ptr(index), _lib.ptr(poses_ba), _lib.ptr(points_ba), _lib.ptr(result),
        _lib.ptr(workspace), int(workspace.numel()) * int(workspace.element_size()), _lib.stream_handle(stream)),
        "orbfe_create_initial_map_batch_device")
