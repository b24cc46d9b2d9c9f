"""PnPsolver over the C ABI of liborbfe.so (L/src/PnPsolver.cc, L/ = Source/Libraries/ORB_SLAM2/): the EPnP RANSAC of
Tracking::Relocalization between search_by_bow and the pose optimisation.

pnp_solve evaluates H hypotheses of one problem on host arrays, pnp_solve_batch P problems in three launches on device tensors;
both run pnp_kernels.hip, there is no CPU path.  The caller draws the minimal sets (draw_minimal_sets) and owns the random state.
The solver's sequential surface -- iterate(n) in chunks, find -- is a cursor over the per-hypothesis counts and the refine records
of the best-so-far hypotheses: iterate_replay.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import (PNP_CAMERA_DTYPE, PNP_DIAG_DTYPE, PNP_HYPOTHESIS_DTYPE, PNP_POINT_DTYPE, PNP_REFINE_DTYPE, PNP_RESULT_DTYPE)

__all__ = ["PNP_POINT_DTYPE", "PNP_CAMERA_DTYPE", "PNP_HYPOTHESIS_DTYPE", "PNP_REFINE_DTYPE", "PNP_RESULT_DTYPE", "PNP_DIAG_DTYPE",
           "PnpSolution", "IterateCall", "ransac_parameters", "draw_minimal_sets", "pack_points", "pnp_camera", "pnp_solve", "pnp_solve_batch",
           "iterate_replay", "inlier_bits"]

PnpSolution = namedtuple("PnpSolution", "result mask hyps words refines refine_words diag refine_diag")
# one iterate() call: the hypothesis it returned at (at exhaustion the best one; -1 without a pose), the refine record whose pose it
# returned (-1: the hypothesis' own pose, or none), nInliers, bNoMore, mnIterations after the call
IterateCall = namedtuple("IterateCall", "returned refine n_inliers no_more consumed")


def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """SetRansacParameters (:119-151) for N correspondences: (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon) after the call."""
    mi, it, eps = C.c_int32(0), C.c_int32(0), C.c_float(0)
    _lib.check(_lib.lib().orbfe_pnp_ransac_parameters(int(N), float(probability), int(min_inliers), int(max_iterations), int(min_set),
                                                      float(np.float32(epsilon)), C.byref(mi), C.byref(it), C.byref(eps)),
               "orbfe_pnp_ransac_parameters")
    return mi.value, it.value, np.float32(eps.value)


def draw_minimal_sets(n, H, rng) -> np.ndarray:
    """H minimal sets as PnPsolver::iterate draws them (:184-197): four times an index r = RandomInt(0, len - 1) into the list of
    available indices, whose entry r is then replaced by the last one.  rng: a callable k -> integer in [0, k) (for the reference's
    stream: lambda k: int(rand() / (RAND_MAX + 1.0) * k)), or a numpy Generator.  Returns int32 (H, 4)."""
    if n < 4:
        raise ValueError("a minimal set needs four correspondences")
    below = (lambda k: int(rng.integers(k))) if hasattr(rng, "integers") else rng
    out = np.empty((H, 4), np.int32)
    for h in range(H):
        avail = list(range(n))
        for i in range(4):
            r = below(len(avail))
            if not 0 <= r < len(avail):
                raise ValueError(f"the generator returned {r} for a list of {len(avail)}")
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def pack_points(Xw, uv, level_sigma2, th2=5.991) -> np.ndarray:
    """orbfe_pnp_point records from (n, 3) world positions, (n, 2) undistorted keypoints and mvLevelSigma2[octave] per point;
    max_err = sigma2 * th2 in float (:155)."""
    Xw = np.asarray(Xw, np.float32).reshape(-1, 3)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    p = np.zeros(len(Xw), PNP_POINT_DTYPE)
    p["Xw"], p["u"], p["v"] = Xw, uv[:, 0], uv[:, 1]
    p["max_err"] = np.asarray(level_sigma2, np.float32) * np.float32(th2)
    return p


def pnp_camera(fx, fy, cx, cy) -> np.ndarray:
    c = np.zeros(1, PNP_CAMERA_DTYPE)
    c["fx"], c["fy"], c["cx"], c["cy"] = fx, fy, cx, cy
    return c


def pnp_solve(camera, points, sets, min_inliers, want_records=True, want_diag=True) -> PnpSolution:
    """orbfe_pnp_solve.  camera: pnp_camera(...); points: PNP_POINT_DTYPE (n); sets: int32 (H, 4); min_inliers: the adjusted value of
    ransac_parameters.  Returns PnpSolution: one PNP_RESULT_DTYPE record, uint64 (ceil(n / 64)) = the inlier words of the returned
    pose, then PNP_HYPOTHESIS_DTYPE (H), uint64 (H, ceil(n / 64)), PNP_REFINE_DTYPE (H), uint64 (H, ceil(n / 64)), PNP_DIAG_DTYPE (H)
    twice (None when not wanted)."""
    cam = np.ascontiguousarray(camera, PNP_CAMERA_DTYPE).reshape(1)
    points = np.ascontiguousarray(points, PNP_POINT_DTYPE).reshape(-1)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
    n, H = len(points), len(sets)
    nw = (n + 63) // 64
    hyps = np.zeros(H, PNP_HYPOTHESIS_DTYPE) if want_records else None
    words = np.zeros((H, nw), np.uint64) if want_records else None
    refines = np.zeros(H, PNP_REFINE_DTYPE) if want_records else None
    rwords = np.zeros((H, nw), np.uint64) if want_records else None
    diag = np.zeros(H, PNP_DIAG_DTYPE) if want_diag else None
    rdiag = np.zeros(H, PNP_DIAG_DTYPE) if want_diag else None
    result, mask = np.zeros(1, PNP_RESULT_DTYPE), np.zeros(max(nw, 1), np.uint64)
    _lib.check(_lib.lib().orbfe_pnp_solve(_lib.ptr(cam), _lib.ptr(points), n, _lib.ptr(sets), 4, H, int(min_inliers), _lib.ptr(hyps),
                                          _lib.ptr(words), _lib.ptr(refines), _lib.ptr(rwords), _lib.ptr(diag), _lib.ptr(rdiag),
                                          _lib.ptr(result), _lib.ptr(mask)), "orbfe_pnp_solve")
    return PnpSolution(result[0], mask[:nw], hyps, words, refines, rwords, diag, rdiag)


def pnp_solve_batch(camera, points, n, sets, H, min_inliers, hyps, words, refines, refine_words, result, result_mask, diag=None,
                    refine_diag=None, stream=None):
    """orbfe_pnp_solve_batch_device on torch CUDA tensors: camera (P,16) u8 = PNP_CAMERA_DTYPE, points (P,cap,24) u8, n (P) i32, sets
    (P,h_cap,4) i32, H / min_inliers (P) i32, hyps / refines (P,h_cap,112) u8, words / refine_words (P,h_cap,ceil(cap/64)) i64, result
    (P,80) u8, result_mask (P,ceil(cap/64)) i64, diag / refine_diag (P,h_cap,640) u8 or None.  stream: a torch.cuda.Stream, or None
    for the NULL stream."""
    P, cap, h_cap = int(points.shape[0]), int(points.shape[1]), int(sets.shape[1])
    _lib.check(_lib.lib().orbfe_pnp_solve_batch_device(P, _lib.ptr(camera), _lib.ptr(points), _lib.ptr(n), cap, _lib.ptr(sets), _lib.ptr(H),
                                                       h_cap, _lib.ptr(min_inliers), _lib.ptr(hyps), _lib.ptr(words), _lib.ptr(refines),
                                                       _lib.ptr(refine_words), _lib.ptr(diag), _lib.ptr(refine_diag), _lib.ptr(result),
                                                       _lib.ptr(result_mask), _lib.stream_handle(stream)), "orbfe_pnp_solve_batch_device")


def iterate_replay(hyps, refines, min_inliers, chunk, max_iterations):
    """The calls iterate(chunk) makes over hypotheses whose counts are hyps['n_inliers'] (or a plain sequence of counts), in order,
    until one reports bNoMore (:163-246).  refines: per hypothesis the count of its Refine() (refines['n_inliers'], or a plain
    sequence); only the entries of hypotheses that become the best so far are read.  The loop condition is
    `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`: the first call runs until mnIterations reaches
    max_iterations unless it returns earlier, a call beyond that runs exactly `chunk` iterations.  An iteration whose count is >=
    min_inliers makes its hypothesis the best when its count is strictly larger, and runs Refine() on the best in either case; a
    refine with count > min_inliers returns.  The cursor and the best persist across calls, so after a returning call a later
    qualifying hypothesis returns the same refine again.  Returns one IterateCall per call.  Raises IndexError when the walk runs
    past the evaluated hypotheses."""
    counts = [int(c) for c in (hyps["n_inliers"] if hasattr(hyps, "dtype") and hyps.dtype.names else hyps)]
    rcounts = [int(c) for c in (refines["n_inliers"] if hasattr(refines, "dtype") and refines.dtype.names else refines)]
    if chunk < 1 or max_iterations < 1:
        raise ValueError("an empty chunk or no iterations")
    calls, cursor, best, best_count = [], 0, -1, 0
    while True:
        taken, call = 0, None
        while cursor < max_iterations or taken < chunk:
            if cursor >= len(counts):
                raise IndexError(f"iterate walks to hypothesis {cursor}, {len(counts)} were evaluated")
            h, cursor, taken = cursor, cursor + 1, taken + 1
            if counts[h] >= min_inliers:
                if counts[h] > best_count:
                    best, best_count = h, counts[h]
                if rcounts[best] > min_inliers:
                    call = IterateCall(h, best, rcounts[best], False, cursor)
                    break
        if call is None:      # the loop ran out: mnIterations >= mRansacMaxIts holds by its condition (:232)
            call = IterateCall(best, -1, best_count, True, cursor) if best_count >= min_inliers else IterateCall(-1, -1, 0, True, cursor)
        calls.append(call)
        if call.no_more:
            return calls


def inlier_bits(words, n) -> np.ndarray:
    """uint64 (..., ceil(n / 64)) inlier words -> bool (..., n)"""
    w = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)
