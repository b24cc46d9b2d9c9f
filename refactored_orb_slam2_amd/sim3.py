"""Sim3Solver over the C ABI of liborbfe.so (L/src/Sim3Solver.cc, L/ = Source/Libraries/ORB_SLAM2/): the RANSAC of
LoopClosing::ComputeSim3 between search_by_bow and the Sim3 search.

sim3_solve evaluates H hypotheses of one problem on host arrays, sim3_solve_batch P problems in one launch pair on device tensors;
both run sim3_kernels.hip, there is no CPU path.  The caller draws the triples (draw_triples) and owns the random state.  The
solver's sequential surface -- iterate(n) in chunks, find -- is a cursor over the per-hypothesis counts: iterate_replay.

correct_points is the map correction of LoopClosing::CorrectLoop and of Optimizer::OptimizeEssentialGraph: every point through
to[ref]^-1 . from[ref] (egraph_kernels.hip, one thread per point); correct_points_device the same on device tensors, reading the
sim3_out of optimizer.essential_graph_batch where it lies.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import EG_SIM3_DTYPE
from ._lib import SIM3_HYPOTHESIS_DTYPE, SIM3_PAIR_DTYPE, SIM3_RESULT_DTYPE, SIM3_VIEW_DTYPE

__all__ = ["SIM3_VIEW_DTYPE", "SIM3_PAIR_DTYPE", "SIM3_HYPOTHESIS_DTYPE", "SIM3_RESULT_DTYPE", "sim3_view", "sim3_pairs", "max_error",
           "ransac_iterations", "draw_triples", "iterate_replay", "sim3_solve", "sim3_solve_batch", "EG_SIM3_DTYPE", "correct_points",
           "correct_points_device"]


def sim3_view(Rcw, tcw, fx, fy, cx, cy) -> np.ndarray:
    """One orbfe_sim3_view record: GetRotation(), GetTranslation() and mK of a KeyFrame."""
    v = np.zeros(1, SIM3_VIEW_DTYPE)
    v["Rcw"][0], v["tcw"][0] = np.asarray(Rcw, np.float32).reshape(9), np.asarray(tcw, np.float32).reshape(3)
    v["fx"], v["fy"], v["cx"], v["cy"] = fx, fy, cx, cy
    return v


def max_error(level_sigma2):
    """mvnMaxError of Sim3Solver.cc:85-86: 9.210 * sigma2 in double, truncated as the reference's vector<size_t> does, as float."""
    return np.floor(9.210 * np.asarray(level_sigma2, np.float32).astype(np.float64)).astype(np.float32)


def sim3_pairs(Xw1, Xw2, max_err1, max_err2) -> np.ndarray:
    """orbfe_sim3_pair records from (n, 3) world positions and the two truncated bounds (max_error)."""
    Xw1 = np.asarray(Xw1, np.float32).reshape(-1, 3)
    p = np.zeros(len(Xw1), SIM3_PAIR_DTYPE)
    p["Xw1"], p["Xw2"] = Xw1, np.asarray(Xw2, np.float32).reshape(-1, 3)
    p["max_err1"], p["max_err2"] = max_err1, max_err2
    return p


def ransac_iterations(N, probability=0.99, min_inliers=6, max_iterations=300) -> int:
    """mRansacMaxIts after SetRansacParameters(probability, min_inliers, max_iterations) for N correspondences."""
    rc = _lib.lib().orbfe_sim3_ransac_iterations(int(N), float(probability), int(min_inliers), int(max_iterations))
    if rc < 0:
        _lib.check(rc, "orbfe_sim3_ransac_iterations")
    return rc


def draw_triples(n, H, rng) -> np.ndarray:
    """H triples as Sim3Solver::iterate draws them (:159-172): three times an index r = RandomInt(0, len - 1) into the list of
    available indices, whose entry r is then replaced by the last one.  rng: a callable k -> integer in [0, k) (for the reference's
    stream: lambda k: int(rand() / (RAND_MAX + 1.0) * k)), or a numpy Generator.  Returns int32 (H, 3)."""
    if n < 3:
        raise ValueError("a triple needs three correspondences")
    below = (lambda k: int(rng.integers(k))) if hasattr(rng, "integers") else rng
    out = np.empty((H, 3), np.int32)
    for h in range(H):
        avail = list(range(n))
        for i in range(3):
            r = below(len(avail))
            if not 0 <= r < len(avail):
                raise ValueError(f"the generator returned {r} for a list of {len(avail)}")
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def iterate_replay(counts, min_inliers, chunk, max_iterations=None):
    """The calls iterate(chunk) makes over hypotheses whose inlier counts are `counts`, in order, until it returns a transform or
    reports bNoMore (:155-199).  max_iterations (mRansacMaxIts) defaults to len(counts) and must not exceed it.  Returns one tuple
    per call: (returned, n_inliers, no_more, consumed) -- returned is the index of the first hypothesis of that call with count >
    min_inliers or -1, consumed the value of mnIterations after the call.  A call that returns does not set bNoMore even on the last
    iteration (:186-192 leaves before :196); the caller may go on calling, and the list continues until bNoMore."""
    counts = [int(c) for c in counts]
    max_its = len(counts) if max_iterations is None else int(max_iterations)
    if max_its > len(counts) or chunk < 1:
        raise ValueError("max_iterations beyond the evaluated hypotheses, or an empty chunk")
    calls, cursor = [], 0
    while True:
        returned, n_inl, taken = -1, 0, 0
        while cursor < max_its and taken < chunk:
            h, cursor, taken = cursor, cursor + 1, taken + 1
            if counts[h] > min_inliers:
                returned, n_inl = h, counts[h]
                break
        no_more = returned < 0 and cursor >= max_its
        calls.append((returned, n_inl, no_more, cursor))
        if no_more:
            return calls


def sim3_solve(view1, view2, pairs, triples, fix_scale, min_inliers, want_hypotheses=True, want_words=True):
    """orbfe_sim3_solve.  view*: sim3_view(...); pairs: SIM3_PAIR_DTYPE (n); triples: int32 (H, 3).  Returns (result, mask, hyps,
    words): one SIM3_RESULT_DTYPE record, uint64 (ceil(n / 64)) = the inlier words of result['best'], SIM3_HYPOTHESIS_DTYPE (H) and
    uint64 (H, ceil(n / 64)) (None when not wanted)."""
    v1, v2 = np.ascontiguousarray(view1, SIM3_VIEW_DTYPE).reshape(1), np.ascontiguousarray(view2, SIM3_VIEW_DTYPE).reshape(1)
    pairs = np.ascontiguousarray(pairs, SIM3_PAIR_DTYPE).reshape(-1)
    triples = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    n, H = len(pairs), len(triples)
    nw = (n + 63) // 64
    hyps = np.zeros(H, SIM3_HYPOTHESIS_DTYPE) if want_hypotheses else None
    words = np.zeros((H, nw), np.uint64) if want_words else None
    result, mask = np.zeros(1, SIM3_RESULT_DTYPE), np.zeros(max(nw, 1), np.uint64)
    _lib.check(_lib.lib().orbfe_sim3_solve(_lib.ptr(v1), _lib.ptr(v2), _lib.ptr(pairs), n, _lib.ptr(triples), H, int(bool(fix_scale)),
                                           int(min_inliers), _lib.ptr(hyps), _lib.ptr(words), _lib.ptr(result), _lib.ptr(mask)),
               "orbfe_sim3_solve")
    return result[0], mask[:nw], hyps, words


def sim3_solve_batch(view1, view2, pairs, n, triples, H, fix_scale, min_inliers, hyps, words, result, result_mask, stream=None):
    """orbfe_sim3_solve_batch_device on torch CUDA tensors: view1 / view2 (P,64) u8 = SIM3_VIEW_DTYPE, pairs (P,cap,32) u8, n (P) i32,
    triples (P,h_cap,3) i32, H / fix_scale / min_inliers (P) i32, hyps (P,h_cap,64) u8, words (P,h_cap,ceil(cap/64)) i64, result
    (P,128) u8, result_mask (P,ceil(cap/64)) i64.  stream: a torch.cuda.Stream, or None for the NULL stream."""
    P, cap, h_cap = int(pairs.shape[0]), int(pairs.shape[1]), int(triples.shape[1])
    _lib.check(_lib.lib().orbfe_sim3_solve_batch_device(P, _lib.ptr(view1), _lib.ptr(view2), _lib.ptr(pairs), _lib.ptr(n), cap,
                                                        _lib.ptr(triples), _lib.ptr(H), h_cap, _lib.ptr(fix_scale), _lib.ptr(min_inliers),
                                                        _lib.ptr(hyps), _lib.ptr(words), _lib.ptr(result), _lib.ptr(result_mask),
                                                        _lib.stream_handle(stream)), "orbfe_sim3_solve_batch_device")


def inlier_bits(words, n) -> np.ndarray:
    """uint64 (..., ceil(n / 64)) inlier words -> bool (..., n)"""
    w = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


def correct_points(points, ref, sim3_from, sim3_to) -> np.ndarray:
    """orbfe_sim3_correct_points: points (n, 3) float32; ref (n) int32, a row of the two tables or < 0 for a point that goes through;
    sim3_from / sim3_to: EG_SIM3_DTYPE (n_tables), vScw and the corrected Siw.  Returns (n, 3) float32:
    sim3_to[ref]^-1 .map( sim3_from[ref].map(P) ), rounded to float once."""
    points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
    a = np.ascontiguousarray(sim3_from, EG_SIM3_DTYPE).reshape(-1)
    b = np.ascontiguousarray(sim3_to, EG_SIM3_DTYPE).reshape(-1)
    if len(ref) != len(points) or len(a) != len(b):
        raise ValueError("one ref per point and two tables of the same length")
    out = np.zeros_like(points)
    opt = lambda x: _lib.ptr(x) if len(x) else None
    _lib.check(_lib.lib().orbfe_sim3_correct_points(opt(points), len(points), opt(ref), opt(a), opt(b), len(a), opt(out)),
               "orbfe_sim3_correct_points")
    return out


def correct_points_device(points, ref, sim3_from, sim3_to, points_out, n_tables=None, stream=None):
    """orbfe_sim3_correct_points_device on torch CUDA tensors: points (n,3) f32, ref (n) i32, sim3_from (K,8) f64 = EG_SIM3_DTYPE or
    (K,136) u8 = EG_VERTEX_DTYPE (its Scw is read in place), sim3_to (K,8) f64, points_out (n,3) f32."""
    stride = int(sim3_from.shape[1]) * int(sim3_from.element_size())
    K = int(sim3_to.shape[0]) if n_tables is None else int(n_tables)
    _lib.check(_lib.lib().orbfe_sim3_correct_points_device(_lib.ptr(points), int(points.shape[0]), _lib.ptr(ref), _lib.ptr(sim3_from), stride,
                                                           _lib.ptr(sim3_to), K, _lib.ptr(points_out), _lib.stream_handle(stream)),
               "orbfe_sim3_correct_points_device")
