#!/usr/bin/env python3
"""Wall time of the neighbour loop of LocalMapping::CreateNewMapPoints for one keyframe: pKF1 with 2 000 keypoints against K = 10
neighbours (the chain scene of tests/np_mapping.py at that size: 40 vocabulary buckets, 60 % stereo keypoints, every neighbour past
the baseline gate), three ways in one process, alternating, warm, medians over the repetitions, in one JSON line:

  chain_ms    one orbfe_create_new_map_points call: pKF1 staged once, search + triangulation per neighbour on one stream, one copy-out
  search_ms   the path without it: K calls of orbfe_search_for_triangulation, each with its upload and synchronisation.  The
              triangulation and the update of has_mpA between neighbours, which that path leaves to the host, are NOT in this figure
              (every call sees the initial mask), so it is a lower bound of what that path costs
  kernel_ms   the triangulation kernel alone: orbfe_triangulate_matches_batch_device for the K neighbours in one launch on the
              chain's own matches, device-resident, HIP events

Host times are host clocks around the synchronous calls; the ctypes arguments are built once, outside the timed region.  The chain's
records are checked against the K searches + triangulations of the first neighbour before anything is timed.
profiles/create_new_map_points.md.

A/B builds: ORBFE_AB_LIB=<name> (refactored_orb_slam2_amd/csrc/_ab/liborbfe_<name>.so).

usage: python tools/mapping_rate.py [--keypoints 2000] [--neighbors 10] [--reps 40] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib  # noqa: E402
if os.environ.get("ORBFE_AB_LIB"): _lib.LIB_PATH = os.path.join(_lib.CSRC, "_ab", "liborbfe_%s.so" % os.environ["ORBFE_AB_LIB"])
from refactored_orb_slam2_amd import mapping  # noqa: E402
from refactored_orb_slam2_amd.matcher import featvec_arrays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--neighbors", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from tests import np_mapping as M

    n, K = args.keypoints, args.neighbors
    rel = [((0.15 * (1 + k % 3), 0.02, 0.6 + 0.25 * k), 0.03 - 0.01 * (k % 5)) for k in range(K)]
    sc = M.make_chain_scene(seed=70, n=n, rel=rel)
    A, nbs = sc["A"], sc["neighbors"]
    L, p = _lib.lib(), _lib.ptr

    # ---- arguments of the chain, built once
    nodesA, nnA, idxA = featvec_arrays(A["groups"])
    keep, rec = [], np.zeros(K, _lib.TRI_NEIGHBOR_DTYPE)
    for k, nb in enumerate(nbs):
        nodes, nn, idx = featvec_arrays(nb["groups"])
        ep = np.ascontiguousarray(nb["epipolar"], _lib.EPIPOLAR_DTYPE)
        keep.append((nodes, nn, idx, ep))
        r = rec[k]
        r["keys"], r["desc"], r["has_mp"] = nb["keys"].ctypes.data, nb["desc"].ctypes.data, nb["has_mp"].ctypes.data
        r["u_right"], r["depth"] = nb["u_right"].ctypes.data, nb["depth"].ctypes.data
        r["nodes"], r["idx"], r["n"], r["n_nodes"] = C.cast(nodes, C.c_void_p).value, idx.ctypes.data, n, nn
        r["view"], r["ep"], r["median_depth"] = nb["view"][0], ep[0], nb["median_depth"]
    pts = np.zeros((K, n), _lib.NEW_POINT_DTYPE)
    nm, nnew, has = np.zeros(K, np.int32), np.zeros(K, np.int32), A["has_mp"].copy()
    cnodesA = C.cast(nodesA, C.c_void_p)

    def chain():
        has[:] = A["has_mp"]
        _lib.check(L.orbfe_create_new_map_points(p(A["keys"]), p(A["desc"]), p(A["u_right"]), p(A["depth"]), p(has), n, cnodesA, nnA,
                                                 p(idxA), p(A["view"]), p(rec), K, 0, 0, 1, p(pts), p(nm), p(nnew)), "chain")

    mA, cnt = np.zeros(n, np.int32), C.c_int(0)

    def searches():
        for k, nb in enumerate(nbs):
            nodes, nn, idx, ep = keep[k]
            _lib.check(L.orbfe_search_for_triangulation(p(A["keys"]), p(A["desc"]), p(A["u_right"]), p(A["has_mp"]), n, cnodesA, nnA, p(idxA),
                                                        p(nb["keys"]), p(nb["desc"]), p(nb["u_right"]), p(nb["has_mp"]), n,
                                                        C.cast(nodes, C.c_void_p), nn, p(idx), p(ep), 0, 1, p(mA), C.byref(cnt)), "search")

    # ---- the chain's first neighbour == search + host-form triangulation (nothing has a new map point yet)
    chain()
    nodes, nn, idx, ep = keep[0]
    _lib.check(L.orbfe_search_for_triangulation(p(A["keys"]), p(A["desc"]), p(A["u_right"]), p(A["has_mp"]), n, cnodesA, nnA, p(idxA),
                                                p(nbs[0]["keys"]), p(nbs[0]["desc"]), p(nbs[0]["u_right"]), p(nbs[0]["has_mp"]), n,
                                                C.cast(nodes, C.c_void_p), nn, p(idx), p(ep), 0, 1, p(mA), C.byref(cnt)), "search")
    first = mapping.triangulate_matches(A["view"], A["keys"], A["u_right"], A["depth"], nbs[0]["view"], nbs[0]["keys"], nbs[0]["u_right"],
                                        nbs[0]["depth"], mA)[0]
    if first.tobytes() != pts[0].tobytes() or cnt.value != nm[0]:
        raise SystemExit("the chain's first neighbour differs from search + triangulation: nothing is timed")
    if (nm < 0).any():
        raise SystemExit("a neighbour was gated out: the scene is not what this tool means to time")

    t_chain, t_search = [], []
    for k in range(args.warmup + args.reps):
        for fn, acc in ((chain, t_chain), (searches, t_search)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                acc.append(dt)
    chain()

    # ---- the kernel alone, on the chain's matches
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a)).to(dev)
    view2 = np.concatenate([nb["view"] for nb in nbs])
    d = [up(A["view"]), up(A["keys"]), up(A["u_right"]), up(A["depth"]), up(np.full(K, n, np.int32)), up(view2),
         up(np.stack([nb["keys"] for nb in nbs])), up(np.stack([nb["u_right"] for nb in nbs])), up(np.stack([nb["depth"] for nb in nbs])),
         up(np.full(K, n, np.int32)), up(np.ascontiguousarray(pts["idx2"]))]
    out = torch.zeros((K, n, 44), dtype=torch.uint8, device=dev)
    n_new = torch.zeros(K, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    t_kernel = []
    with torch.cuda.stream(s):
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            mapping.triangulate_matches_batch(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], out, n_new, s)
            e1.record(s)
            e1.synchronize()
            if k >= args.warmup:
                t_kernel.append(e0.elapsed_time(e1))
    s.synchronize()
    same = out.cpu().numpy().reshape(K, n * 44).tobytes() == pts.tobytes()
    med = lambda t: round(float(np.median(t)), 4)
    print(json.dumps({"keypoints": n, "neighbors": K, "reps": args.reps, "matches": int(nm.sum()), "new_points": int(nnew.sum()),
                      "chain_ms": med(t_chain), "chain_min_ms": round(float(np.min(t_chain)), 4), "search_ms": med(t_search),
                      "search_min_ms": round(float(np.min(t_search)), 4), "chain_over_search": round(med(t_chain) / med(t_search), 3),
                      "kernel_ms": med(t_kernel), "kernel_min_ms": round(float(np.min(t_kernel)), 4),
                      "kernel_equals_chain_bytes": bool(same)}))


if __name__ == "__main__":
    main()
