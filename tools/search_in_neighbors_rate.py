#!/usr/bin/env python3
"""Host-clock time of the Fuse calls of LocalMapping::SearchInNeighbors for one keyframe, four ways, alternating in one process after
warm-up (every timed call ends with its own stream synchronisation):
  A  K single orbfe_kf_search calls, as ORBmatcher::Fuse makes them (upload of the target and of all points, grid, three launches, wait)
  B  orbfe_fuse_batch_create + one full search + destroy
  C  one full search on a resident handle
  D  a repair search of 8 points in the targets 1 .. K-1
on K targets of 2 000 keypoints and 1 000 / 2 000 candidate points (synthetic: noisy projections with descriptors 0 .. 60 bits away).
B's rows are compared with A's byte for byte first.  Also counts the repair searches mapping.search_in_neighbors makes on the census
scenes of tests/np_neighbors.py and on a seeded 30-target scene.  Prints one JSON line; --out writes the Markdown table.

usage: python tools/search_in_neighbors_rate.py [--shapes 10x1000,30x1000,...] [--reps 10] [--warmup 2] [--ab-lib NAME]
       [--out profiles/search_in_neighbors.md]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refactored_orb_slam2_amd import _lib, mapping  # noqa: E402
from refactored_orb_slam2_amd.matcher import FrameView, FuseBatch  # noqa: E402
from tests import np_neighbors as N  # noqa: E402

W, H, N_KEYS = 640, 480, 2000


def camera(k, th=3.0):
    a = 0.01 * ((k % 7) - 3)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    t = np.array([0.05 * ((k % 5) - 2), 0.03 * ((k % 3) - 1), 0.02 * (k % 4)], np.float32)
    cam = np.zeros(1, _lib.KF_CAMERA_DTYPE)
    cam["R"][0], cam["t"][0] = R.reshape(9), t
    cam["Ow"][0] = -(R.T.astype(np.float64) @ t.astype(np.float64))
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"] = 517.3, 516.5, 318.6, 255.3, 40.0
    cam["min_x"], cam["max_x"], cam["min_y"], cam["max_y"] = 0, W, 0, H
    cam["log_scale_factor"] = np.float32(np.log(1.2))
    cam["n_levels"] = N.N_LEVELS
    cam["th"] = th
    cam["scale_factors"][0, :N.N_LEVELS] = N.SCALE_FACTORS
    return cam


def make_world(K, n_points, seed=7):
    rng = np.random.default_rng(seed)
    pts = np.zeros(n_points, _lib.KF_POINT_DTYPE)
    pos = np.stack([rng.uniform(-3.5, 3.5, n_points), rng.uniform(-2.5, 2.5, n_points), rng.uniform(4, 10, n_points)], 1).astype(np.float32)
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1))
    pts["pos"], pts["normal"] = pos, (pos / dist[:, None]).astype(np.float32)
    pts["max_distance"] = (dist * rng.uniform(1.0, 1.9, n_points)).astype(np.float32)
    pts["min_distance"] = (dist * rng.uniform(0.3, 0.9, n_points)).astype(np.float32)
    pts["desc"] = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    targets = []
    for k in range(K):
        cam = camera(k)
        R = cam["R"][0].reshape(3, 3).astype(np.float64); t = cam["t"][0].astype(np.float64)
        pc = pos.astype(np.float64) @ R.T + t
        u = 517.3 * pc[:, 0] / pc[:, 2] + 318.6; v = 516.5 * pc[:, 1] / pc[:, 2] + 255.3
        keys = np.zeros(N_KEYS, _lib.KP_DTYPE)
        src = rng.integers(0, n_points, N_KEYS)
        own = rng.random(N_KEYS) < 0.7                                     # keypoints near a projection; the rest anywhere
        keys["x"] = np.where(own, u[src] + rng.normal(0, 1.2, N_KEYS), rng.uniform(5, W - 5, N_KEYS))
        keys["y"] = np.where(own, v[src] + rng.normal(0, 1.2, N_KEYS), rng.uniform(5, H - 5, N_KEYS))
        keys["x"], keys["y"] = np.clip(keys["x"], 1, W - 2), np.clip(keys["y"], 1, H - 2)
        d3 = np.sqrt(((pos[src] - cam["Ow"][0]).astype(np.float64) ** 2).sum(1))
        lvl = np.clip(np.ceil(np.log(pts["max_distance"][src] / d3) / np.log(1.2)), 0, N.N_LEVELS - 1).astype(np.int32)
        keys["octave"] = np.maximum(0, lvl - rng.integers(0, 3, N_KEYS))
        keys["size"], keys["response"], keys["class_id"] = 31, 20, -1
        flips = rng.integers(0, 61, N_KEYS)                                # expected number of flipped bits per keypoint
        desc = pts["desc"][src] ^ np.packbits(rng.random((N_KEYS, 256)) < (flips / 256.0)[:, None], axis=1)
        ur = np.where(rng.random(N_KEYS) < 0.5, keys["x"] - 40.0 / np.maximum(pc[src, 2], 0.1), -1).astype(np.float32) if k % 2 else None
        targets.append(dict(keys=keys, desc=desc, u_right=ur, inv=N.INV_LEVEL_SIGMA2.copy()))
    return pts, targets


def big_scene(seed=30, K=30, n_sites=60):
    """a seeded 30-target map for the repair count: every site has a query point and, in 3 .. 6 targets, a keypoint a few bits away, half
    of them held by a point of their own (so Replace chains run through the targets)"""
    b = N.Builder(seed, K=K, stereo_target=7)
    rng = np.random.default_rng(seed)
    for _ in range(n_sites):
        s = b.site()
        p = b.point(s, N.D()); b.keypoint(b.current, s, N.D(), p)
        for kf in sorted(rng.choice(K, int(rng.integers(3, 7)), replace=False)):
            d = N.D(*[int(x) for x in rng.choice(256, int(rng.integers(1, 25)), replace=False)])
            q = b.point(s, d) if rng.random() < 0.5 else -1
            b.keypoint(int(kf), s, d, q, dx=float(rng.integers(-1, 2)))
    return dict(map=b.m, current=b.current, targets=list(range(K)))


def repair_counts():
    out = {}
    for name, s in [(f"census {sd}", N.build_scene(sd)) for sd in N.SCENE_SEEDS] + [("30 targets, 60 sites", big_scene())]:
        c = N.clone(s)
        log, n_fused, _ = N.sequential(c["map"], c["current"], c["targets"])
        d = N.clone(s)
        r = mapping.search_in_neighbors(d["map"], d["current"], d["targets"])
        assert r["log"] == log and d["map"].state() == c["map"].state(), name
        out[name] = dict(targets=len(s["targets"]), n_fused=n_fused, replaces=sum(op[0] == "replace" for op in log), n_full=r["n_full"],
                         n_repair=r["n_repair"], round_trips_before=len(s["targets"]) + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10x1000,30x1000,100x1000,10x2000,30x2000,100x2000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-repair-counts", action="store_true")
    ap.add_argument("--ab-lib", default=None, help='a tools/ab_build.sh <name> "-DFUSE_WAVE_ROWS=n" fuse_kernels.hip build (rows per wave)')
    a = ap.parse_args()
    if a.ab_lib:
        _lib.LIB_PATH = os.path.join(_lib.CSRC, "_ab", "liborbfe_%s.so" % a.ab_lib)
    L = _lib.lib()
    results = []
    for shape in a.shapes.split(","):
        K, n = (int(x) for x in shape.split("x"))
        pts, targets = make_world(K, n)
        views = [FrameView(t["keys"], t["desc"], 0, W, 0, H, t["u_right"]) for t in targets]
        cams = np.concatenate([camera(k) for k in range(K)])
        invs = [t["inv"] for t in targets]
        single = np.zeros((K, n), _lib.KF_RESULT_DTYPE)
        nm = C.c_int(0)

        def run_a():
            for k in range(K):
                _lib.check(L.orbfe_kf_search(C.byref(views[k].c), _lib.ptr(invs[k]), _lib.ptr(cams[k:k + 1]), _lib.ptr(pts), n, _lib.KF_FUSE, 0, 50,
                                             None, _lib.ptr(single[k]), C.byref(nm)), "orbfe_kf_search")
        rows_b = np.zeros((K, n), _lib.KF_RESULT_DTYPE)

        def run_b():
            b = FuseBatch(views, cams, invs, _lib.KF_FUSE)
            b.search(pts, results=rows_b)
            b.close()
        resident = FuseBatch(views, cams, invs, _lib.KF_FUSE)
        rows_c = np.zeros((K, n), _lib.KF_RESULT_DTYPE)
        idx = np.arange(8, dtype=np.int32) * (n // 8)

        def run_c():
            resident.search(pts, results=rows_c)

        def run_d():
            resident.search(pts[idx], idx, 1, results=rows_c)
        run_a(); run_b(); run_c()
        assert rows_b.tobytes() == single.tobytes() and rows_c.tobytes() == single.tobytes(), "batch rows differ from the single calls"
        times = {x: [] for x in "ABCD"}
        for r in range(a.warmup + a.reps):
            for name, fn in (("A", run_a), ("B", run_b), ("C", run_c), ("D", run_d)):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[name].append(dt)
        resident.close()
        rec = dict(K=K, n_points=n, keypoints=N_KEYS, rows_with_candidate=int((single["best_idx"] >= 0).sum()),
                   rows_past_prologue=int((single["level"] >= 0).sum()),
                   bytes_targets=K * N_KEYS * (28 + 32 + 4), bytes_points=n * 72, bytes_results=K * n * 24)
        for x in "ABCD":
            v = np.array(times[x])
            rec[x] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))
        rec["A_over_B"] = rec["A"]["median_ms"] / rec["B"]["median_ms"]
        rec["A_over_C"] = rec["A"]["median_ms"] / rec["C"]["median_ms"]
        results.append(rec)
    out = dict(shapes=results)
    if not a.no_repair_counts:
        out["repairs"] = repair_counts()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write("| K | points | A: K single calls (ms) | B: create + search (ms) | C: resident search (ms) | D: repair of 8 (ms) | A / B | A / C | "
                    "bytes: targets + points + results |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in results:
                cell = lambda x: f"{r[x]['median_ms']:.3f} ({r[x]['min_ms']:.3f} .. {r[x]['max_ms']:.3f})"   # noqa: E731
                f.write(f"| {r['K']} | {r['n_points']} | {cell('A')} | {cell('B')} | {cell('C')} | {cell('D')} | {r['A_over_B']:.1f} | "
                        f"{r['A_over_C']:.1f} | {r['bytes_targets']} + {r['bytes_points']} + {r['bytes_results']} |\n")
            if "repairs" in out:
                f.write("\n| scene | targets | replaces | full searches | repair searches | round trips before |\n|---|---|---|---|---|---|\n")
                for name, r in out["repairs"].items():
                    f.write(f"| {name} | {r['targets']} | {r['replaces']} | {r['n_full']} | {r['n_repair']} | {r['round_trips_before']} |\n")


if __name__ == "__main__":
    main()
