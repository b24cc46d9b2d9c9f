#!/usr/bin/env python3
"""Time of the global bundle adjustment across the device (orbfe_global_bundle_adjustment_device) per call and per trial, split by
phase, at 64, 256, 1 024 and 2 047 free keyframes (2 048 keyframes, the first one fixed) with about 100 points per keyframe and about 5 edges per point, as
LoopClosing::RunGlobalBundleAdjustment calls it (10 iterations, not robust).  At 64 free keyframes orbfe_bundle_adjustment, the
one-workgroup form, is timed on the same scene and the outputs are compared byte for byte.  Writes a Markdown table
(profiles/global_bundle_adjustment.md) and prints one JSON line.

Per call: wall time around the synchronous call on device-resident data, warm-ups, the median of the repetitions with minimum and
maximum.  Per phase: one more call with orbfe_debug_gba_phases switched on, which brackets every phase with stream events and
synchronises after each -- the sums are device times of the phases and that call is not among the timed ones.  The scenes are
generated here, vectorised (tests/np_lba.make_scene loops in Python): a camera moving along z, tracks of 2 - 6 consecutive
keyframes, a fifth of the points with one more observation 10 - 40 keyframes earlier.

usage: python tools/gba_rate.py [--sizes 64,256,1024,2048] [--reps 3] [--warmup 1] [--out profiles/global_bundle_adjustment.md]
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
from refactored_orb_slam2_amd import _lib, optimizer  # noqa: E402

PHASES = ("plan", "build", "Dinv / Schur", "factorisation", "solves", "update / chi2", "control read-back")
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, mbf=386.1448)


def scene(n_free, points_per_kf=100, seed=1):
    rng = np.random.default_rng(seed)
    n_free = min(n_free, _lib.GBA_MAX_KEYFRAMES - 1)       # keyframe 0 is fixed: the largest map has 2 047 free keyframes
    n_kf, n_pt = n_free + 1, points_per_kf * n_free
    centre = np.zeros((n_kf, 3))
    centre[:, 2] = 0.9 * np.arange(n_kf)
    centre[1:, :2] = np.cumsum(rng.normal(size=(n_kf - 1, 2)) * 0.02, axis=0)
    poses_true = np.zeros((n_kf, 12))
    poses_true[:, [0, 5, 10]] = 1.0
    poses_true[:, [3, 7, 11]] = -centre
    last = rng.integers(1, n_kf, n_pt)
    span = np.minimum(rng.integers(2, 7, n_pt), last + 1)
    z = rng.uniform(4, 40, n_pt)
    u, v = rng.uniform(20, 1220, n_pt), rng.uniform(20, 360, n_pt)
    X = centre[last] + np.stack([(u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z], 1)
    back = np.where(rng.uniform(size=n_pt) < 0.2, rng.integers(10, 41, n_pt), 0)
    offs = np.concatenate([-(span - 1 + back)[:, None], np.arange(-5, 1)[None, :].repeat(n_pt, 0)], 1)     # the long one first: keyframes ascend
    kf = last[:, None] + offs
    keep = (kf >= 0) & np.concatenate([(back > 0)[:, None], np.arange(-5, 1)[None, :] > -span[:, None]], 1)
    pt = np.arange(n_pt)[:, None].repeat(7, 1)
    kf, pt = kf[keep], pt[keep]
    c = X[pt] - centre[kf]
    ok = c[:, 2] > 1.0
    kf, pt, c = kf[ok], pt[ok], c[ok]
    octave = rng.integers(0, 8, len(kf))
    sc = 1.2 ** octave
    pu = c[:, 0] / c[:, 2] * CAM["fx"] + CAM["cx"] + rng.normal(size=len(kf)) * 0.7 * sc
    pv = c[:, 1] / c[:, 2] * CAM["fy"] + CAM["cy"] + rng.normal(size=len(kf)) * 0.7 * sc
    pr = pu - CAM["mbf"] / c[:, 2]
    mono = (rng.uniform(size=len(kf)) < 0.3) | (pr < 0)
    edges = np.zeros(len(kf), _lib.LBA_EDGE_DTYPE)
    edges["kf"], edges["point"], edges["u"], edges["v"] = kf, pt, pu, pv
    edges["u_right"], edges["inv_sigma2"] = np.where(mono, -1.0, pr), 1.0 / sc ** 2
    poses = poses_true.copy()
    poses[1:, [3, 7, 11]] += rng.normal(size=(n_free, 3)) * 0.02
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    points = (X + rng.normal(size=X.shape) * 0.05).astype(np.float32)
    return dict(poses=poses.astype(np.float32), fixed=fixed, points=points, edges=edges)


def spread(times):
    t = np.array(times) * 1e3
    return dict(median_ms=round(float(np.median(t)), 2), min_ms=round(float(t.min()), 2), max_ms=round(float(t.max()), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,2048")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "global_bundle_adjustment.md"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam_rec = optimizer.pose_camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["mbf"], [1.0])
    L = _lib.lib()
    out = {}
    for n_free in [int(x) for x in args.sizes.split(",")]:
        s = scene(n_free)
        n_kf, n_pt, n_e = len(s["poses"]), len(s["points"]), len(s["edges"])
        n_free = n_kf - 1
        d = [up(cam_rec.view(np.uint8)), up(s["poses"]), up(s["fixed"]), up(s["points"]), up(s["edges"].view(np.uint8).reshape(-1, 24))]
        poses_out, points_out = torch.zeros((n_kf, 12), dtype=torch.float32, device=dev), torch.zeros((n_pt, 3), dtype=torch.float32, device=dev)
        result = torch.zeros((40,), dtype=torch.uint8, device=dev)
        ws_bytes = optimizer.gba_workspace_bytes(n_kf, n_pt, n_e)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)

        def call():
            optimizer.global_bundle_adjustment_device(d[0], d[1], d[2], d[3], d[4], poses_out, points_out, result, ws,
                                                      n_iterations=args.iterations, robust=False)
        times = []
        for k in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if k >= args.warmup:
                times.append(time.perf_counter() - t0)
        res = result.cpu().numpy().view(_lib.BA_RESULT_DTYPE)[0]
        L.orbfe_debug_gba_phases(1, None)
        call()
        ms = (C.c_float * 7)()
        L.orbfe_debug_gba_phases(0, ms)
        trials = int(res["trials"])
        row = dict(free_keyframes=n_free, points=n_pt, edges=n_e, workspace_mb=round(ws_bytes / 2 ** 20, 1), rounds=int(res["rounds"]),
                   iterations=int(res["iterations"]), trials=trials, chi2=[round(float(res["chi2_first"]), 1), round(float(res["chi2_final"]), 1)],
                   call=spread(times), ms_per_trial=round(float(np.median(times)) * 1e3 / max(trials, 1), 2),
                   phase_ms={p: round(float(m), 2) for p, m in zip(PHASES, ms)})
        if n_free <= _lib.LBA_MAX_FREE:        # the one-workgroup form on the same scene: host forms of both, the same staging
            host = {}
            for name, f in (("one_workgroup", optimizer.bundle_adjustment), ("grid", optimizer.global_bundle_adjustment)):
                t, got = [], None
                for k in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    got = f(cam_rec, s["poses"], s["fixed"], s["points"], s["edges"], args.iterations, False)
                    if k >= args.warmup:
                        t.append(time.perf_counter() - t0)
                host[name] = (spread(t), got)
            same = all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(host["one_workgroup"][1], host["grid"][1]))
            row["host_form"] = dict(one_workgroup=host["one_workgroup"][0], grid=host["grid"][0], bytes_equal=same,
                                    grid_over_one_workgroup=round(host["grid"][0]["median_ms"] / host["one_workgroup"][0]["median_ms"], 3))
        out[str(n_free)] = row
        del ws
        torch.cuda.empty_cache()
    lines = ["# Global bundle adjustment across the device: time per call, per trial and per phase", "",
             f"`tools/gba_rate.py`: {args.iterations} iterations, not robust, {args.warmup} warm-up and {args.reps} timed calls of",
             "`orbfe_global_bundle_adjustment_device` per size (wall time around the synchronous call, median with minimum and maximum);",
             "the phase columns are stream-event sums of one more call (`orbfe_debug_gba_phases`), in ms over the whole call.", "",
             "| free keyframes | points | edges | workspace MB | iterations | trials | call ms (min .. max) | ms / trial | " + " | ".join(PHASES) + " |",
             "|---|---|---|---|---|---|---|---|" + "---|" * len(PHASES)]
    for r in out.values():
        c = r["call"]
        lines.append(f"| {r['free_keyframes']} | {r['points']} | {r['edges']} | {r['workspace_mb']} | {r['iterations']} | {r['trials']} | "
                     f"{c['median_ms']} ({c['min_ms']} .. {c['max_ms']}) | {r['ms_per_trial']} | " + " | ".join(str(r["phase_ms"][p]) for p in PHASES) + " |")
    for r in out.values():
        if "host_form" in r:
            h = r["host_form"]
            lines += ["", f"At {r['free_keyframes']} free keyframes, host forms on the same scene (upload and download included): one workgroup "
                      f"(`orbfe_bundle_adjustment`) {h['one_workgroup']['median_ms']} ms ({h['one_workgroup']['min_ms']} .. {h['one_workgroup']['max_ms']}), "
                      f"grid (`orbfe_global_bundle_adjustment`) {h['grid']['median_ms']} ms ({h['grid']['min_ms']} .. {h['grid']['max_ms']}): "
                      f"ratio grid / one workgroup {h['grid_over_one_workgroup']}; outputs byte-equal: {h['bytes_equal']}."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
