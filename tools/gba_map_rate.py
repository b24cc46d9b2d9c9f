#!/usr/bin/env python3
"""Device time of the map update behind the global bundle adjustment (orbfe_gba_update_map_device) on device-resident data:
  loop     the map a loop closure leaves: 2 048 optimised keyframes in a sequence, 64 more that local mapping inserted meanwhile as
           a chain under the last one, 1 048 575 points -- 85 % optimised, 14 % carried by a reference keyframe, 1 % bad
  chain    the worst chain the limit admits: one optimised origin and 65 535 keyframes in one chain under it, rows in chain order
  shuffled the same chain with the rows shuffled
  fan      one optimised origin and 65 535 children
each of the last three with 1 025 points.  The call is asynchronous; its device time is the time between two stream events around it,
warm-ups first, then the median of the repetitions with minimum and maximum.  Every scene's outputs are compared byte for byte with
the numpy reading (tests/np_gba_map.rule) once.  Writes a Markdown table (profiles/gba_map_update.md) and prints one JSON line.

usage: python tools/gba_map_rate.py [--scenes loop,chain,shuffled,fan] [--reps 10] [--warmup 2] [--out profiles/gba_map_update.md]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refactored_orb_slam2_amd import _lib, optimizer  # noqa: E402
from tests import np_gba_map as M  # noqa: E402


def loop_scene():
    n_opt, n_new, n_pt = _lib.GBA_MAX_KEYFRAMES, 64, _lib.GBA_MAX_POINTS
    parent = list(range(-1, n_opt + n_new - 1))
    s = M.make_scene(1, parent, [True] * n_opt + [False] * n_new, 3)
    rng = np.random.default_rng(2)
    kind = rng.choice(3, n_pt, p=[0.85, 0.14, 0.01])
    n_take = int((kind == 0).sum())
    s["points"] = rng.uniform(-50, 50, (n_pt, 3)).astype(np.float32)
    s["gba_points"] = rng.uniform(-50, 50, (n_take, 3)).astype(np.float32)
    s["point_gba_row"] = np.full(n_pt, -1, np.int32)
    s["point_gba_row"][kind == 0] = rng.permutation(n_take)
    s["ref"] = np.where(kind == 2, -1, rng.integers(0, n_opt + n_new, n_pt)).astype(np.int32)
    return s


SCENES = {
    "loop": loop_scene,
    "chain": lambda: M.make_scene(3, *M.chain(_lib.GBA_MAP_MAX_KEYFRAMES - 1), 1025, shuffle=False),
    "shuffled": lambda: M.make_scene(4, *M.chain(_lib.GBA_MAP_MAX_KEYFRAMES - 1), 1025),
    "fan": lambda: M.make_scene(5, *M.fan(_lib.GBA_MAP_MAX_KEYFRAMES - 1), 1025),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="loop,chain,shuffled,fan")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_map_update.md"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}
    for name in args.scenes.split(","):
        s = SCENES[name]()
        n, m = len(s["poses"]), len(s["points"])
        d = {k: up(s[k]) for k in ("poses", "parent", "kf_gba_row", "gba_poses", "points", "point_gba_row", "ref", "gba_points")}
        kf_out = torch.zeros((n, 112), dtype=torch.uint8, device=dev)
        pts_out = torch.zeros((m, 3), dtype=torch.float32, device=dev)
        result = torch.zeros((32,), dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream()

        def call():
            optimizer.gba_update_map_device(d["poses"], d["parent"], d["kf_gba_row"], d["gba_poses"], float(s["half_baseline"]), d["points"],
                                            d["point_gba_row"], d["ref"], d["gba_points"], kf_out, pts_out, result, stream=st)
        torch.cuda.synchronize()
        times = []
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if k >= args.warmup:
                times.append(e0.elapsed_time(e1))
        res = result.cpu().numpy().view(_lib.GBA_MAP_RESULT_DTYPE)[0]
        want_kf, want_pts, want_res = M.rule(s)
        same = (kf_out.cpu().numpy().tobytes() == want_kf.tobytes() and pts_out.cpu().numpy().tobytes() == want_pts.tobytes()
                and {f: int(res[f]) for f in M.RESULT_FIELDS} == want_res)
        t = np.array(times)
        out[name] = dict(keyframes=n, points=m, optimised=int(res["n_optimised"]), propagated=int(res["n_propagated"]),
                         rounds=int(res["rounds"]), taken=int(res["n_taken"]), moved=int(res["n_moved"]), left=int(res["n_left"]),
                         median_ms=round(float(np.median(t)), 3), min_ms=round(float(t.min()), 3), max_ms=round(float(t.max()), 3),
                         us_per_round=round(float(np.median(t)) * 1e3 / max(int(res["rounds"]), 1), 3), bytes_equal_the_reading=bool(same))
    lines = ["# Map update behind the global bundle adjustment: device time of the device form", "",
             f"`python tools/gba_map_rate.py --scenes {args.scenes} --reps {args.reps} --warmup {args.warmup}`: the time between two stream",
             "events around one asynchronous `orbfe_gba_update_map_device` call on device-resident data (the clearing of the result record,",
             "three launches over the keyframes, one over the points), median with minimum and maximum.", "",
             "| scene | keyframes | optimised | propagated | rounds | points | taken | moved | left | ms (min .. max) | us / round | bytes equal the reading |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out.items():
        lines.append(f"| {name} | {r['keyframes']} | {r['optimised']} | {r['propagated']} | {r['rounds']} | {r['points']} | {r['taken']} | "
                     f"{r['moved']} | {r['left']} | {r['median_ms']} ({r['min_ms']} .. {r['max_ms']}) | {r['us_per_round']} | "
                     f"{r['bytes_equal_the_reading']} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
