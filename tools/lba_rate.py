#!/usr/bin/env python3
"""Device time of Optimizer::LocalBundleAdjustment (orbfe_local_bundle_adjustment_batch_device) for two windows, each as a batch of 1
and tiled to a batch of 256, in one JSON line:

  standard   the `standard` case of tests/np_lba.py: 6 free + 3 fixed keyframes, 300 points
  kitti      a KITTI-sized window: 20 free + 10 fixed keyframes, 2 000 points

Device-resident data, HIP events around the launch on one stream, warm-ups, the median of the repetitions with its spread (minimum
and maximum).  Problem 0 of every batch is compared with the numpy reading (tests/np_lba.py, the parity criterion of
tests/test_lba_gpu.py) before anything is timed.  There is no device predecessor to compare with; the reference runs this on the host.
profiles/local_bundle_adjustment.md.

usage: python tools/lba_rate.py [--reps 11] [--warmup 2] [--batch 256]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib, optimizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    import torch
    from tests import np_lba as Q

    windows = {"standard": Q.case_scene("standard"), "kitti": Q.make_scene(2020, n_free=20, n_fixed=10, n_points=2000)}
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}
    for name, s in windows.items():
        ref = Q.run_scene(s)
        nk, npt, ne = len(s["poses"]), len(s["points"]), len(s["edges"])
        c = s["cam"]
        cam = up(optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], [1.0]).view(np.uint8))
        for P in (1, args.batch):
            prob = np.zeros(P, _lib.LBA_PROBLEM_DTYPE)
            for i in range(P):
                prob[i] = (i * nk, nk, i * npt, npt, i * ne, ne)
            d = [up(prob.view(np.uint8).reshape(P, 24)), up(np.tile(s["poses"], (P, 1))), up(np.tile(s["fixed"], P)),
                 up(np.tile(s["points"], (P, 1))), up(np.tile(s["edges"], P).view(np.uint8).reshape(-1, 24))]
            poses_out = torch.zeros((P * nk, 12), dtype=torch.float32, device=dev)
            points_out = torch.zeros((P * npt, 3), dtype=torch.float32, device=dev)
            erase = torch.zeros((P * ne,), dtype=torch.uint8, device=dev)
            result = torch.zeros((P, 72), dtype=torch.uint8, device=dev)
            ws_bytes = optimizer.lba_workspace_bytes(P, nk, npt, ne)
            ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=dev)

            def launch():
                optimizer.local_bundle_adjustment_batch(cam, d[0], d[1], d[2], d[3], d[4], nk, npt, ne, poses_out, points_out, erase, result, ws,
                                                        stream=st)
            with torch.cuda.stream(st):
                launch()
            torch.cuda.synchronize()
            res = result.cpu().numpy().view(_lib.LBA_RESULT_DTYPE).reshape(P)[0]
            ratio = Q.worst_ratio(poses_out[:nk].cpu().numpy(), points_out[:npt].cpu().numpy(), ref["poses"], ref["points"])
            er = erase[:ne].cpu().numpy()
            assert ratio <= 1.0 and np.array_equal(er & 1, ref["erase"]) and np.array_equal(er >> 1, ref["dropped"]), (name, P, ratio)
            assert (int(res["rounds"]), int(res["n_dropped"]), int(res["n_erase"])) == (ref["rounds"], ref["n_dropped"], ref["n_erase"])
            times = []
            for k in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    launch()
                    e1.record(st)
                e1.synchronize()
                if k >= args.warmup:
                    times.append(e0.elapsed_time(e1))
            times = np.array(times)
            out[f"{name}_x{P}"] = dict(keyframes=nk, free=int(res["n_free"]), points=npt, edges=ne, problems=P,
                                       trials=res["trials"].tolist(), workspace_mb=round(ws_bytes / 2 ** 20, 2),
                                       parity_max_over_tolerance=round(ratio, 4), median_ms=round(float(np.median(times)), 3),
                                       min_ms=round(float(times.min()), 3), max_ms=round(float(times.max()), 3),
                                       ms_per_problem=round(float(np.median(times)) / P, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
