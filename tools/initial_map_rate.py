#!/usr/bin/env python3
"""Device time of Tracking::CreateInitialMapMonocular (orbfe_create_initial_map_batch_device: build, 20 robust iterations of the
global bundle adjustment, finish) for two maps, each as a batch of 1 and tiled to a batch of 256, in one JSON line:

  typical   the `typical` case of tests/np_ba.py: 340 / 380 keypoints, about 260 map points
  cap       a frame pair at the keypoint cap: 4 048 / 4 096 keypoints, about 3 600 map points

Device-resident data, HIP events around the three launches on one stream, warm-ups, the median of the repetitions with its spread
(minimum and maximum).  Problem 0 of the typical batches is compared with the numpy reading (tests/np_ba.py, the parity criterion of
tests/test_ba_gpu.py) before anything is timed; at the cap the reading takes too long to sit in a timing tool, and every problem of a
batch is compared with problem 0 instead.  There is no device predecessor to compare with; the reference runs this on the host.
profiles/initial_map.md.

usage: python tools/initial_map_rate.py [--reps 11] [--warmup 2] [--batch 256]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib, initializer, optimizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    import torch
    from tests import np_ba as B

    maps = {"typical": B.map_scene("typical"), "cap": B._two_view(4096, N=4000, n_extra=48)}
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}
    for name, s in maps.items():
        ref = B.map_reference("typical") if name == "typical" else None
        n1, n2 = len(s["keys1"]), len(s["keys2"])
        cap = max(n1, n2)
        W = (cap + 63) // 64
        c = s["cam"]
        cam = up(optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], 0.0, s["inv_level_sigma2"]).view(np.uint8))
        pad = lambda a, n, fill=0: np.concatenate([a, np.full((n - len(a),) + a.shape[1:], fill, a.dtype)])
        tri = np.zeros(W * 64, np.uint8)
        tri[:n1] = s["triangulated"]
        words = np.packbits(tri.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.int64)
        init = np.zeros(1, _lib.INIT_RESULT_DTYPE)
        init["R21"][0], init["t21"][0] = s["R21"].reshape(9), s["t21"].reshape(3)
        one = [pad(s["keys1"], cap), np.array([n1], np.int32), pad(s["keys2"], cap), np.array([n2], np.int32), pad(s["matches12"].astype(np.int32), cap, -1),
               pad(s["P3D"], cap), words, init.view(np.uint8).reshape(1, 224), pad(s["octaves1"], cap), pad(s["octaves2"], cap)]
        for P in (1, args.batch):
            d = [up(np.concatenate([a] * P) if a.ndim == 1 and len(a) == 1 or a.shape == (1, 224) else np.stack([a] * P)) for a in one]
            poses = torch.zeros((P, 2, 12), dtype=torch.float32, device=dev)
            points = torch.zeros((P, cap, 3), dtype=torch.float32, device=dev)
            index = torch.zeros((P, cap), dtype=torch.int32, device=dev)
            poses_ba = torch.zeros((P, 2, 12), dtype=torch.float32, device=dev)
            points_ba = torch.zeros((P, cap, 3), dtype=torch.float32, device=dev)
            result = torch.zeros((P, 72), dtype=torch.uint8, device=dev)
            ws_bytes = initializer.initial_map_workspace_bytes(P, cap)
            ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=dev)

            def launch():
                initializer.create_initial_map_batch(cam, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], poses, points, index, result,
                                                     ws, poses_ba=poses_ba, points_ba=points_ba, stream=st)
            with torch.cuda.stream(st):
                launch()
            torch.cuda.synchronize()
            res = result.cpu().numpy().view(_lib.INITIAL_MAP_RESULT_DTYPE).reshape(P)
            n = int(res["n_points"][0])
            ratio = None
            if ref is not None:
                idx = index[0, :n].cpu().numpy()
                ratio = B.worst_ratio(poses_ba[0].cpu().numpy(), points_ba[0].cpu().numpy()[idx], ref["unscaled_poses"], ref["unscaled_points"])
                assert ratio <= 1.0 and np.array_equal(idx, ref["index"]) and int(res["reason"][0]) == ref["reason"], (name, P, ratio)
            assert all(res[p].tobytes() == res[0].tobytes() for p in range(P))
            assert all(x.cpu().numpy().reshape(P, -1).tobytes() == np.tile(x[0].cpu().numpy().reshape(1, -1), (P, 1)).tobytes() for x in (poses, points))
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
            ba = res["ba"][0]
            out[f"{name}_x{P}"] = dict(keypoints=[n1, n2], points=n, problems=P, iterations=int(ba["iterations"]), trials=int(ba["trials"]),
                                       chi2=[round(float(ba["chi2_first"]), 1), round(float(ba["chi2_final"]), 1)],
                                       median_depth=round(float(res["median_depth"][0]), 4), workspace_mb=round(ws_bytes / 2 ** 20, 2),
                                       parity_max_over_tolerance=None if ratio is None else round(ratio, 4),
                                       median_ms=round(float(np.median(times)), 3), min_ms=round(float(times.min()), 3),
                                       max_ms=round(float(times.max()), 3), ms_per_problem=round(float(np.median(times)) / P, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
