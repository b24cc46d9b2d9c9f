#!/usr/bin/env python3
"""Device time of Optimizer::OptimizeEssentialGraph (orbfe_essential_graph_batch_device) for two graphs, each as the lone problem of a
launch and on both paths (Sim3, and SE3 with a fixed scale), in one JSON line:

  wide    the `wide` / `wide_se3` cases of tests/np_egraph.py: 300 keyframes, band 8, three loop rows
  kitti   a KITTI-loop-sized graph: 2 000 keyframes, band 20, 30 loop rows

Device-resident data, HIP events around the one launch on one stream, warm-ups, the median of the repetitions with its spread (minimum
and maximum), the workspace bytes.  `wide` is compared with the numpy reading (tests/np_egraph.py, the parity criterion of
tests/test_egraph_gpu.py) before anything is timed; the dense matrix of the reading does not bear `kitti`, which is checked for its
status and a falling chi2 only.  There is no device predecessor to compare with; the reference runs this on the host.
profiles/essential_graph.md.

usage: python tools/egraph_rate.py [--reps 11] [--warmup 2] [--skip-kitti]
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
    ap.add_argument("--skip-kitti", action="store_true")
    args = ap.parse_args()
    import torch
    from tests import np_egraph as G

    graphs = {"wide": (G.case_scene("wide"), True), "wide_se3": (G.case_scene("wide_se3"), True)}
    if not args.skip_kitti:
        rows = tuple(range(400, 2000, 54))[:30]
        kw = dict(n_kf=2000, band=20, n_corrected=10, loop_rows=rows, drift_rot=0.05, drift_trans=0.5)
        graphs["kitti"] = (G.make_scene(2000, drift_scale=1.05, **kw), False)
        graphs["kitti_se3"] = (G.make_scene(2000, fix_scale=True, **kw), False)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}
    for name, (s, check) in graphs.items():
        V, E, fs = s["vertices"], s["edges"], s["fix_scale"]
        nk, ne = len(V), len(E)
        env = optimizer.essential_graph_envelope_blocks(nk, (V["fixed"] != 0).astype(np.uint8), E)
        prob = np.zeros(1, _lib.EG_PROBLEM_DTYPE)
        prob[0] = (0, nk, 0, ne)
        d = [up(prob.view(np.uint8).reshape(1, 16)), up(V.view(np.uint8).reshape(-1, 136)), up(E.view(np.uint8).reshape(-1, 12))]
        sim3_out = torch.zeros((nk, 8), dtype=torch.float64, device=dev)
        poses_out = torch.zeros((nk, 12), dtype=torch.float32, device=dev)
        result = torch.zeros((1, 48), dtype=torch.uint8, device=dev)
        ws_bytes = optimizer.essential_graph_workspace_bytes(1, nk, ne, env)
        ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=dev)

        def launch():
            optimizer.essential_graph_batch(d[0], d[1], d[2], nk, ne, env, sim3_out, poses_out, result, ws, fix_scale=fs, stream=st)
        with torch.cuda.stream(st):
            launch()
        torch.cuda.synchronize()
        res = result.cpu().numpy().view(_lib.EG_RESULT_DTYPE).reshape(1)[0]
        assert int(res["status"]) == _lib.EG_DONE and float(res["chi2_last"]) < float(res["chi2_first"]), (name, res)
        units = None
        if check:
            ref = G.run_case(s)
            units = max(G.sim3_units(sim3_out.cpu().numpy().view(_lib.EG_SIM3_DTYPE).reshape(-1), ref["sim3"]),
                        G.pose_units(poses_out.cpu().numpy(), ref["poses"]))
            assert units <= G.BOUND_UNITS[fs], (name, units)
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
        out[name] = dict(keyframes=nk, free=int(res["n_free"]), edges=ne, envelope_blocks=env, iterations=int(res["iterations"]),
                         trials=int(res["trials"]), chi2_first=float(res["chi2_first"]), chi2_last=float(res["chi2_last"]),
                         workspace_mb=round(ws_bytes / 2 ** 20, 2), parity_units=None if units is None else round(units, 4),
                         bound_units=G.BOUND_UNITS[fs], median_ms=round(float(np.median(times)), 3), min_ms=round(float(times.min()), 3),
                         max_ms=round(float(times.max()), 3), ms_per_trial=round(float(np.median(times)) / max(1, int(res["trials"])), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
