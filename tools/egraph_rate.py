#!/usr/bin/env python3
"""Device time of Optimizer::OptimizeEssentialGraph for one graph, on both paths (Sim3, and SE3 with a fixed scale) and in both forms
-- one workgroup (orbfe_essential_graph_batch_device, the lone problem of a launch) and across the device
(orbfe_essential_graph_grid_device) --, in one JSON line:

  wide    the `wide` / `wide_se3` cases of tests/np_egraph.py: 300 keyframes, band 8, three loop rows
  kitti   a KITTI-loop-sized graph: 2 000 keyframes, band 20, 30 loop rows
  band_N  (--bands N,N,...) N keyframes, band 20, no loop row: the graphs the crossover between the two forms is read from

Device-resident data, HIP events around the one call on one stream, warm-ups, the median of the repetitions with its spread (minimum
and maximum), the workspace bytes.  `wide` is compared with the numpy reading (tests/np_egraph.py, the parity criterion of
tests/test_egraph_gpu.py) before anything is timed; the dense matrix of the reading does not bear the larger graphs, which are checked
for their status and a falling chi2 only.  Where both forms run, their outputs are compared byte for byte before anything is timed.
The grid form is synchronous -- the host reads one control record per trial --, so its events enclose the host's part as well; one
more call with orbfe_debug_egrid_phases switched on gives the sums of stream-event times per phase and the level count.
profiles/essential_graph.md.

usage: python tools/egraph_rate.py [--reps 11] [--warmup 2] [--skip-kitti] [--forms one,grid] [--bands 40,100,300,1000,2000]
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
    ap.add_argument("--skip-wide", action="store_true")
    ap.add_argument("--forms", default="one,grid")
    ap.add_argument("--bands", default="")
    args = ap.parse_args()
    forms = [f for f in args.forms.split(",") if f]
    assert forms and set(forms) <= {"one", "grid"}, forms
    import torch
    from tests import np_egraph as G

    graphs = {}
    if not args.skip_wide:
        graphs.update({"wide": (G.case_scene("wide"), True), "wide_se3": (G.case_scene("wide_se3"), True)})
    if not args.skip_kitti:
        rows = tuple(range(400, 2000, 54))[:30]
        kw = dict(n_kf=2000, band=20, n_corrected=10, loop_rows=rows, drift_rot=0.05, drift_trans=0.5)
        graphs["kitti"] = (G.make_scene(2000, drift_scale=1.05, **kw), False)
        graphs["kitti_se3"] = (G.make_scene(2000, fix_scale=True, **kw), False)
    for n in [int(v) for v in args.bands.split(",") if v]:
        kw = dict(n_kf=n, band=20, n_corrected=min(10, n // 4), drift_rot=0.05, drift_trans=0.5)
        graphs[f"band_{n}"] = (G.make_scene(n, drift_scale=1.05, **kw), False)
        graphs[f"band_{n}_se3"] = (G.make_scene(n, fix_scale=True, **kw), False)
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
        ref = G.run_case(s) if check else None
        first = None
        for form in forms:
            if form == "one" and env > _lib.EG_MAX_ENVELOPE_BLOCKS:
                continue
            sim3_out = torch.zeros((nk, 8), dtype=torch.float64, device=dev)
            poses_out = torch.zeros((nk, 12), dtype=torch.float32, device=dev)
            result = torch.zeros((1, 48), dtype=torch.uint8, device=dev)
            ws_bytes = (optimizer.essential_graph_workspace_bytes(1, nk, ne, env) if form == "one" else
                        optimizer.essential_graph_grid_workspace_bytes(nk, ne, env))
            ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=dev)

            def launch():
                if form == "one":
                    optimizer.essential_graph_batch(d[0], d[1], d[2], nk, ne, env, sim3_out, poses_out, result, ws, fix_scale=fs, stream=st)
                else:
                    optimizer.essential_graph_grid_device(d[1], d[2], sim3_out, poses_out, result[0], ws, fix_scale=fs, stream=st)
            with torch.cuda.stream(st):
                launch()
            torch.cuda.synchronize()
            res = result.cpu().numpy().view(_lib.EG_RESULT_DTYPE).reshape(1)[0]
            assert int(res["status"]) == _lib.EG_DONE and float(res["chi2_last"]) < float(res["chi2_first"]), (name, form, res)
            got = (sim3_out.cpu().numpy().tobytes(), poses_out.cpu().numpy().tobytes(), res.tobytes())
            if first is None:
                first = got
            assert got == first, f"{name}: the two forms differ"
            units = None
            if ref is not None:
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
            row = dict(keyframes=nk, free=int(res["n_free"]), edges=ne, envelope_blocks=env, iterations=int(res["iterations"]),
                       trials=int(res["trials"]), chi2_first=float(res["chi2_first"]), chi2_last=float(res["chi2_last"]),
                       workspace_mb=round(ws_bytes / 2 ** 20, 2), parity_units=None if units is None else round(units, 4),
                       bound_units=G.BOUND_UNITS[fs], median_ms=round(float(np.median(times)), 3), min_ms=round(float(times.min()), 3),
                       max_ms=round(float(times.max()), 3), ms_per_trial=round(float(np.median(times)) / max(1, int(res["trials"])), 3))
            if form == "grid":                                             # one more call, timed per phase
                ms = np.zeros(len(_lib.EGRID_PHASES), np.float32)
                _lib.check(_lib.lib().orbfe_debug_egrid_phases(1, None), "orbfe_debug_egrid_phases")
                with torch.cuda.stream(st):
                    launch()
                torch.cuda.synchronize()
                _lib.check(_lib.lib().orbfe_debug_egrid_phases(0, _lib.ptr(ms)), "orbfe_debug_egrid_phases")
                row["levels"] = int(ms[-1])
                row["phase_ms"] = {k: round(float(v), 3) for k, v in zip(_lib.EGRID_PHASES[:-1], ms[:-1])}
            out[f"{name}/{form}"] = row
            print(f"{name}/{form}: {row['median_ms']} ms, {row['trials']} trials", file=sys.stderr, flush=True)
            del ws
    print(json.dumps(out))


if __name__ == "__main__":
    main()
