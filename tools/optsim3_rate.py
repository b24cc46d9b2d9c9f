#!/usr/bin/env python3
"""Wall time of Optimizer::OptimizeSim3 for the candidates of one LoopClosing::ComputeSim3 call: P = 5 candidate keyframes with n = 150
correspondences each (the scenes of tests/np_optsim3.py at that size, free scale, 20 % outliers), three ways in one process,
alternating, warm, medians (and minima) over the repetitions, in one JSON line:

  chain_ms    P calls of orbfe_optimize_sim3, one per candidate, each with its packed upload, launch, packed download and
              synchronisation; host clock around the P calls
  batch_ms    all candidates in ONE orbfe_optimize_sim3_batch_device: pinned inputs copied up, the launch, results and flags copied
              back, all on one stream between two HIP events
  kernel_ms   the kernel alone: the same batch call on device-resident data, HIP events

The ctypes arguments are built once, outside the timed region.  The batch's bytes are checked against the P host calls before anything
is timed.  There is no device predecessor to compare with; the reference runs this on the host.  profiles/optimize_sim3.md.

usage: python tools/optsim3_rate.py [--candidates 5] [--pairs 150] [--reps 40] [--warmup 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=150)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from tests import np_optsim3 as Q

    P, n = args.candidates, args.pairs
    scenes = [Q.make_scene(90 + k, n_pairs=n, outliers=0.2, fix_scale=False, true_scale=1.0 + 0.03 * k) for k in range(P)]
    view = lambda v: optimizer.sim3_view(v["Rcw"], v["tcw"], v["fx"], v["fy"], v["cx"], v["cy"])
    v1, v2 = np.concatenate([view(s["view1"]) for s in scenes]), np.concatenate([view(s["view2"]) for s in scenes])
    pairs = np.stack([s["pairs"] for s in scenes])
    sRt = np.stack([s["sRt_in"] for s in scenes])
    th2 = np.array([s["th2"] for s in scenes], np.float32)
    L, p = _lib.lib(), _lib.ptr

    # ---- the host form, arguments built once
    res, bad = np.zeros(P, _lib.OPTSIM3_RESULT_DTYPE), np.zeros((P, n), np.uint8)
    host_args = [(p(v1[k:k + 1]), p(v2[k:k + 1]), p(pairs[k]), n, p(sRt[k]), C.c_float(float(th2[k])), 0, p(res[k:k + 1]), p(bad[k]))
                 for k in range(P)]

    def chain():
        for a in host_args:
            _lib.check(L.orbfe_optimize_sim3(*a), "orbfe_optimize_sim3")

    # ---- the device form
    dev = torch.device("cuda", 0)
    raw = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    h_in = [raw(v1), raw(v2), raw(pairs), raw(np.full(P, n, np.int32)), raw(sRt), raw(th2), raw(np.zeros(P, np.int32))]
    h_in = [t.pin_memory() for t in h_in]
    d_in = [torch.empty(t.shape, dtype=torch.uint8, device=dev) for t in h_in]
    d_out = [torch.zeros(P * _lib.OPTSIM3_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev), torch.zeros(P * n, dtype=torch.uint8, device=dev)]
    h_out = [torch.empty(t.shape, dtype=torch.uint8).pin_memory() for t in d_out]
    st = torch.cuda.Stream(dev)

    def launch():
        optimizer.optimize_sim3_batch(d_in[0], d_in[1], d_in[2].view(P, n, 48), d_in[3], d_in[4], d_in[5], d_in[6], d_out[0],
                                      d_out[1].view(P, n), st)

    def batch():
        for h, d in zip(h_in, d_in):
            d.copy_(h, non_blocking=True)
        launch()
        for h, d in zip(h_out, d_out):
            h.copy_(d, non_blocking=True)

    chain()
    with torch.cuda.stream(st):
        batch()
    st.synchronize()
    same = h_out[0].numpy().tobytes() == res.tobytes() and h_out[1].numpy().tobytes() == bad.tobytes()
    if not same:
        raise SystemExit("the batch differs from the per-candidate calls: nothing is timed")

    t_chain, t_batch, t_kernel = [], [], []
    with torch.cuda.stream(st):
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            chain()
            dt = (time.perf_counter() - t0) * 1e3
            times = [dt]
            for fn in (batch, launch):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            if k >= args.warmup:
                for acc, t in zip((t_chain, t_batch, t_kernel), times):
                    acc.append(t)
    st.synchronize()
    med = lambda t: round(float(np.median(t)), 4)
    mn = lambda t: round(float(np.min(t)), 4)
    print(json.dumps({"candidates": P, "pairs": n, "reps": args.reps, "n_bad": [int(r) for r in res["n_bad"]],
                      "n_inliers": [int(r) for r in res["n_inliers"]], "iterations": [[int(x) for x in r] for r in res["iterations"]],
                      "chain_ms": med(t_chain), "chain_min_ms": mn(t_chain), "batch_ms": med(t_batch), "batch_min_ms": mn(t_batch),
                      "kernel_ms": med(t_kernel), "kernel_min_ms": mn(t_kernel), "batch_equals_chain_bytes": bool(same)}))


if __name__ == "__main__":
    main()
