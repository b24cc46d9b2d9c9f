#!/usr/bin/env python3
"""Wall time of the Sim3 RANSAC of one LoopClosing::ComputeSim3 call: P = 5 candidate keyframes, H = 300 hypotheses each over n = 150
correspondences (the scenes of tests/np_sim3.py at that size, free scale, 30 % outliers), three ways in one process, alternating, warm,
medians over the repetitions, in one JSON line:

  chain_ms    P calls of orbfe_sim3_solve, one per candidate, each with its packed upload, launch pair, packed download and
              synchronisation; host clock around the P calls
  batch_ms    all candidates in ONE orbfe_sim3_solve_batch_device: pinned inputs copied up, the launch pair, results, hypothesis
              records and inlier words copied back, all on one stream between two HIP events
  kernel_ms   the two kernels alone: the same batch call on device-resident data, HIP events

The ctypes arguments are built once, outside the timed region.  The batch's bytes are checked against the P host calls before anything
is timed.  There is no device predecessor to compare with; the reference runs this on the host.  profiles/sim3_solver.md.

usage: python tools/sim3_rate.py [--candidates 5] [--hypotheses 300] [--pairs 150] [--reps 40] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib, sim3  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=5)
    ap.add_argument("--hypotheses", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=150)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from tests import np_sim3 as S

    P, H, n = args.candidates, args.hypotheses, args.pairs
    W = (n + 63) // 64
    scenes = [S.make_scene(90 + k, n=n, H=H, fix_scale=False, true_scale=1.0 + 0.05 * k) for k in range(P)]
    L, p = _lib.lib(), _lib.ptr

    # ---- the host form, arguments built once
    hyps = np.zeros((P, H), _lib.SIM3_HYPOTHESIS_DTYPE)
    words = np.zeros((P, H, W), np.uint64)
    res, mask = np.zeros(P, _lib.SIM3_RESULT_DTYPE), np.zeros((P, W), np.uint64)
    host_args = [(p(s["view1"]), p(s["view2"]), p(s["pairs"]), n, p(s["triples"]), H, 0, s["min_inliers"], p(hyps[k]), p(words[k]),
                  p(res[k:k + 1]), p(mask[k])) for k, s in enumerate(scenes)]

    def chain():
        for a in host_args:
            _lib.check(L.orbfe_sim3_solve(*a), "orbfe_sim3_solve")

    # ---- the device form
    dev = torch.device("cuda", 0)
    raw = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    h_in = [raw(np.concatenate([s["view1"] for s in scenes])), raw(np.concatenate([s["view2"] for s in scenes])),
            raw(np.stack([s["pairs"] for s in scenes])), raw(np.full(P, n, np.int32)), raw(np.stack([s["triples"] for s in scenes])),
            raw(np.full(P, H, np.int32)), raw(np.zeros(P, np.int32)), raw(np.array([s["min_inliers"] for s in scenes], np.int32))]
    h_in = [t.pin_memory() for t in h_in]
    d_in = [torch.empty(t.shape, dtype=torch.uint8, device=dev) for t in h_in]
    d_out = [torch.zeros(P * H * 64, dtype=torch.uint8, device=dev), torch.zeros(P * H * W * 8, dtype=torch.uint8, device=dev),
             torch.zeros(P * 128, dtype=torch.uint8, device=dev), torch.zeros(P * W * 8, dtype=torch.uint8, device=dev)]
    h_out = [torch.empty(t.shape, dtype=torch.uint8).pin_memory() for t in d_out]
    st = torch.cuda.Stream(dev)

    def launch():
        sim3.sim3_solve_batch(d_in[0], d_in[1], d_in[2].view(P, n, 32), d_in[3], d_in[4].view(P, H, 12), d_in[5], d_in[6], d_in[7], d_out[0],
                              d_out[1], d_out[2], d_out[3], st)

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
    same = (h_out[0].numpy().tobytes() == hyps.tobytes() and h_out[1].numpy().tobytes() == words.tobytes() and
            h_out[2].numpy().tobytes() == res.tobytes() and h_out[3].numpy().tobytes() == mask.tobytes())
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
    print(json.dumps({"candidates": P, "hypotheses": H, "pairs": n, "reps": args.reps, "returned": [int(r) for r in res["returned"]],
                      "best_inliers": [int(r) for r in res["best_inliers"]], "chain_ms": med(t_chain), "chain_min_ms": mn(t_chain),
                      "batch_ms": med(t_batch), "batch_min_ms": mn(t_batch), "kernel_ms": med(t_kernel), "kernel_min_ms": mn(t_kernel),
                      "batch_equals_chain_bytes": bool(same)}))


if __name__ == "__main__":
    main()
