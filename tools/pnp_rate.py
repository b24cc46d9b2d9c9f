#!/usr/bin/env python3
"""Device time of the PnP RANSAC of one Tracking::Relocalization call at the call site's parameters (SetRansacParameters(0.99, 10, 300,
4, 0.5, 5.991): 35 hypotheses over n = 60 correspondences, 30 % outliers, 0.7 px noise -- the scenes of tests/np_pnp.py), for P in
{1, 8, 32} candidate keyframes, two ways in one process, alternating, warm, medians over the repetitions, one JSON line per P:

  chain_ms    P calls of orbfe_pnp_solve, one per candidate, each with its packed upload, three launches, packed download and
              synchronisation; host clock around the P calls (each ends in a synchronise)
  batch_ms    all candidates in ONE orbfe_pnp_solve_batch_device on device-resident data: the three launches between two HIP events
  window_ms   the same batch launched `--window` times back to back between two events, divided by the window: the steady rate, with the
              launch gaps of a single call amortised

The ctypes arguments are built once, outside the timed region.  The batch's bytes are checked against the P host calls before anything
is timed.  There is no device predecessor to compare with, and the reference cannot be built where this library is (it needs the legacy
OpenCV C API); the batch of 32 against 32 single calls says what batching buys, nothing else.  profiles/pnp_solver.md.

usage: python tools/pnp_rate.py [--candidates 1 8 32] [--pairs 60] [--reps 40] [--warmup 5] [--window 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib, pnp  # noqa: E402


def measure(P, n, args, torch, Y):
    mi, H, _ = pnp.ransac_parameters(n, **{k: Y.CALL_SITE[k] for k in ("probability", "min_inliers", "max_iterations", "min_set", "epsilon")})
    W = (n + 63) // 64
    n_out = int(round(0.3 * n))
    scenes = [Y.make_scene(n - n_out, n_out, 0.7, 500 + k) for k in range(P)]
    sets = [pnp.draw_minimal_sets(n, H, np.random.default_rng(900 + k)) for k in range(P)]
    cams = np.zeros(P, _lib.PNP_CAMERA_DTYPE)
    for k, s in enumerate(scenes):
        for f in ("fx", "fy", "cx", "cy"):
            cams[f][k] = s["cam"][f]
    pts = np.stack([s["points"] for s in scenes])
    L, p = _lib.lib(), _lib.ptr

    # ---- the host form, arguments built once
    hyps, refs = np.zeros((P, H), _lib.PNP_HYPOTHESIS_DTYPE), np.zeros((P, H), _lib.PNP_REFINE_DTYPE)
    words, rwords = np.zeros((P, H, W), np.uint64), np.zeros((P, H, W), np.uint64)
    res, mask = np.zeros(P, _lib.PNP_RESULT_DTYPE), np.zeros((P, W), np.uint64)
    host_args = [(p(cams[k:k + 1]), p(pts[k]), n, p(sets[k]), 4, H, mi, p(hyps[k]), p(words[k]), p(refs[k]), p(rwords[k]), None, None,
                  p(res[k:k + 1]), p(mask[k])) for k in range(P)]

    def chain():
        for a in host_args:
            _lib.check(L.orbfe_pnp_solve(*a), "orbfe_pnp_solve")

    # ---- the device form on resident data
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_in = [up(cams), up(pts), up(np.full(P, n, np.int32)), up(np.stack(sets)), up(np.full(P, H, np.int32)), up(np.full(P, mi, np.int32))]
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_out = [zeros(P * H * 112), zeros(P * H * W * 8), zeros(P * H * 112), zeros(P * H * W * 8), zeros(P * 80), zeros(P * W * 8)]
    st = torch.cuda.Stream(dev)

    def launch():
        pnp.pnp_solve_batch(d_in[0], d_in[1].view(P, n, 24), d_in[2], d_in[3].view(torch.int32).view(P, H, 4), d_in[4], d_in[5], d_out[0],
                            d_out[1], d_out[2], d_out[3], d_out[4], d_out[5], stream=st)

    chain()
    launch()
    st.synchronize()
    same = (d_out[0].cpu().numpy().tobytes() == hyps.tobytes() and d_out[1].cpu().numpy().tobytes() == words.tobytes() and
            d_out[2].cpu().numpy().tobytes() == refs.tobytes() and d_out[3].cpu().numpy().tobytes() == rwords.tobytes() and
            d_out[4].cpu().numpy().tobytes() == res.tobytes() and d_out[5].cpu().numpy().tobytes() == mask.tobytes())
    if not same:
        raise SystemExit("the batch differs from the per-candidate calls: nothing is timed")

    t_chain, t_batch, t_window = [], [], []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        chain()
        times = [(time.perf_counter() - t0) * 1e3]
        for count in (1, args.window):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(count):
                launch()
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / count)
        if k >= args.warmup:
            for acc, t in zip((t_chain, t_batch, t_window), times):
                acc.append(t)
    med = lambda t: round(float(np.median(t)), 4)
    mn = lambda t: round(float(np.min(t)), 4)
    n_refines = int((hyps["refine"] >= 0).sum())
    return {"candidates": P, "hypotheses": H, "pairs": n, "min_inliers": mi, "reps": args.reps, "window": args.window, "refines": n_refines,
            "returned": int((res["returned"] >= 0).sum()), "refined": int(res["refined"].sum()),
            "chain_ms": med(t_chain), "chain_min_ms": mn(t_chain), "batch_ms": med(t_batch), "batch_min_ms": mn(t_batch),
            "window_ms": med(t_window), "window_min_ms": mn(t_window), "batch_equals_chain_bytes": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--pairs", type=int, default=60)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    args = ap.parse_args()
    import torch
    from tests import np_pnp as Y
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    for P in args.candidates:
        print(json.dumps(measure(P, args.pairs, args, torch, Y)), flush=True)


if __name__ == "__main__":
    main()
