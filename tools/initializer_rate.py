#!/usr/bin/env python3
"""Wall time of Initializer::Initialize at the size the monocular examples reach: N = 1 500 matches, H = 200 hypotheses per model
(the general scene of tests/np_initializer.py at that size), medians over the repetitions after a warm-up, in one JSON line:

  host_ms     one orbfe_initializer_initialize: packed upload, five launches, packed download, one synchronisation; host clock
  batch_ms    P = 8 problems in ONE orbfe_initializer_initialize_batch_device: pinned inputs copied up, the launches, result records,
              points and words copied back, on one stream between two HIP events
  kernel_ms   the five kernels alone: the same batch call on device-resident data, HIP events
  cpu_ms      the single-thread host build of the same header (tests/cpp_initializer) on one problem; the reference runs its two
              models on two threads, so its Find* half would take about half of a single thread's

There is no device predecessor to compare with, so no ratio is claimed.  profiles/initializer.md.

usage: python tools/initializer_rate.py [--problems 8] [--hypotheses 200] [--matches 1500] [--reps 40] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib, initializer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=8)
    ap.add_argument("--hypotheses", type=int, default=200)
    ap.add_argument("--matches", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from tests import initializer_host as IH
    from tests import np_initializer as Y

    P, H, N = args.problems, args.hypotheses, args.matches
    scenes = []
    for k in range(P):
        k1, k2, m12, params, _ = Y.scene(seed=200 + k, kind="general", N=N, n_extra=100)
        scenes.append((k1, k2, m12, Y.draw_sets(N, H, 300 + k), IH.params_of(params)))
    cap = max(max(len(s[0]), len(s[1])) for s in scenes)
    W = (cap + 63) // 64

    def host():
        return initializer.initialize(scenes[0][4], scenes[0][0], scenes[0][1], scenes[0][2], scenes[0][3], want_candidates=False)

    def cpu():
        return IH.host_run(scenes[0][0], scenes[0][1], scenes[0][2], scenes[0][3], scenes[0][4])

    dev = torch.device("cuda", 0)
    keys1, keys2 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    m12, sets = np.full((P, cap), -1, np.int32), np.zeros((P, H, 8), np.int32)
    n1, n2, par = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, _lib.INIT_PARAMS_DTYPE)
    for k, s in enumerate(scenes):
        keys1[k, :len(s[0])], keys2[k, :len(s[1])], m12[k, :len(s[2])], sets[k], par[k] = s[0], s[1], s[2], s[3], s[4][0]
        n1[k], n2[k] = len(s[0]), len(s[1])
    h_in = [torch.from_numpy(par.view(np.uint8).reshape(P, 32)), torch.from_numpy(keys1), torch.from_numpy(n1), torch.from_numpy(keys2),
            torch.from_numpy(n2), torch.from_numpy(m12), torch.from_numpy(sets), torch.from_numpy(np.full(P, H, np.int32))]
    h_in = [t.pin_memory() for t in h_in]
    d_in = [torch.empty_like(t, device=dev) for t in h_in]
    d_out = {"result": torch.zeros((P, 224), dtype=torch.uint8, device=dev), "P3D": torch.zeros((P, cap, 3), dtype=torch.float32, device=dev),
             "tri": torch.zeros((P, W), dtype=torch.int64, device=dev), "inl": torch.zeros((P, W), dtype=torch.int64, device=dev)}
    d_work = {"hyps": torch.zeros((P, 2, H, 64), dtype=torch.uint8, device=dev), "words": torch.zeros((P, 2, H, W), dtype=torch.int64, device=dev),
              "cands": torch.zeros((P, 8, 64), dtype=torch.uint8, device=dev),
              "ws": torch.zeros(initializer.workspace_bytes(P, cap), dtype=torch.uint8, device=dev)}
    h_out = {k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in d_out.items()}
    st = torch.cuda.Stream(dev)

    def launch():
        initializer.initialize_batch(*d_in, d_out["result"], d_out["P3D"], d_out["tri"], d_out["inl"], d_work["hyps"], d_work["words"],
                                     d_work["cands"], d_work["ws"], stream=st)

    def batch():
        for h, d in zip(h_in, d_in):
            d.copy_(h, non_blocking=True)
        launch()
        for k in h_out:
            h_out[k].copy_(d_out[k], non_blocking=True)

    one = host()
    with torch.cuda.stream(st):
        batch()
    st.synchronize()
    if h_out["result"].numpy()[0].tobytes() != one["result"].tobytes():
        raise SystemExit("the batch differs from the host call: nothing is timed")

    t_host, t_batch, t_kernel, t_cpu = [], [], [], []
    with torch.cuda.stream(st):
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            host()
            times = [(time.perf_counter() - t0) * 1e3]
            for fn in (batch, launch):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            if k >= args.warmup:
                for acc, t in zip((t_host, t_batch, t_kernel), times):
                    acc.append(t)
    st.synchronize()
    for k in range(2 + max(args.reps // 8, 3)):
        t0 = time.perf_counter()
        cpu()
        if k >= 2:
            t_cpu.append((time.perf_counter() - t0) * 1e3)
    med = lambda t: round(float(np.median(t)), 4)
    res = h_out["result"].numpy().view(_lib.INIT_RESULT_DTYPE).reshape(P)
    print(json.dumps({"problems": P, "hypotheses": H, "matches": N, "reps": args.reps, "success": [int(x) for x in res["success"]],
                      "model": [int(x) for x in res["model"]], "host_ms": med(t_host), "batch_ms": med(t_batch), "kernel_ms": med(t_kernel),
                      "cpu_single_thread_ms": med(t_cpu), "cpu_reps": len(t_cpu), "batch_equals_host_bytes": True}))


if __name__ == "__main__":
    main()
