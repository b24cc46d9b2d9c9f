#!/usr/bin/env python3
"""Call times of the keyframe database: N entries of about W words each over n_words word ids (places with word pools, as the scenes of
tests/np_kfdb.py), Q relocalisation queries per call, in one process, alternating, warm, medians over the repetitions, one JSON line:

  host_ms       orbfe_kfdb_detect_relocalization: packed upload, the passes, packed download, synchronisation; host clock
  device_ms     orbfe_kfdb_detect_relocalization_device on device-resident queries, HIP events around the call
  fused_ms      the same device call under orbfe_debug_kfdb_arrangement(1): the common pass scores every pair (the arrangement that
                was measured and not kept)
  common_bound_ms   the entries' ids read once per batch at 8 TB/s; the common pass's share of it needs the kernel trace
                (rocprofv3 --kernel-trace --stats -- python tools/kfdb_rate.py ... in a run of its own)

The device form's outputs are compared with the host form's before anything is timed, under both arrangements.  The carried
relocalisation scores move with every call; a database twin keeps the compared calls on equal state.  profiles/keyframe_database.md.

usage: python tools/kfdb_rate.py [--entries 1000] [--words 1000] [--n-words 1000000] [--queries 1] [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib  # noqa: E402
from refactored_orb_slam2_amd.keyframe_database import KeyFrameDatabase, pack_queries  # noqa: E402


def draw(rng, pool, w):
    ids = np.unique(pool[rng.integers(0, len(pool), int(w * 1.25))])[:w].astype(np.int32)
    vals = rng.random(len(ids)) + 0.05
    return ids, vals / vals.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--n-words", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    N, W, Q = args.entries, args.words, args.queries
    rng = np.random.default_rng(5)
    n_places = max(N // 25, 1)
    pools = [rng.choice(args.n_words, size=3 * W, replace=False) for _ in range(n_places)]
    entries = [draw(rng, pools[k * n_places // N], W) for k in range(N)]
    queries = [draw(rng, pools[int(rng.integers(n_places))], W) for _ in range(Q)]
    rows = [[int(j) for j in rng.permutation(np.arange(max(0, k - 8), min(N, k + 9)))[:10] if j != k] for k in range(N)]

    def database():
        db = KeyFrameDatabase(args.n_words)
        for k, (ids, vals) in enumerate(entries):
            db.add(k, ids, vals)
        db.set_covisibles(np.arange(N), rows)
        return db

    L, p = _lib.lib(), _lib.ptr
    db, twin = database(), database()
    cap = 32
    off, ids, vals = pack_queries(queries)
    cand, n_cand, info = np.zeros((Q, cap), np.int64), np.zeros(Q, np.int32), np.zeros(Q, _lib.KFDB_INFO_DTYPE)
    host_args = (db._h, Q, p(off), p(ids), p(vals), cap, p(cand), p(n_cand), p(info), None, None)

    dev = torch.device("cuda", 0)
    d_in = [torch.from_numpy(a).to(dev) for a in (off, ids, vals)]
    d_cand = torch.zeros((Q, cap), dtype=torch.int64, device=dev)
    d_n = torch.zeros(Q, dtype=torch.int32, device=dev)
    d_info = torch.zeros((Q, 32), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)

    def host():
        _lib.check(L.orbfe_kfdb_detect_relocalization(*host_args), "orbfe_kfdb_detect_relocalization")

    def device(which=twin):
        which.detect_relocalization_device(Q, d_in[0], d_in[1], d_in[2], cap, d_cand, d_n, d_info, None, None, st)

    def fused():
        _lib.check(L.orbfe_debug_kfdb_arrangement(1), "orbfe_debug_kfdb_arrangement")
        try:
            device()
        finally:
            _lib.check(L.orbfe_debug_kfdb_arrangement(0), "orbfe_debug_kfdb_arrangement")

    def device_bytes():
        st.synchronize()
        return d_n.cpu().numpy().tobytes() + d_info.cpu().numpy().tobytes() + d_cand.cpu().numpy().tobytes()

    host()
    want = n_cand.tobytes() + info.tobytes()
    device()
    got = device_bytes()
    third = database()
    _lib.check(L.orbfe_debug_kfdb_arrangement(1), "orbfe_debug_kfdb_arrangement")
    device(third)
    got_fused = device_bytes()
    _lib.check(L.orbfe_debug_kfdb_arrangement(0), "orbfe_debug_kfdb_arrangement")
    k = len(want)
    rows_equal = all(np.array_equal(cand[q, : min(n_cand[q], cap)], np.frombuffer(got[k:], np.int64).reshape(Q, cap)[q, : min(n_cand[q], cap)])
                     for q in range(Q))
    if got[:k] != want or got_fused != got or not rows_equal:
        raise SystemExit("the device form differs from the host form: nothing is timed")
    third.close()

    t_host, t_dev, t_fused = [], [], []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        host()
        times = [(time.perf_counter() - t0) * 1e3]
        for fn in (device, fused):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        if r >= args.warmup:
            for acc, t in zip((t_host, t_dev, t_fused), times):
                acc.append(t)
    med = lambda t: round(float(np.median(t)), 4)
    mn = lambda t: round(float(np.min(t)), 4)
    id_bytes = sum(len(e[0]) for e in entries) * 4
    print(json.dumps({"entries": N, "words": W, "n_words": args.n_words, "queries": Q, "reps": args.reps,
                      "n_scored": [int(x) for x in info["n_scored"][:8]], "n_cand": [int(x) for x in n_cand[:8]],
                      "host_ms": med(t_host), "host_min_ms": mn(t_host), "device_ms": med(t_dev), "device_min_ms": mn(t_dev),
                      "fused_ms": med(t_fused), "fused_min_ms": mn(t_fused), "entry_id_bytes": id_bytes,
                      "common_bound_ms": round(id_bytes / 8.0e12 * 1e3, 5), "device_equals_host_bytes": True}))


if __name__ == "__main__":
    main()
