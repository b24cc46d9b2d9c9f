#!/usr/bin/env python3
"""Device time of the map-point refresh (orbfe_refresh_map_points_batch_device: MapPoint::ComputeDistinctiveDescriptors and
MapPoint::UpdateNormalAndDepth) for one keyframe's worth of points, beside the single-thread host time of the same reading on the same
data, in one JSON line:

  keyframe        about 2 000 points; observations per point drawn from the histogram
                  2-3: 40 %, 4-7: 30 %, 8-15: 18 %, 16-31: 9 %, 32-64: 3 %   (every point is the wave kernel's)
  keyframe_tail   the same points plus 100 long-lived ones with 200 .. 1 024 observations, evenly spaced (the workgroup kernel's)
  tail            the 100 long-lived points alone
  keyframe_nd     `keyframe` with ORBFE_MP_NORMAL_DEPTH alone: what follows a local bundle adjustment

Device-resident data, HIP events around the two launches on one stream, warm-ups, the median of the repetitions with its spread.  The
device records are compared byte for byte with the host build of csrc/mappoint_internal.h (tests/cpp_mappoint/host_arith.cpp, which
tests/test_mappoint_cpu.py ties to the literal reading) before anything is timed; the host time is that library's, one thread, the
median of three runs.  profiles/map_point_refresh.md.

usage: python tools/bench_map_points.py [--reps 21] [--warmup 3] [--points 2000] [--tail 100]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refactored_orb_slam2_amd import _lib, map_point  # noqa: E402

BINS = ((2, 3, 0.40), (4, 7, 0.30), (8, 15, 0.18), (16, 31, 0.09), (32, 64, 0.03))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--tail", type=int, default=100)
    args = ap.parse_args()
    import torch
    from tests import np_mappoint as M

    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_mappoint")], check=True, capture_output=True)
    H = C.CDLL(os.path.join(ROOT, "tests", "cpp_mappoint", "_build", "libmappoint_host.so"))
    H.mappoint_host_refresh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p]
    H.mappoint_host_refresh.restype = None

    rng = np.random.default_rng(2024)
    which = rng.choice(len(BINS), args.points, p=[b[2] for b in BINS])
    sizes = [int(rng.integers(BINS[b][0], BINS[b][1] + 1)) for b in which]
    sizes += [int(x) for x in np.linspace(200, 1024, args.tail).round()]
    scene = M.make_scene(7, sizes)
    table, obs, recs, positions, keep = map_point.pack_map_points(scene["keyframes"], scene["points"])
    sf = np.ascontiguousarray(scene["scale_factors"], np.float32)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).to(dev)
    blocks = [np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1) for kf in scene["keyframes"]]
    offs = np.cumsum([0] + [b.size for b in blocks])
    d_desc = torch.from_numpy(np.concatenate(blocks)).to(dev)
    d_table_np = table.copy()
    d_table_np["desc"] = d_desc.data_ptr() + offs[:-1]
    d_table, d_obs = up(d_table_np), up(obs)

    both = _lib.MP_DESCRIPTOR | _lib.MP_NORMAL_DEPTH
    n = args.points
    workloads = {"keyframe": (slice(0, n), both), "keyframe_tail": (slice(0, len(recs)), both), "tail": (slice(n, len(recs)), both),
                 "keyframe_nd": (slice(0, n), _lib.MP_NORMAL_DEPTH)}
    out = {}
    for name, (sl, flags) in workloads.items():
        r, p = np.ascontiguousarray(recs[sl]), np.ascontiguousarray(positions[sl])
        P = len(r)
        if P == 0:
            continue
        d_recs, d_pos = up(r), up(p)
        d_out = torch.zeros((P, 64), dtype=torch.uint8, device=dev)

        def launch():
            map_point.refresh_map_points_device(d_table, d_obs, d_recs, d_pos, 12, sf, flags, d_out, stream=st)
        with torch.cuda.stream(st):
            launch()
        torch.cuda.synchronize()
        host = np.zeros(P, _lib.MP_UPDATE_DTYPE)
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            H.mappoint_host_refresh(_lib.ptr(table), len(table), _lib.ptr(obs), len(obs), _lib.ptr(r), _lib.ptr(p), P, _lib.ptr(sf), len(sf), flags,
                                    _lib.ptr(host))
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert d_out.cpu().numpy().tobytes() == host.tobytes(), name
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
        n_obs = r["n_obs"]
        out[name] = dict(points=P, observations=int(n_obs.sum()), max_obs=int(n_obs.max()), wave_points=int((n_obs <= _lib.MP_SMALL_OBS).sum()),
                         workgroup_points=int((n_obs > _lib.MP_SMALL_OBS).sum()), flags=flags, median_ms=round(float(np.median(times)), 4),
                         min_ms=round(float(times.min()), 4), max_ms=round(float(times.max()), 4), host_one_thread_ms=round(float(np.median(host_ms)), 3))
    del keep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
