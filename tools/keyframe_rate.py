#!/usr/bin/env python3
"""Times the keyframe decision and the close stereo points (orbfe_keyframe_insertion_batch_device) on one KITTI-shaped batch.

    python tools/keyframe_rate.py [--frames 256] [--keys 2000] [--iters 25] [--out FILE.json]

The batch (its actual numbers are printed): --frames frames of about --keys keypoints, two thirds with a stereo depth between 2 and
120 m, a third of the slots holding points of a local map of 4 096 records per frame, mThDepth 40 m, decision records that make every
frame need a keyframe.  Everything is resident before the clock starts.  Timed with events on one stream, warm, median of --iters (at
least 20):
  (a) the call alone: statistics, decision and creation in one launch
  (b) the same work as a caller without it does it: the download of depth / assigned / outlier (and the observed flags), the
      yardstick's rule vectorised with numpy on the host, and the upload of the new records (wall clock around the whole)
  (c) the share of the sort: the call on the same batch with every depth at 0 (no candidates, so no keys, no sort and no records),
      with the creation switched off (statistics and decision only), and two pairs that differ in the sort alone: a record for every
      candidate without slots, once in initialisation mode (index order, NO sort) and once in keyframe mode with an mThDepth beyond
      every depth (the whole sorted order is the prefix) -- on the batch, and on the same batch with a third of the depths kept, where
      the network is sized by the frame's few candidates and not by cap
(a) is set beside its byte bound -- every input row read once, the records and depth_selected written once -- over the 6.3 TB/s a
streaming kernel reaches on this device.  The records of (a) are compared with the host route's byte for byte.  One JSON line at the
end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refactored_orb_slam2_amd import _lib, tracking  # noqa: E402

HBM_TBS = 6.3


def build_batch(S, n, cap, p_cap, seed=3):
    rng = np.random.default_rng(seed)
    keys = np.zeros((S, cap), _lib.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, 1241, (S, cap)).astype(np.float32), rng.uniform(0, 376, (S, cap)).astype(np.float32)
    keys["octave"] = rng.integers(0, 8, (S, cap))
    desc = rng.integers(0, 256, (S, cap, 32), dtype=np.uint8)
    depth = rng.uniform(2, 120, (S, cap)).astype(np.float32)
    depth[rng.random((S, cap)) < 0.33] = 0
    ns = (n - rng.integers(0, n // 10, S)).astype(np.int32)
    cam = np.zeros(S, _lib.UNPROJECT_CAM_DTYPE)
    cam["Rwc"], cam["Ow"] = np.eye(3, dtype=np.float32).reshape(9), rng.uniform(-50, 50, (S, 3)).astype(np.float32)
    cam["cx"], cam["cy"], cam["invfx"], cam["invfy"] = 607.19, 185.22, np.float32(1) / np.float32(718.856), np.float32(1) / np.float32(718.856)
    points = np.zeros((S, p_cap), _lib.MAP_POINT_DTYPE)
    points["pos"] = rng.uniform(-100, 100, (S, p_cap, 3)).astype(np.float32)
    points["observed"] = rng.random((S, p_cap)) < 0.8
    assigned = np.where(rng.random((S, cap)) < 0.33, rng.integers(0, p_cap, (S, cap)), -1).astype(np.int32)
    outlier = ((rng.random((S, cap)) < 0.1) & (assigned >= 0)).astype(np.uint8)
    decision = tracking.pack_decision([dict(frame_id=100 + f, last_keyframe_id=50, max_frames=30, sensor=1, accept_keyframes=1, n_kfs=10)
                                       for f in range(S)])
    ref_slots = np.arange(2000, dtype=np.int32)
    return dict(keys=keys, desc=desc, depth=depth, n=ns, cam=cam, points=points, n_points=np.full(S, p_cap, np.int32), assigned=assigned,
                outlier=outlier, decision=decision, ref_slots=ref_slots, point_bad=np.zeros(4096, np.uint8),
                point_observations=np.full(4096, 3, np.int32))


def host_route(B, scales, cap):
    """the yardstick's rule for a batch, vectorised: (n_new [S], records [S][cap], index [S][cap]) -- keyframe mode, every frame needed"""
    S = len(B["n"])
    th, sf = scales["th_depth"][0], scales["scale_factors"][0]
    out, idx_out, n_out = np.zeros((S, cap), _lib.MAP_POINT_DTYPE), np.zeros((S, cap), np.int32), np.zeros(S, np.int32)
    for f in range(S):
        n = int(B["n"][f])
        d = B["depth"][f, :n]
        cand = np.flatnonzero(d > 0)
        key = (d[cand].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)
        order = cand[np.argsort(key, kind="stable")]
        c = int(np.count_nonzero(d[cand] <= th))
        sel = order[:min(len(cand), max(100, c) + 1)]
        a = B["assigned"][f, sel]
        create = (a < 0) | (B["points"]["observed"][f, np.maximum(a, 0)] <= 0)
        i = sel[create]
        cam, kp = B["cam"][f], B["keys"][f]
        z = d[i]
        xc = ((kp["x"][i] - cam["cx"]) * z) * cam["invfx"]
        yc = ((kp["y"][i] - cam["cy"]) * z) * cam["invfy"]
        R = cam["Rwc"]
        pos = np.stack([(((R[3 * r] * xc) + (R[3 * r + 1] * yc)) + (R[3 * r + 2] * z)).astype(np.float64) + np.float64(cam["Ow"][r])
                        for r in range(3)], axis=1).astype(np.float32)
        dlt = pos - cam["Ow"][None, :]
        s = np.zeros(len(i), np.float64)
        for k in range(3):
            s = s + dlt[:, k].astype(np.float64) * dlt[:, k].astype(np.float64)
        norm = np.sqrt(s)
        rec = out[f, :len(i)]
        rec["pos"], rec["normal"] = pos, (np.float32(0) + dlt * (1.0 / norm).astype(np.float32)[:, None]) * np.float32(1)
        rec["max_distance"] = norm.astype(np.float32) * sf[kp["octave"][i]]
        rec["min_distance"] = rec["max_distance"] / sf[int(scales["n_levels"][0]) - 1]
        rec["observed"], rec["desc"] = 1, B["desc"][f, i]
        idx_out[f, :len(i)], n_out[f] = i, len(i)
    return n_out, out, idx_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.iters = max(20, a.iters)
    import torch
    S, cap, p_cap = a.frames, a.keys + 48, 4096
    B = build_batch(S, a.keys, cap, p_cap)
    scales = tracking.pack_scales([1.2 ** k for k in range(8)], 40.0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (-1,)) if x.dtype.names else np.ascontiguousarray(x)).cuda()
    slots = dev(B["ref_slots"])
    table = np.zeros(1, _lib.COV_KEYFRAME_DTYPE)
    table["n_keys"], table["slots"] = len(B["ref_slots"]), slots.data_ptr()
    D = {k: dev(B[k]) for k in ("keys", "desc", "depth", "n", "cam", "points", "n_points", "outlier", "decision", "point_bad", "point_observations")}
    D["table"], D["ref"], D["assigned0"] = dev(table), dev(np.zeros(S, np.int32)), dev(B["assigned"])
    D["no_depth"] = torch.zeros_like(D["depth"])
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
    O = dict(headers=z(S, 64), new_points=z(S, cap, 72), new_index=z(S, cap, dtype=torch.int32), n_new=z(S, dtype=torch.int32),
             depth_selected=z(S, cap, dtype=torch.float32), assigned=z(S, cap, dtype=torch.int32))
    stream = torch.cuda.Stream()
    ALL = tracking.KF_STATISTICS | tracking.KF_DECISION | tracking.KF_CREATE

    def timed(fn):
        ts = []
        with torch.cuda.stream(stream):
            for it in range(a.iters + 5):
                O["assigned"].copy_(D["assigned0"])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if it >= 5:
                    ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    def launch(flags=ALL, depth=None, mode=tracking.KF_MODE_KEYFRAME, sc=None, slots=True):   # timed() resets the slots outside the events
        tracking.keyframe_insertion_device(
            scales if sc is None else sc, flags, mode, S=S, cap=cap, new_cap=cap, depth=D["depth"] if depth is None else depth, n=D["n"],
            headers=O["headers"], keys_un=D["keys"], desc=D["desc"], cam=D["cam"], assigned=O["assigned"] if slots else None, points=D["points"],
            n_points=D["n_points"], p_cap=p_cap, outlier=D["outlier"], decision=D["decision"], ref_kf=D["ref"], keyframes=D["table"], n_kf=1,
            point_bad=D["point_bad"], point_observations=D["point_observations"], n_map_points=4096, new_points=O["new_points"],
            new_index=O["new_index"], n_new=O["n_new"], depth_selected=O["depth_selected"], stream=stream)

    with torch.cuda.stream(stream):
        O["assigned"].copy_(D["assigned0"])
        launch()
    stream.synchronize()
    H = O["headers"].cpu().numpy().reshape(-1).view(_lib.KF_HEADER_DTYPE)
    assert (H["status"] == tracking.KF_OK).all() and (H["need"] == 1).all()
    got_n, got_rec = O["n_new"].cpu().numpy(), O["new_points"].cpu().numpy().reshape(S, cap * 72).view(_lib.MAP_POINT_DTYPE).reshape(S, cap)
    got_idx = O["new_index"].cpu().numpy()
    t_all = timed(launch)
    t_nodepth = timed(lambda: launch(depth=D["no_depth"]))
    t_stats = timed(lambda: launch(flags=tracking.KF_STATISTICS | tracking.KF_DECISION))
    t_init = timed(lambda: launch(flags=tracking.KF_CREATE, mode=tracking.KF_MODE_STEREO_INIT, slots=False))
    H_init = O["headers"].cpu().numpy().reshape(-1).view(_lib.KF_HEADER_DTYPE).copy()
    far = tracking.pack_scales([1.2 ** k for k in range(8)], 1e30)   # every candidate is close: the whole order is the prefix
    t_sorted = timed(lambda: launch(flags=tracking.KF_CREATE, sc=far, slots=False))
    sparse = D["depth"] * (torch.rand(D["depth"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < 0.3)
    t_sparse = timed(lambda: launch(flags=tracking.KF_CREATE, sc=far, slots=False, depth=sparse))
    M_sparse = float(O["headers"].cpu().numpy().reshape(-1).view(_lib.KF_HEADER_DTYPE)["M"].mean())
    t_sparse_init = timed(lambda: launch(flags=tracking.KF_CREATE, mode=tracking.KF_MODE_STEREO_INIT, slots=False, depth=sparse))

    # (b) the host route: download, numpy, upload
    up = torch.zeros((S, cap, 72), dtype=torch.uint8, device="cuda")
    walls = []
    for it in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Bh = dict(B, depth=D["depth"].cpu().numpy(), assigned=D["assigned0"].cpu().numpy(), outlier=D["outlier"].cpu().numpy())
        Bh["points"] = D["points"].cpu().numpy().reshape(S, p_cap * 72).view(_lib.MAP_POINT_DTYPE).reshape(S, p_cap)
        n_host, rec_host, idx_host = host_route(Bh, scales, cap)
        up.copy_(torch.from_numpy(rec_host.view(np.uint8).reshape(S, cap, 72)), non_blocking=False)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    same = bool(np.array_equal(n_host, got_n)) and all(
        got_rec[f, :got_n[f]].tobytes() == rec_host[f, :got_n[f]].tobytes() and np.array_equal(got_idx[f, :got_n[f]], idx_host[f, :got_n[f]])
        for f in range(S))
    rows = int(B["n"].sum())
    bytes_in = rows * (28 + 32 + 4 + 4 + 1) + int(H["n_created"].sum()) * 0 + S * cap * 4
    bytes_out = int(got_n.sum()) * (72 + 4 + 4) + S * cap * 4
    bound_us = (bytes_in + bytes_out) / (HBM_TBS * 1e12) * 1e6
    res = dict(frames=S, keys_mean=float(B["n"].mean()), cap=cap, candidates_mean=float(H["M"].mean()), close_mean=float(H["c"].mean()),
               prefix_mean=float(H["L"].mean()), created_mean=float(H["n_created"].mean()), cleared_mean=float(H["n_cleared"].mean()),
               call_us=dict(median=t_all[0], min=t_all[1], max=t_all[2]), call_no_candidates_us=dict(median=t_nodepth[0], min=t_nodepth[1], max=t_nodepth[2]),
               statistics_decision_only_us=dict(median=t_stats[0], min=t_stats[1], max=t_stats[2]),
               unsorted_all_candidates_us=dict(median=t_init[0], min=t_init[1], max=t_init[2], created_mean=float(H_init["n_created"].mean())),
               sorted_all_candidates_us=dict(median=t_sorted[0], min=t_sorted[1], max=t_sorted[2]),
               sparse_sorted_us=dict(median=t_sparse[0], min=t_sparse[1], max=t_sparse[2], candidates_mean=M_sparse),
               sparse_unsorted_us=dict(median=t_sparse_init[0], min=t_sparse_init[1], max=t_sparse_init[2]),
               byte_bound_us=bound_us,
               host_route_s=dict(median=float(np.median(walls)), min=float(np.min(walls))), records_equal_host_route=same, iters=a.iters,
               device=torch.cuda.get_device_name(0))
    print(f"batch: {S} frames, {res['keys_mean']:.0f} keypoints, {res['candidates_mean']:.0f} candidates, {res['close_mean']:.0f} close, prefix "
          f"{res['prefix_mean']:.0f}, {res['created_mean']:.0f} created ({res['cleared_mean']:.0f} temporal slots cleared)")
    print(f"(a) call alone        {t_all[0]:9.1f} us   (min {t_all[1]:.1f}, max {t_all[2]:.1f}; byte bound {bound_us:.1f} us)")
    print(f"(c) no candidates     {t_nodepth[0]:9.1f} us   statistics + decision only {t_stats[0]:.1f} us")
    print(f"    no sort, every candidate a record (initialisation mode) {t_init[0]:.1f} us for {res['unsorted_all_candidates_us']['created_mean']:.0f} records")
    print(f"    the same records WITH the sort (every candidate close, no slots) {t_sorted[0]:.1f} us: the sort of {res['candidates_mean']:.0f} keys in 2048 "
          f"takes {t_sorted[0] - t_init[0]:.1f} us")
    print(f"    {M_sparse:.0f} candidates per frame (keys padded to 512 or 1024, not to {cap}): sorted {t_sparse[0]:.1f} us, unsorted {t_sparse_init[0]:.1f} us")
    print(f"(b) host route        {np.median(walls) * 1e6:9.0f} us   records equal: {same}")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
