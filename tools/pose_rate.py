#!/usr/bin/env python3
"""HIP-event time of orbfe_pose_optimization_batch_device, device-resident: 256 frames of the *standard* scene of tests/np_pose.py
(1 000 edges among ~1 540 keypoint rows, 15 % gross outliers, 30 % monocular rows, the input pose 0.01 rad / 0.05 m off; 16 seeds
tiled) -- one launch per repetition, warm, median and minimum over the repetitions, in one JSON line.  `--edges` / `--outliers`
change the scene.  Frame 0 is checked against the numpy reading before anything is timed.  profiles/pose_optimization.md.
`--chain` times the call on what the device chain leaves in HBM instead: 16 synthetic 1241 x 376 stereo pairs (2 000 features) tiled
to 256 frames through extraction -> stereo matching -> UnprojectStereo -> track queries (frame_shift 1) -> projection search, then the
pose optimisation of every frame from the identity -- the inputs of tests/test_pose_gpu.py::test_chain_on_the_device_end_to_end.
A/B builds: ORBFE_AB_LIB=<name> (tools/ab_build.sh <name> "-DPO_THREADS=64" pose_kernels.hip).

usage: python tools/pose_rate.py [--frames 256] [--reps 60] [--warmup 10] [--edges 1000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib  # noqa: E402

if os.environ.get("ORBFE_AB_LIB"):
    _lib.LIB_PATH = os.path.join(_lib.CSRC, "_ab", "liborbfe_%s.so" % os.environ["ORBFE_AB_LIB"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--edges", type=int, default=1000)
    ap.add_argument("--outliers", type=float, default=0.15)
    ap.add_argument("--chain", action="store_true")
    args = ap.parse_args()
    if args.chain:
        return chain(args)
    import torch
    from refactored_orb_slam2_amd import optimizer
    from refactored_orb_slam2_amd._lib import KP_DTYPE, LAST_POINT_DTYPE, POSE_RESULT_DTYPE
    from tests import np_pose as P

    F = args.frames
    scenes = [P.make_scene(500 + i, n_edges=args.edges, outliers=args.outliers) for i in range(16)]
    cap = max(len(s["keys_xy"]) for s in scenes)
    p_cap = max(len(s["points"]) for s in scenes)
    kps, ur = np.zeros((F, cap), KP_DTYPE), np.full((F, cap), -1, np.float32)
    asg, pts = np.full((F, cap), -1, np.int32), np.zeros((F, p_cap), LAST_POINT_DTYPE)
    n, npts, T = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros((F, 12), np.float32)
    for f in range(F):
        s = scenes[f % 16]
        m = len(s["keys_xy"])
        kps["x"][f, :m], kps["y"][f, :m], kps["octave"][f, :m] = s["keys_xy"][:, 0], s["keys_xy"][:, 1], s["octave"]
        ur[f, :m], asg[f, :m], n[f], T[f] = s["u_right"], s["assigned"], m, s["Tcw_in"]
        pts["pos"][f, : len(s["points"])] = s["points"]
        npts[f] = len(s["points"])
    c = scenes[0]["cam"]
    cam = optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["inv_level_sigma2"])
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a)).to(dev)
    d = [up(a) for a in (kps, ur, n, asg, pts, npts, cam, T)]
    res = torch.zeros((F, POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    out = torch.zeros((F, cap), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)

    def run():
        optimizer.pose_optimization_batch(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], res, out, stream=s)

    run()
    s.synchronize()
    r = res.cpu().numpy().view(POSE_RESULT_DTYPE).reshape(-1)
    ref = P.run_case(scenes[0])
    if not (P.poses_agree(r[0]["Tcw"], ref["Tcw"]) and np.array_equal(out[0, : n[0]].cpu().numpy(), ref["outlier"])):
        raise SystemExit("frame 0 differs from the numpy reading: nothing is timed")
    times = []
    with torch.cuda.stream(s):
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); run(); e1.record(s)
            e1.synchronize()
            if k >= args.warmup:
                times.append(e0.elapsed_time(e1))
    s.synchronize()
    print(json.dumps({"tag": os.environ.get("ORBFE_AB_LIB", ""), "frames": F, "edges_per_frame": args.edges, "rows_per_frame": int(cap),
                      "reps": args.reps, "pose_ms": round(float(np.median(times)), 4), "pose_min_ms": round(float(np.min(times)), 4),
                      "pose_max_ms": round(float(np.max(times)), 4), "us_per_frame": round(float(np.median(times)) * 1000 / F, 3),
                      "iterations_per_frame": round(float(r["iterations"].mean()), 2),
                      "inliers_per_frame": round(float(r["n_inliers"].mean()), 1)}))


def chain(args):
    import torch
    from refactored_orb_slam2_amd import ORBextractor, optimizer, synth
    from refactored_orb_slam2_amd._lib import POSE_RESULT_DTYPE, TRACK_POSE_DTYPE, UNPROJECT_CAM_DTYPE
    from refactored_orb_slam2_amd.matcher import Matcher, track_queries_batch, unproject_stereo_batch

    W, H, NF, F = 1241, 376, 2000, args.frames
    bf, fx, fy, cx, cy = 386.1448, 718.856, 718.856, 607.1928, 185.2157
    pairs = synth.sequence(W, H, 16, seq=20, stereo=True)
    dev = torch.device("cuda", 0)
    exL, exR, mt = ORBextractor(NF, device=0), ORBextractor(NF, device=0), Matcher(0)
    cap, sf = exL.max_keypoints(W, H), exL.GetScaleFactors()
    cam = np.zeros(F, UNPROJECT_CAM_DTYPE); pose = np.zeros(F, TRACK_POSE_DTYPE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    cam["Rwc"] = eye; cam["cx"] = cx; cam["cy"] = cy; cam["invfx"] = np.float32(1) / np.float32(fx); cam["invfy"] = np.float32(1) / np.float32(fy)
    pose["Rcw"] = eye; pose["fx"] = fx; pose["fy"] = fy; pose["cx"] = cx; pose["cy"] = cy; pose["mbf"] = bf
    pose["max_x"] = W; pose["max_y"] = H; pose["th"] = 7.0; pose["scale_factors"][:, :len(sf)] = sf
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a)).to(dev)
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)
    kl, dl, nl, kr, dr, nr = z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32), z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32)
    ur, depth, nst = z(F, cap, dt=torch.float32), z(F, cap, dt=torch.float32), z(F, dt=torch.int32)
    pts, q, nq = z(F, cap, 60), z(F, cap, 68), z(F, dt=torch.int32)
    blocked, assigned, ntr = z(F, cap), z(F, cap, dt=torch.int32), z(F, dt=torch.int32)
    t_cams, t_poses = up(cam), up(pose)
    t_pcam = up(optimizer.pose_camera(fx, fy, cx, cy, bf, exL.GetInverseScaleSigmaSquares()))
    t_eye = up(np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (F, 1)))
    res, out = z(F, POSE_RESULT_DTYPE.itemsize), z(F, cap)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        dL = torch.from_numpy(np.stack([pairs[i % 16][0] for i in range(F)])).to(dev)
        dR = torch.from_numpy(np.stack([pairs[i % 16][1] for i in range(F)])).to(dev)
        exL.extract_batch_device(dL, kl, dl, nl, stream=s)
        exR.extract_batch_device(dR, kr, dr, nr, stream=s)
        mt.stereo_match(exL, exR, kl, dl, nl, kr, dr, nr, bf, bf / fx, ur, depth, nst, stream=s)
        unproject_stereo_batch(kl, dl, nl, depth, t_cams, 1, pts, s)
        track_queries_batch(t_poses, pts, nl, 1, q, nq, s)
        assigned.fill_(-1)
        mt.proj_match_batch(kl, dl, nl, ur, (0.0, float(W), 0.0, float(H)), q, nq, 1, 0.9, True, blocked, assigned, ntr, stream=s)
    s.synchronize()

    def run():
        optimizer.pose_optimization_batch(kl, ur, nl, assigned, pts, nl, t_pcam, t_eye, res, out, frame_shift=1, stream=s)

    times = []
    with torch.cuda.stream(s):
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); run(); e1.record(s)
            e1.synchronize()
            if k >= args.warmup:
                times.append(e0.elapsed_time(e1))
    s.synchronize()
    r = res.cpu().numpy().view(POSE_RESULT_DTYPE).reshape(-1)
    print(json.dumps({"tag": os.environ.get("ORBFE_AB_LIB", ""), "input": "chain", "frames": F, "rows_per_frame": round(float(nl.sum()) / F, 1),
                      "edges_per_frame": round(float(r["n_initial"].mean()), 1), "reps": args.reps,
                      "pose_ms": round(float(np.median(times)), 4), "pose_min_ms": round(float(np.min(times)), 4),
                      "pose_max_ms": round(float(np.max(times)), 4), "us_per_frame": round(float(np.median(times)) * 1000 / F, 3),
                      "iterations_per_frame": round(float(r["iterations"].mean()), 2),
                      "inliers_per_frame": round(float(r["n_inliers"].mean()), 1)}))
    for h in (exL, exR, mt):
        h.close()


if __name__ == "__main__":
    main()
