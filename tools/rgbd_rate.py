#!/usr/bin/env python3
"""HIP-event time of the RGB-D step, device-resident: 256 synthetic 640 x 480 frames, 1 000 features, the TUM1 RGB-D calibration
(Source/Examples/RGB-D/TUM1.yaml) and a 16-bit depth map per frame.  The step is what examples/rgbd_tum.py runs per batch:
    extract -> orbfe_undistort_frames_device (U16) -> orbfe_track_queries_stereo_device (keys_un, depth) -> orbfe_proj_match_batch_device
Reports, as medians over the repetitions, the new kernel alone (`undistort_ms`), the extraction alone (`extract_ms`) and the whole
step (`step_ms`), per 256 frames, in one JSON line.  profiles/rgbd_step.md.

usage: python tools/rgbd_rate.py [--frames 256] [--reps 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from refactored_orb_slam2_amd import ORBextractor, camera, synth
    from refactored_orb_slam2_amd._lib import TRACK_POSE_DTYPE, UNPROJECT_CAM_DTYPE
    from refactored_orb_slam2_amd.matcher import Matcher, track_queries_stereo_batch

    W, H, F = 640, 480, args.frames
    cal = camera.calibration(517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314,
                             40.0, 5000.0)
    bounds = camera.image_bounds(cal, W, H)
    base = synth.sequence(W, H, 16, seq=7)
    imgs = np.stack([base[i % 16] for i in range(F)])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    raw = np.stack([np.rint((2.0 + 0.8 * np.sin(xx / 83.0 + 0.1 * f) * np.cos(yy / 61.0)) * 5000).astype(np.uint16) for f in range(16)])
    maps = np.stack([raw[i % 16] for i in range(F)])
    dev = torch.device("cuda", 0)
    ex, mt = ORBextractor(1000, device=0), Matcher(0)
    cap = ex.max_keypoints(W, H)
    sf = ex.GetScaleFactors()
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)
    kps, desc, n = z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32)
    kpu, ur, dep, nd = z(F, cap, 28), z(F, cap, dt=torch.float32), z(F, cap, dt=torch.float32), z(F, dt=torch.int32)
    q, nq = z(F, cap, 68), z(F, dt=torch.int32)
    blocked, assigned, ntr = z(F, cap), z(F, cap, dt=torch.int32), z(F, dt=torch.int32)
    cams = np.zeros(F, UNPROJECT_CAM_DTYPE); poses = np.zeros(F, TRACK_POSE_DTYPE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    cams["Rwc"] = eye; cams["cx"] = cal.cx; cams["cy"] = cal.cy
    cams["invfx"] = np.float32(1) / np.float32(cal.fx); cams["invfy"] = np.float32(1) / np.float32(cal.fy)
    poses["Rcw"] = eye; poses["fx"] = cal.fx; poses["fy"] = cal.fy; poses["cx"] = cal.cx; poses["cy"] = cal.cy; poses["mbf"] = cal.mbf
    poses["min_x"], poses["max_x"], poses["min_y"], poses["max_y"] = bounds
    poses["th"] = 15.0; poses["scale_factors"][:, :len(sf)] = sf
    t_cams = torch.from_numpy(cams.view(np.uint8).reshape(F, -1)).to(dev)
    t_poses = torch.from_numpy(poses.view(np.uint8).reshape(F, -1)).to(dev)
    d_img = torch.from_numpy(imgs).to(dev)
    d_map = torch.from_numpy(maps.view(np.int16)).to(dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def undistort():
        camera.undistort_frames_batch(kps, n, cal, camera.DEPTH_U16, d_map, kpu, ur, dep, nd, s)

    def extract():
        ex.extract_batch_device(d_img, kps, desc, n, stream=s)

    def step():
        extract()
        undistort()
        track_queries_stereo_batch(kpu, desc, n, dep, t_cams, 1, t_poses, 1, q, nq, s)
        blocked.zero_(); assigned.fill_(-1)
        mt.proj_match_batch(kpu, desc, n, ur, bounds, q, nq, 1, 0.9, True, blocked, assigned, ntr, stream=s)

    def timed(fn):
        out = []
        with torch.cuda.stream(s):
            for r in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s); fn(); e1.record(s)
                e1.synchronize()
                if r >= args.warmup:
                    out.append(e0.elapsed_time(e1))
        return float(np.median(out)), float(np.min(out))

    with torch.cuda.stream(s):
        step()
    s.synchronize()
    und_med, und_min = timed(undistort)
    ext_med, _ = timed(extract)
    step_med, step_min = timed(step)
    s.synchronize()
    res = {"frames": F, "width": W, "height": H, "features": 1000, "reps": args.reps,
           "keypoints_per_frame": round(float(n.sum()) / F, 1), "depth_points_per_frame": round(float(nd.sum()) / F, 1),
           "tracked_per_frame": round(float(ntr[1:].sum()) / (F - 1), 1),
           "undistort_ms": round(und_med, 4), "undistort_min_ms": round(und_min, 4), "extract_ms": round(ext_med, 4),
           "step_ms": round(step_med, 4), "step_min_ms": round(step_min, 4),
           "undistort_share_of_extract": round(und_med / ext_med, 5), "step_frames_per_s": round(F / (step_med / 1000.0), 1)}
    print(json.dumps(res))
    ex.close(); mt.close()


if __name__ == "__main__":
    main()
