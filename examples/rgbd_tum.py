#!/usr/bin/env python3
"""RGB-D sequence driver for the ORB front end on a TUM RGB-D directory: Source/Examples/RGB-D/rgbd_tum.cc without the vocabulary.

Reads the association file (LoadImages, rgbd_tum.cc:171-200: `t rgb/<file>.png t depth/<file>.png` per line), the colour frames
with the library's zlib PNG reader converted as Tracking::GrabImageRGBD does for the settings file's Camera.RGB
(L/src/Tracking.cc:193-208), the 16-bit depth maps unchanged, and pushes every frame through the per-frame hot path of an RGB-D
tracker:
    ORBextractor -> Frame::UndistortKeyPoints + ComputeStereoFromRGBD (L/src/Frame.cc:157-159; the depth map scaled by
    1 / DepthMapFactor as GrabImageRGBD does) -> Frame::UnprojectStereo of the points with depth -> SearchByProjection(cur, last,
    th = 15) against the previous frame with the constant-velocity prediction Tcw = Tlw (L/src/Tracking.cc:780-805)
on the device, the image bounds of ComputeImageBounds (L/src/Frame.cc:447-476) in every search.  Prints the examples' timing report
("median tracking time" / "mean tracking time") for the front end; pose optimisation, local mapping and loop closing are out of scope.

  per-frame  (default)  one frame at a time, like the reference's loop
  --batch F             F frames per launch through the device-resident batch API; the last frame of a batch is carried into the next
  --dump FILE.npz       per frame i: kp_i (mvKeys), kpu_i (mvKeysUn), desc_i, ur_i (mvuRight), depth_i (mvDepth), assigned_i, ntrack_i

usage: rgbd_tum.py <settings.yaml> <sequence_dir> <association_file> [--batch F] [--max-frames N] [--dump FILE.npz]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_images(association: str):
    """LoadImages of rgbd_tum.cc:171-200: (rgb files, depth files, timestamps)."""
    rgb, depth, times = [], [], []
    with open(association) as f:
        for line in f:
            parts = line.split()
            if len(parts) < 4:
                continue
            times.append(float(parts[0])); rgb.append(parts[1]); depth.append(parts[3])
    return rgb, depth, times


def read_gray(path: str, out: np.ndarray, camera_rgb: int):
    from refactored_orb_slam2_amd import _lib
    w, h = C.c_int(0), C.c_int(0)
    L = _lib.lib()
    L.orbfe_png_read_gray2.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    _lib.check(L.orbfe_png_read_gray2(path.encode(), out.ctypes.data_as(C.c_void_p), out.strides[0], out.shape[0], C.byref(w), C.byref(h),
                                      int(camera_rgb)), "orbfe_png_read_gray2")
    if (h.value, w.value) != out.shape:
        raise ValueError(f"{path}: {w.value}x{h.value}, expected {out.shape[1]}x{out.shape[0]}")


def read_depth(path: str, out: np.ndarray):
    from refactored_orb_slam2_amd import _lib
    w, h = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().orbfe_png_read_gray16(path.encode(), out.ctypes.data_as(C.c_void_p), out.strides[0] // 2, out.shape[0], C.byref(w),
                                                C.byref(h)), "orbfe_png_read_gray16")
    if (h.value, w.value) != out.shape:
        raise ValueError(f"{path}: {w.value}x{h.value}, expected {out.shape[1]}x{out.shape[0]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings")
    ap.add_argument("sequence_dir")
    ap.add_argument("association")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--dump", default="")
    args = ap.parse_args()

    import torch
    from refactored_orb_slam2_amd import ORBextractor, _lib, camera
    from refactored_orb_slam2_amd._lib import KP_DTYPE, TRACK_POSE_DTYPE, UNPROJECT_CAM_DTYPE
    from refactored_orb_slam2_amd.matcher import Matcher, track_queries_stereo_batch

    s = camera.read_settings(args.settings)
    cal, xp = s["calibration"], s["extractor"]
    rgb, dep, times = load_images(args.association)
    n_all = len(times) if args.max_frames <= 0 else min(len(times), args.max_frames)
    print(f"\n-------\nStart processing sequence ...\nImages in the sequence: {n_all}\n")
    L = _lib.lib()
    w, h = C.c_int(0), C.c_int(0)
    _lib.check(L.orbfe_png_info(os.path.join(args.sequence_dir, rgb[0]).encode(), C.byref(w), C.byref(h)), "orbfe_png_info")
    w, h = w.value, h.value
    dev = torch.device("cuda", 0)
    ex = ORBextractor(xp["n_features"], xp["scale_factor"], xp["n_levels"], xp["ini_th_fast"], xp["min_th_fast"], device=0)
    mt = Matcher(0)
    cap = ex.max_keypoints(w, h)
    sf = ex.GetScaleFactors()
    bounds = camera.image_bounds(cal, w, h)   # ComputeImageBounds: every search of this camera takes these
    F = max(args.batch, 1)
    z = lambda *sh, dt=torch.uint8: torch.zeros(sh, dtype=dt, device=dev)
    kps, desc, n = z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32)
    kpu, ur, depth, n_depth = z(F, cap, 28), z(F, cap, dt=torch.float32), z(F, cap, dt=torch.float32), z(F, dt=torch.int32)
    q, nq = z(F, cap, 68), z(F, dt=torch.int32)
    blocked, assigned, ntr = z(F, cap), z(F, cap, dt=torch.int32), z(F, dt=torch.int32)
    carry = (z(cap, 28), z(cap, 32), z(1, dt=torch.int32), z(cap, dt=torch.float32), z(64))   # the last frame of the batch before
    # constant-velocity prediction with zero velocity: the current pose equals the last one (identity in the last camera's frame)
    cams = np.zeros(F, UNPROJECT_CAM_DTYPE); poses = np.zeros(F, TRACK_POSE_DTYPE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    cams["Rwc"] = eye; cams["cx"] = cal.cx; cams["cy"] = cal.cy
    cams["invfx"] = np.float32(1) / np.float32(cal.fx); cams["invfy"] = np.float32(1) / np.float32(cal.fy)
    poses["Rcw"] = eye; poses["fx"] = cal.fx; poses["fy"] = cal.fy; poses["cx"] = cal.cx; poses["cy"] = cal.cy; poses["mbf"] = cal.mbf
    poses["min_x"], poses["max_x"], poses["min_y"], poses["max_y"] = bounds
    poses["th"] = 15.0   # RGB-D: th = 15 (L/src/Tracking.cc:793-798)
    poses["scale_factors"][:, :len(sf)] = sf
    t_cams = torch.from_numpy(cams.view(np.uint8).reshape(F, -1)).to(dev)
    t_poses = torch.from_numpy(poses.view(np.uint8).reshape(F, -1)).to(dev)
    stream = torch.cuda.Stream(dev)
    imgs = np.empty((F, h, w), np.uint8); maps = np.empty((F, h, w), np.uint16)
    track_times, n_kp, n_dp, n_tr = [], 0, 0, 0
    dump = {}
    have_prev = False
    for b in range(0, n_all, F):
        idx = list(range(b, min(b + F, n_all)))
        B = len(idx)
        for j, i in enumerate(idx):
            read_gray(os.path.join(args.sequence_dir, rgb[i]), imgs[j], s["camera_rgb"])
            read_depth(os.path.join(args.sequence_dir, dep[i]), maps[j])
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            d_img = torch.from_numpy(imgs[:B]).to(dev, non_blocking=True)
            d_map = torch.from_numpy(maps[:B].view(np.int16)).to(dev, non_blocking=True)   # 16-bit samples; torch has no uint16 arithmetic
            ex.extract_batch_device(d_img, kps[:B], desc[:B], n[:B], stream=stream)
            camera.undistort_frames_batch(kps[:B], n[:B], cal, camera.DEPTH_U16, d_map, kpu[:B], ur[:B], depth[:B], n_depth[:B], stream)
            # queries of frame j from the undistorted keypoints / depth of frame j - 1 (UnprojectStereo reads mvKeysUn)
            track_queries_stereo_batch(kpu[:B], desc[:B], n[:B], depth[:B], t_cams[:B], 1, t_poses[:B], 1, q[:B], nq[:B], stream,
                                       carry=carry if have_prev else None)
            blocked[:B].zero_(); assigned[:B].fill_(-1)
            mt.proj_match_batch(kpu[:B], desc[:B], n[:B], ur[:B], bounds, q[:B], nq[:B], 1, 0.9, True, blocked[:B], assigned[:B], ntr[:B],
                                stream=stream)
            if not have_prev:   # the first frame has no predecessor
                ntr[0] = 0; assigned[0].fill_(-1)
            for c, src in zip(carry, (kpu[B - 1], desc[B - 1], n[B - 1:B], depth[B - 1], t_cams[B - 1])):
                c.copy_(src)
        stream.synchronize()
        dt = time.perf_counter() - t0
        track_times += [dt / B] * B
        n_kp += int(n[:B].sum()); n_dp += int(n_depth[:B].sum()); n_tr += int(ntr[:B].sum())
        if args.dump:
            for j, i in enumerate(idx):
                m = int(n[j])
                dump[f"kp_{i}"] = kps[j, :m].cpu().numpy().reshape(-1).view(KP_DTYPE)
                dump[f"kpu_{i}"] = kpu[j, :m].cpu().numpy().reshape(-1).view(KP_DTYPE)
                dump[f"desc_{i}"] = desc[j, :m].cpu().numpy()
                dump[f"ur_{i}"] = ur[j, :m].cpu().numpy(); dump[f"depth_{i}"] = depth[j, :m].cpu().numpy()
                dump[f"assigned_{i}"] = assigned[j, :m].cpu().numpy(); dump[f"ntrack_{i}"] = np.int32(int(ntr[j]))
        have_prev = True
    if args.dump:
        dump["bounds"] = np.array(bounds, np.float32)
        np.savez_compressed(args.dump, **dump)
    track_times.sort()
    print("-------\n")
    print(f"median tracking time: {track_times[len(track_times) // 2]}")
    print(f"mean tracking time: {sum(track_times) / len(track_times)}")
    print(f"frames: {n_all}, keypoints/frame: {n_kp / n_all:.1f}, depth points/frame: {n_dp / n_all:.1f}, "
          f"tracked/frame: {n_tr / max(n_all - 1, 1):.1f}, front-end frames/s (incl. H2D, excl. PNG decoding): "
          f"{len(track_times) / sum(track_times):.1f}")
    ex.close(); mt.close()


if __name__ == "__main__":
    main()
