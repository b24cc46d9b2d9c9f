#!/usr/bin/env python3
"""HIP-event time of stereo rectification, device-resident: 256 synthetic EuRoC pairs (512 images of 752 x 480, the LEFT / RIGHT
calibration of tests/golden/euroc_stereo.yaml, 1 200 features).  Reports, as medians over the repetitions on one stream, in one JSON
line (profiles/rectify.md):
    rectify_ms      orbfe_rectify_batch_device of the 512 images (one launch per eye), its bytes (source + destination once, the two
                    fixed-point maps once per launch) and GB/s
    copy_ms         a plain device-to-device copy of the same 512 images in the same process: the floor of anything that reads and
                    writes each image once; rectify_over_copy is the ratio
    extract_ms      the extraction of the same 512 images (left + right extractor, one stream) and the rectification's share of it
    pipeline_*      frames/s of the pipeline handle on resident chunks of 256 pairs with and without the rectification stage

usage: python tools/rectify_rate.py [--frames 256] [--reps 30] [--warmup 5] [--pipeline-chunks 12]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refactored_orb_slam2_amd import _lib  # noqa: E402
if os.environ.get("ORBFE_AB_LIB"): _lib.LIB_PATH = os.path.join(_lib.CSRC, "_ab", "liborbfe_%s.so" % os.environ["ORBFE_AB_LIB"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pipeline-chunks", type=int, default=12)
    args = ap.parse_args()
    import torch
    from refactored_orb_slam2_amd import ORBextractor, camera, synth
    from refactored_orb_slam2_amd.pipeline import OUT_COUNTS, StereoPipeline
    from refactored_orb_slam2_amd.rectify import rectifiers_from_settings

    settings = os.path.join(ROOT, "tests", "golden", "euroc_stereo.yaml")
    st = camera.read_settings(settings)
    cal, ep = st["calibration"], st["extractor"]
    W, H, F, NF = st["width"], st["height"], args.frames, ep["n_features"]
    rl, rr = rectifiers_from_settings(settings, device=0)
    base = synth.sequence(W, H, 16, seq=9, stereo=True)
    left = np.stack([base[i % 16][0] for i in range(F)])
    right = np.stack([base[i % 16][1] for i in range(F)])
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        raw = torch.from_numpy(np.stack([left, right])).to(dev)           # (2, F, H, W)
        rect = torch.zeros_like(raw)
        cpy = torch.zeros_like(raw)
        exL, exR = (ORBextractor(NF, ep["scale_factor"], ep["n_levels"], ep["ini_th_fast"], ep["min_th_fast"], device=0) for _ in range(2))
        cap = exL.max_keypoints(W, H)
        z = lambda *sh, dt=torch.uint8: torch.zeros(sh, dtype=dt, device=dev)
        kl, dl, nl, kr, dr, nr = z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32), z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32)
    s.synchronize()

    def rectify():
        rl.rectify_batch(raw[0], rect[0], s)
        rr.rectify_batch(raw[1], rect[1], s)

    def copy():
        cpy.copy_(raw)

    def extract():
        exL.extract_batch_device(rect[0], kl, dl, nl, stream=s)
        exR.extract_batch_device(rect[1], kr, dr, nr, stream=s)

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

    rect_med, rect_min = timed(rectify)
    copy_med, copy_min = timed(copy)
    ext_med, _ = timed(extract)
    s.synchronize()
    cov = (rl.coverage(), rr.coverage())
    map_bytes = 2 * 6 * ((W + 3) // 4 * 4) * H
    nbytes = 2 * raw.numel() + map_bytes
    res = {"frames": F, "images": 2 * F, "width": W, "height": H, "features": NF, "reps": args.reps,
           "coverage_left": cov[0], "coverage_right": cov[1],
           "rectify_ms": round(rect_med, 4), "rectify_min_ms": round(rect_min, 4), "rectify_bytes": nbytes,
           "rectify_GBps": round(nbytes / rect_med / 1e6, 1),
           "copy_ms": round(copy_med, 4), "copy_min_ms": round(copy_min, 4), "copy_GBps": round(2 * raw.numel() / copy_med / 1e6, 1),
           "rectify_over_copy": round(rect_med / copy_med, 3),
           "extract_ms": round(ext_med, 4), "rectify_share_of_extract": round(rect_med / ext_med, 4),
           "keypoints_per_left_image": round(float(nl.sum()) / F, 1)}
    exL.close(); exR.close()
    del raw, rect, cpy, kl, dl, kr, dr

    # the pipeline handle on resident chunks: three slots, the images uploaded once, counts only copied out
    def pipeline_rate(with_rectifiers):
        with StereoPipeline(W, H, F, cal.fx, cal.fy, cal.cx, cal.cy, cal.mbf, 7.0, n_features=NF, scale_factor=ep["scale_factor"],
                            n_levels=ep["n_levels"], ini_th=ep["ini_th_fast"], min_th=ep["min_th_fast"], slots=3,
                            output_mask=OUT_COUNTS) as p:
            if with_rectifiers:
                p.set_rectifiers(rl, rr)
            for k in range(3):
                p.left(k)[:, :, :W] = left
                p.right(k)[:, :, :W] = right
                p.submit(k, F, has_predecessor=k > 0)
            for k in range(3):
                p.wait(k)
            t0 = time.perf_counter()
            for c in range(args.pipeline_chunks):
                k = c % 3
                p.wait(k)
                p.submit_resident(k, F, has_predecessor=True)
            for k in range(3):
                p.wait(k)
            dt = time.perf_counter() - t0
            tracked = int(p.output(0)["n_tracked"].sum())
        return args.pipeline_chunks * F / dt, tracked

    if args.pipeline_chunks <= 0:   # the kernel A/B alone
        print(json.dumps(res))
        return
    fps_plain, _ = pipeline_rate(False)
    fps_rect, tracked = pipeline_rate(True)
    res.update({"pipeline_chunks": args.pipeline_chunks, "pipeline_frames_per_s": round(fps_plain, 1),
                "pipeline_rectified_frames_per_s": round(fps_rect, 1), "pipeline_rectified_over_plain": round(fps_rect / fps_plain, 4),
                "tracked_in_a_chunk": tracked})
    print(json.dumps(res))
    rl.close(); rr.close()


if __name__ == "__main__":
    main()
