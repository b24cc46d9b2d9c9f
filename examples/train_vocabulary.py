#!/usr/bin/env python3
"""Train a DBoW2 vocabulary on the device: the counterpart of DBoW2's demo that calls TemplatedVocabulary::create, for users with their
own camera or without ORBvoc.txt.

    python examples/train_vocabulary.py IMAGE_DIR --out myvoc.txt          # every *.png of a directory (one size)
    python examples/train_vocabulary.py --synthetic 200 --out synth.bin    # 200 rendered frames (refactored_orb_slam2_amd.synth)

The images are extracted on the device in batches, the descriptors stay in HBM as orbfe_extract_batch_device leaves them, and
orbfe_vocabulary_train_device clusters them there.  A file name ending in .bin is written in the reference's binary format, anything
else in the text format of ORBvoc.txt.  Prints the statistics and the time per level."""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_png(L, _lib, path, out):
    w, h = C.c_int(0), C.c_int(0)
    _lib.check(L.orbfe_png_read_gray(path.encode(), out.ctypes.data_as(C.c_void_p), out.strides[0], out.shape[0], C.byref(w), C.byref(h)),
               "orbfe_png_read_gray")
    if (h.value, w.value) != out.shape:
        raise ValueError(f"{path}: {w.value}x{h.value}, expected {out.shape[1]}x{out.shape[0]}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("image_dir", nargs="?", help="directory of equally sized PNG images")
    ap.add_argument("--synthetic", type=int, default=0, metavar="F", help="render F frames instead of reading a directory")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--features", type=int, default=1000, help="ORBextractor.nFeatures")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("-L", type=int, default=5)
    ap.add_argument("--weighting", type=int, default=0, help="0 TF_IDF, 1 TF, 2 IDF, 3 BINARY")
    ap.add_argument("--scoring", type=int, default=0, help="0 L1_NORM .. 5 DOT_PRODUCT")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=16, help="images per extraction batch")
    ap.add_argument("--out", default="vocabulary.txt")
    args = ap.parse_args(argv)
    if bool(args.image_dir) == bool(args.synthetic):
        ap.error("give IMAGE_DIR or --synthetic F")

    import torch
    from refactored_orb_slam2_amd import ORBextractor, _lib, synth
    from refactored_orb_slam2_amd.vocabulary import ORBVocabulary
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    if args.synthetic:
        w, h, n_frames = args.width, args.height, args.synthetic
        files = None
    else:
        files = sorted(glob.glob(os.path.join(args.image_dir, "*.png")))
        if not files:
            raise SystemExit(f"no *.png in {args.image_dir}")
        cw, ch = C.c_int(0), C.c_int(0)
        _lib.check(L.orbfe_png_info(files[0].encode(), C.byref(cw), C.byref(ch)), "orbfe_png_info")
        w, h, n_frames = cw.value, ch.value, len(files)

    ex = ORBextractor(args.features, 1.2, 8, 20, 7, device=0)
    cap = ex.max_keypoints(w, h)
    desc = torch.zeros((n_frames, cap, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(n_frames, dtype=torch.int32, device=dev)
    kps = torch.zeros((args.batch, cap, 28), dtype=torch.uint8, device=dev)
    host = np.zeros((args.batch, h, w), np.uint8)
    stream = torch.cuda.Stream(dev)
    t0 = time.perf_counter()
    for b in range(0, n_frames, args.batch):
        nb = min(args.batch, n_frames - b)
        for i in range(nb):
            if files is None:
                host[i] = synth.frame(w, h, seq=(b + i) // 8, f=(b + i) % 8)
            else:
                read_png(L, _lib, files[b + i], host[i])
        imgs = torch.from_numpy(host[:nb]).to(dev)
        ex.extract_batch_device(imgs, kps[:nb], desc[b:b + nb], counts[b:b + nb], stream=stream)
        stream.synchronize()
    ex.device_status()
    t_extract = time.perf_counter() - t0
    n_desc = int(counts.sum().item())
    print(f"{n_frames} images of {w}x{h}: {n_desc} descriptors in {t_extract:.2f} s")

    t0 = time.perf_counter()
    voc = ORBVocabulary.create((desc, counts), args.k, args.L, weighting=args.weighting, scoring=args.scoring, seed=args.seed)
    t_train = time.perf_counter() - t0
    if args.out.endswith(".bin"):
        voc.saveToBinaryFile(args.out)
    else:
        voc.saveToTextFile(args.out)
    print(f"trained k = {args.k}, L = {args.L} in {t_train:.3f} s -> {args.out}")
    for lv in voc.train_levels():
        print("  level {level}: {ms:9.2f} ms, {rounds:4d} rounds, segments: {wide} wide, {narrow} narrow, {trivial} trivial".format(**lv))
    print(json.dumps({"n_images": n_frames, "n_descriptors": n_desc, "train_seconds": t_train, **voc.train_stats}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
