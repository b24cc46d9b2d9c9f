#!/usr/bin/env python3
"""Writes a synthetic stereo sequence in the EuRoC directory layout for examples/stereo_euroc.py: <dir>/cam0/data/<stamp>.png,
<dir>/cam1/data/<stamp>.png (8-bit grey, taken as RAW, unrectified camera images) and the time-stamp file <dir>/stamps.txt (one
stamp in nanoseconds per line, 20 frames/s, as Source/Examples/Stereo/EuRoC_TimeStamps/*.txt).

usage: python tools/make_euroc_layout.py <dir> <pairs> [--width 752 --height 480 --seq 5]
"""
import argparse
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_png_gray(path, img, level=6):
    """8-bit greyscale PNG, filter 0"""
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    h, w = img.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows, level)) + chunk(b"IEND", b""))


def write_layout(root, pairs, first_stamp=1403636579763555584, step=50000000):
    """pairs: [(left, right)] uint8 images -> the stamps written"""
    for cam in ("cam0", "cam1"):
        os.makedirs(os.path.join(root, cam, "data"), exist_ok=True)
    stamps = [first_stamp + i * step for i in range(len(pairs))]
    with open(os.path.join(root, "stamps.txt"), "w") as f:
        for s, (left, right) in zip(stamps, pairs):
            write_png_gray(os.path.join(root, "cam0", "data", f"{s}.png"), left)
            write_png_gray(os.path.join(root, "cam1", "data", f"{s}.png"), right)
            f.write(f"{s}\n")
    return stamps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("pairs", type=int)
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--seq", type=int, default=5)
    a = ap.parse_args()
    from refactored_orb_slam2_amd import synth
    write_layout(a.dir, synth.sequence(a.width, a.height, a.pairs, seq=a.seq, stereo=True))


if __name__ == "__main__":
    main()
