#!/usr/bin/env python3
"""First measurements of the vocabulary training at ORBvoc's shape (k = 10, L = 6) on unstructured descriptors that are made on the
device: wall time, rounds and the form that took the segments, per level.

    python tools/vocab_train_rate.py --frames 3000 --cap 1000 [--out profiles/vocabulary_training.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--cap", type=int, default=1000, help="descriptors per frame")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("-L", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--wide-min", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=2, help="timed runs after one warm-up run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch
    from refactored_orb_slam2_amd.vocabulary import ORBVocabulary
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    desc = torch.randint(0, 256, (args.frames, args.cap, 32), dtype=torch.uint8, device=dev, generator=g)
    counts = torch.full((args.frames,), args.cap, dtype=torch.int32, device=dev)
    runs = []
    for it in range(args.repeat + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        voc = ORBVocabulary.create((desc, counts), args.k, args.L, seed=args.seed, wide_min=args.wide_min)
        seconds = time.perf_counter() - t0
        levels = voc.train_levels()
        if it > 0:   # the first run pays for code-object loading and the allocator
            runs.append({"seconds": seconds, "levels": levels})
        stats = voc.train_stats
        voc.close()
    best = min(runs, key=lambda r: r["seconds"])
    print(f"{args.frames * args.cap} descriptors, k = {args.k}, L = {args.L}: {best['seconds']:.3f} s (best of {len(runs)}); "
          f"{stats['n_nodes']} nodes, {stats['n_words']} words, max rounds {stats['max_rounds']}, capped {stats['n_capped_nodes']}")
    for lv in best["levels"]:
        print("  level {level}: {ms:10.2f} ms, {rounds:4d} rounds, segments: {wide} wide, {narrow} narrow, {trivial} trivial".format(**lv))
    result = {"n_descriptors": args.frames * args.cap, "k": args.k, "L": args.L, "seed": args.seed, "wide_min": args.wide_min,
              "seconds": [r["seconds"] for r in runs], "levels": best["levels"], "stats": stats}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
