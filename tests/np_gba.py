"""The scenes of the global bundle adjustment across the device (tests/test_gba_cpu.py, tests/test_gba_gpu.py).  The yardstick is
tests/np_ba.optimize, which takes any number of keyframes; nothing of the reading is restated here.

np_ba.make_scene's tracks span 2 - 6 consecutive keyframes, so its reduced system is a band around the diagonal.  long_tracks() adds,
for a share of the points, ONE more monocular observation from a keyframe 10 - 40 rows before the point's first observer: the
projection of the input point from poses_true (no pixel noise, octave 0), kept if the depth exceeds 1 m and it falls in the image.  It is
inserted in front of the point's edges, so the list stays point by point with keyframes ascending.  That puts blocks far off the
band and into off-diagonal tiles of the factorisation."""
from __future__ import annotations

import functools

import numpy as np

from tests import np_ba as B
from tests.np_lba import EDGE_DTYPE

F32 = np.float32
IMAGE = (1241.0, 376.0)                        # KITTI, the camera of np_lba.make_scene
LONG_SHARE = 0.2


def long_tracks(s, seed, share=LONG_SHARE):
    """the scene with its long tracks; s["n_long"] counts them"""
    rng = np.random.default_rng(seed + 77)
    cam, e = s["cam"], s["edges"]
    T = np.asarray(s["poses_true"], np.float64).reshape(-1, 3, 4)
    n_pt = len(s["points"])
    X = np.asarray(s["points"], np.float64)    # make_scene hands out no true points: the input point (truth + point_noise) is projected
    first = np.full(n_pt, -1)
    for i in range(len(e) - 1, -1, -1):
        first[e["point"][i]] = e["kf"][i]
    rows, n_long = [], 0
    chosen = rng.uniform(size=n_pt) < share
    back = rng.integers(10, 41, n_pt)
    start = np.searchsorted(e["point"], np.arange(n_pt), "left")
    end = np.searchsorted(e["point"], np.arange(n_pt), "right")
    for p in range(n_pt):
        k = first[p] - back[p]
        if chosen[p] and first[p] >= 0 and k >= 0:
            c = T[k, :, :3] @ X[p] + T[k, :, 3]
            if c[2] > 1.0:
                u, v = c[0] / c[2] * cam["fx"] + cam["cx"], c[1] / c[2] * cam["fy"] + cam["cy"]
                if 0.0 <= u < IMAGE[0] and 0.0 <= v < IMAGE[1]:
                    rows.append(np.array([(k, p, u, v, -1.0, 1.0)], EDGE_DTYPE))
                    n_long += 1
        rows.append(e[start[p]:end[p]])
    out = dict(s)
    out["edges"] = np.concatenate(rows) if rows else e
    out["n_long"] = n_long
    return out


# name -> (seed, free keyframes, fixed keyframes, long tracks?, n_iterations, robust); five points per free keyframe.  The first
# seven are the cases the feature was specified with; tile_* stand on the edges of ORBFE_GBA_TILE_KEYFRAMES = 8 (the smallest m with
# 8 m - 1 > 64 is 9) and past_256 has more than ORBFE_LBA_MAX_KEYFRAMES keyframes in all.  Seeds of the added cases: the case's free
# keyframes x 100, the first ones tried.
CASES = {
    "plain_65": (6500, 65, 1, False, 3, True),
    "plain_96": (9600, 96, 1, False, 3, True),
    "plain_129": (12900, 129, 1, False, 2, False),
    "plain_255": (25600, 255, 1, False, 2, True),
    "long_65": (6500, 65, 1, True, 3, True),
    "long_72_robust_5": (7200, 72, 1, True, 5, True),
    "long_97_plain": (9700, 97, 1, True, 3, False),
    "tile_71": (7100, 71, 1, True, 2, False),
    "tile_72": (7200, 72, 1, True, 2, True),
    "tile_73": (7300, 73, 1, True, 2, True),
    "past_256": (25500, 255, 3, True, 2, False),
}
GPU_CASES = ("long_65", "tile_71", "tile_72", "tile_73", "long_97_plain", "past_256")


def make_scene(seed, n_free, n_fixed=1, long=True):
    s = B.make_scene(seed, n_free=n_free, n_fixed=n_fixed, n_points=5 * n_free)
    return long_tracks(s, seed) if long else s


@functools.lru_cache(maxsize=None)
def case_scene(name):
    seed, n_free, n_fixed, long, n_it, robust = CASES[name]
    s = make_scene(seed, n_free, n_fixed, long)
    s["n_iterations"], s["robust"] = n_it, robust
    return s


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reading of a case, computed once and shared; treat it as read-only"""
    return B.run_scene(case_scene(name))


@functools.lru_cache(maxsize=None)
def nan_scene():
    """65 free keyframes, 325 points, one coordinate NaN: every trial of the four robust iterations is rejected"""
    s = dict(B.make_scene(6500, n_free=65, n_points=325))
    s["points"] = s["points"].copy()
    s["points"][7, 1] = np.nan
    s["n_iterations"], s["robust"] = 4, True
    return s
