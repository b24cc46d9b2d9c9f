"""The ordered projection searches -- SearchByProjection(F, MapPoints) (L/src/ORBmatcher.cc:45-128), SearchByProjection(cur, last)
(:1289-1383) and SearchByProjection(F, KF, set, th, ORBdist) (:1439-1501) -- on DIRECTED input: a builder of scenes with hand-placed
keypoints and queries, and the census of what those scenes reach.

  proj_walk      tests/np_restatement.proj_walk -- the one body behind ref_search_by_projection_points / _frame / _keyframe -- with
                 its exit code per query and the facts the census reads
  build_scenes   the scenes of one (form, w, h); a scene is a frame (keypoints, descriptors, mvuRight, the slots taken before the
                 call) plus a query array and the exit every query was placed for.  Building a scene walks it and asserts the exits.
  census         the conditions tests/test_projection_cpu.py asserts on the walk's own exits and facts (never on the kernel's output)

No images: every descriptor is the scene's base pattern with chosen bits turned, keypoints in bits 0 .. 127 and queries in bits
156 .. 255 (or in named key bits), so every distance of a scene is the size of a known set.  UNRELATED descriptors are the
complement of the base pattern with at most two of bits 128 .. 155 turned: at least 129 bits from every keypoint and query placed
(Scene.finish asserts it).  Cases sit on sites 40 pixels apart with windows of a few pixels, so they meet only where placed.

What extracted frames with jitter reach and what the directed scenes of 640 x 480 reach, queries per exit and facts of the walk.
The first two columns are the inputs of tests/test_matcher_gpu.py::test_search_by_projection_frame at (640, 480, 1000) with th 15
(mode 1 with the rotation check) and ::test_search_by_projection_points at (640, 480, 1000) with th 3 and ratio 0.8 (mode 0),
rebuilt with the C oracle's extractor, whose keypoints and descriptors are the device's byte for byte:

  exit / fact                                    frame test   points test   directed frame   directed points   directed keyframe
  valid == 0                                             54            55             2438              2438                2438
  outside the grid                                        0             0             2438              2438                2438
  empty window                                           15            61             2438              2438                2438
  every index blocked or gated                            6           134              211               211                   4
  best distance > th_high                                68            86                4                 4                 249
  rejected by the ratio test                              -             7                -                 7                   -
  matched                                               689           789              721               634                 724
  matched, then overwritten                              95            71               43                40    - (all blocking)
  removed by the rotation check                          76             -               18                 -                  16
  largest depth                                          14            15              204               204                 204
  dependency across query 1023 -> 1024                   no           yes              yes               yes                 yes
  decision changed by a match of the call                 0             4                0                 2                   0
  largest n_window                                       19            14               65                65                  65
  windows of more than 64 (truncated lists)               0             0                6                 6                   6
  matters_kept == 4 / == 5                         119 / 61       89 / 44            3 / 1             3 / 1               3 / 1
  staged entries within 1024 queries                   1892           404            18000             18000               18000
  queries with a tie at the best distance                 8             1                3                 3                   3
  ... that index order would decide otherwise             4             1                2                 2                   2
  second-best distance tied across levels                 -             2                -                 2                   -
  best distance th_high - 1 / th_high / + 1       2 / 3 / 1     0 / 2 / 2        1 / 1 / 1         1 / 3 / 1         2 / 2 / 246
  cleared although the last taker's bin was kept         11             -                1                 -                   0
  rotation bins hit                                 0 .. 12             -          0 .. 12                 -             0 .. 12

The jittered frames reach more than the kernel's comment suggests (chains 14 and 15 deep, ties, both sides of TH_HIGH), but by
accident and without a test saying so; they reach no chain deeper than 15, no truncated list, no query outside the grid, and an
eighth of the staging area.  The directed columns are what test_projection_cpu.py asserts through census().

Bins 13 .. 29 of the rotation histogram, and with them the wrap "bin == HISTO_LENGTH", are unreachable: rot < 360 and the factor is
1 / HISTO_LENGTH (not HISTO_LENGTH / 360), so round(rot / 30) <= 12.  The census records bins 0 .. 12 and does not ask for more; the
kernel keeps the wrap because it mirrors the reference.
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import np_restatement as nr
from tests.np_restatement import (PX_SKIPPED, PX_OUTSIDE_GRID, PX_EMPTY_WINDOW, PX_ALL_GONE, PX_TOO_FAR, PX_RATIO, PX_MATCHED,  # noqa: F401
                                  PX_OVERWRITTEN, PX_ROTATION, TH_HIGH)
from tests.oracle_lib import KP_DTYPE, QUERY_DTYPE

EXIT_NAMES = {PX_SKIPPED: "valid == 0", PX_OUTSIDE_GRID: "outside the grid", PX_EMPTY_WINDOW: "empty window",
              PX_ALL_GONE: "every index blocked or gated", PX_TOO_FAR: "best distance > th_high", PX_RATIO: "rejected by the ratio test",
              PX_MATCHED: "matched", PX_OVERWRITTEN: "matched, then overwritten", PX_ROTATION: "removed by the rotation check"}
FORMS = ("points", "frame", "keyframe")
GEOMETRIES = ((640, 480), (641, 479))     # cells of 10 x 10 pixels, and cells whose sizes are no round numbers
N_LEVELS, ORB_DIST = 8, 64
SCALE_FACTORS = np.array([np.float32(1.2) ** i for i in range(N_LEVELS)], np.float32)
BASE = np.random.default_rng(20).integers(0, 256, 32, dtype=np.uint8)
_f32 = np.float32
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "refactored_orb_slam2_amd", "csrc")


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """RC_THREADS, RC_REG, RC_LIST_CAP, ORBFE_CAND_LANES (projection_kernels.hip) and ORBFE_MAX_CAND (matcher.cpp), from their #define lines:
    the census follows the kernel when one of them moves, and fails when one is no longer found"""
    out = {}
    for fn, names in (("projection_kernels.hip", ("RC_THREADS", "RC_REG", "RC_LIST_CAP", "ORBFE_CAND_LANES")), ("matcher.cpp", ("ORBFE_MAX_CAND",))):
        with open(os.path.join(_CSRC, fn)) as f:
            text = f.read()
        for name in names:
            m = re.search(r"^\s*#define\s+" + name + r"\s+(\d+)\b", text, re.M)
            assert m, f"#define {name} not found in {fn}"
            out[name] = int(m.group(1))
    return out


def bits(flips, top=False):
    """a descriptor mask: an int n turns bits 0 .. n - 1 (top: 255 .. 256 - n), an iterable turns the bits it names"""
    m = np.zeros(32, np.uint8)
    for b in (range(255, 255 - flips, -1) if top else range(flips)) if isinstance(flips, int) else flips:
        m[b >> 3] ^= np.uint8(1 << (b & 7))
    return m


class Scene:
    """hand-placed keypoints and queries of one call; `expect[i]` is the exit query i was placed for, `on[i]` the keypoint it ends on"""

    def __init__(self, name, form, w, h, nnratio=0.8, check_ori=True):
        self.name, self.form, self.w, self.h = name, form, w, h
        self.mode = 0 if form == "points" else 1
        self.nnratio = float(_f32(nnratio)) if form == "points" else 0.0
        self.check_ori = bool(check_ori) and form != "points"
        self.th_high = ORB_DIST if form == "keyframe" else TH_HIGH
        self.stereo_gate = form != "keyframe"
        self._k, self._d, self._ur, self._b0, self._unrelated, self._q = [], [], [], [], [], []
        self.expect, self.on, self.tags = [], {}, {}
        self._site = 0
        self._fill = 0

    def pick(self, default, **by_form):
        return by_form.get(self.form, default)

    def site(self):
        """the next free site: lattice of 40 pixels, x 40 .. 600, y 100 .. 420"""
        k = self._site
        self._site += 1
        assert k < 15 * 9, self.name
        return 40.0 * (1 + k % 15), 100.0 + 40.0 * (k // 15)

    def kp(self, x, y, octave=1, flips=0, angle=0.0, ur=-1.0, blocked=0, unrelated=None):
        if unrelated is not None:
            d = ~BASE ^ bits([128 + 9 * j for j in range(unrelated)])
            self._unrelated.append(len(self._k))
        else:
            d = BASE ^ bits(flips)
        self._k.append((_f32(x), _f32(y), _f32(31.0) * SCALE_FACTORS[octave], _f32(angle), _f32(1), octave, -1))
        self._d.append(d); self._ur.append(_f32(ur)); self._b0.append(blocked)
        return len(self._k) - 1

    def query(self, u, v, r, expect, qflips=0, lo=-1, hi=-1, blocks=1, valid=1, u_r=0.0, angle=0.0, on=None, tag=None):
        q = np.zeros(1, QUERY_DTYPE)[0]
        q["u"], q["v"], q["u_r"], q["radius"], q["min_level"], q["max_level"] = u, v, u_r, r, lo, hi
        q["valid"], q["blocks"], q["angle"] = valid, 1 if self.form == "keyframe" else blocks, angle
        q["desc"] = BASE ^ bits(qflips, top=True)
        self._q.append(q); self.expect.append(expect)
        i = len(self._q) - 1
        if on is not None:
            self.on[i] = on
        if tag:
            self.tags.setdefault(tag, []).append(i)
        return i

    def filler(self):
        """a query that meets nothing: invalid, outside the grid, or over an empty corner, in turn"""
        k = self._fill
        self._fill += 1
        if k % 3 == 0:
            return self.query(320.0, 240.0, 9.0, PX_SKIPPED, valid=0, lo=0, hi=7)
        if k % 3 == 1:
            return self.query((-500.0, self.w + 500.0)[k % 2], 240.0, 9.0, PX_OUTSIDE_GRID)
        return self.query(600.0, 465.0, 2.0, PX_EMPTY_WINDOW)

    def finish(self):
        self.keys = np.array(self._k, KP_DTYPE) if self._k else np.zeros(0, KP_DTYPE)
        self.desc = np.array(self._d, np.uint8).reshape(-1, 32)
        self.u_right = np.array(self._ur, np.float32)
        self.has_u_right = bool((self.u_right != -1).any())
        self.blocked0 = np.array(self._b0, np.uint8)
        self.queries = np.array(self._q, QUERY_DTYPE) if self._q else np.zeros(0, QUERY_DTYPE)
        if self._unrelated:     # >= 129 bits from everything placed
            placed = np.concatenate([np.delete(self.desc, self._unrelated, 0), self.queries["desc"]])
            far = nr._POPCOUNT[self.desc[self._unrelated][:, None, :] ^ placed[None, :, :]].sum(-1)
            assert far.min() >= 129, (self.name, far.min())
        self.result = self.walk()
        nm, assigned, blocked, exits, facts = self.result
        for i, want in enumerate(self.expect):
            assert exits[i] == want, (self.name, self.form, (self.w, self.h), i, EXIT_NAMES[want], EXIT_NAMES[int(exits[i])])
        for i, k in self.on.items():
            assert facts["best_idx"][i] == k, (self.name, self.form, i, k, facts["best_idx"][i])
        return self

    def ref_frame(self):
        return nr.RefFrame(self.keys, self.desc, 0, self.w, 0, self.h, self.u_right if self.has_u_right else None)

    def walk(self, queries=None, rules=None, check_ori=None):
        """(n_matches, assigned, blocked, exits, facts) of the walk, as arrays"""
        q = self.queries if queries is None else queries
        nm, assigned, blocked, exits, facts = nr.proj_walk(
            self.ref_frame(), q, self.mode, self.nnratio, self.check_ori if check_ori is None else check_ori, self.blocked0,
            th_high=self.th_high, stereo_gate=self.stereo_gate, rules=rules)
        return nm, np.array(assigned, np.int32).reshape(-1), np.array(blocked, np.uint8).reshape(-1), exits, facts


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
def _chain(sc):
    """Query j of a chain sees K(j - 1) at distance 10 and K(j) at distance 20; every match blocks, so query j ends on K(j) after
    K(j - 1) went to query j - 1: a dependency chain as long as the chain.  Chain A: 205 links at queries 0, 5, .. 1020 (across every
    wave of the first chunk).  Chain B: 60 links at queries 902, 907, .. with links at 1022 and 1027, on both sides of the chunk
    boundary; every 7th link does not block, the next one takes the same keypoint (the last taker wins) and the keypoint after it is
    taken before the call, so that the chain starts again."""
    S = list(range(10))
    kA = [sc.kp(15 + 2.5 * j, 30.0, 1, range(20) if j % 2 == 0 else range(10, 20)) for j in range(205)]
    breaks = sc.form != "keyframe"
    kB = [sc.kp(15 + 2.5 * j, 60.0, 1, range(20) if j % 2 == 0 else range(10, 20), blocked=int(breaks and j % 7 == 0 and j > 0)) for j in range(60)]

    def link(ks, j, y, blocks, expect, on):
        q = sc.query(15 + 2.5 * j - 1.25, y, 2.0, expect, lo=0, hi=1, blocks=blocks, on=ks[on])
        sc._q[q]["desc"] = BASE ^ bits(S if j % 2 else [])
        return q

    for i in range(1200):
        if i % 5 == 0 and i <= 1020:
            link(kA, i // 5, 30.0, 1, PX_MATCHED, i // 5)
        elif i % 5 == 2 and 902 <= i <= 1197:
            j = (i - 902) // 5
            if breaks and j % 7 == 6:
                link(kB, j, 60.0, 0, PX_OVERWRITTEN, j)
            elif breaks and j % 7 == 0 and j > 0:
                link(kB, j, 60.0, 1, PX_MATCHED, j - 1)
            else:
                link(kB, j, 60.0, 1, PX_MATCHED, j)
        else:
            sc.filler()


def _withdrawn(sc):
    """mode 0.  b's first choice is Y (30) with second-best Z (31) and W (32) behind it; an earlier query a of depth 1 ends on Z, which
    changes b's second-best and with it the ratio test: b gives up a keypoint it claimed (case 1), or claims one it had left to the later
    query c (case 2)."""
    for case in (1, 2):
        cx, cy = sc.site()
        lz, lw = (2, 1) if case == 1 else (1, 2)
        P = sc.kp(cx - 8, cy, 1, 5); Z = sc.kp(cx - 4, cy, lz, 20); Y = sc.kp(cx, cy, 1, 19); W = sc.kp(cx, cy + 2.5, lw, 21)
        V = sc.kp(cx + 6, cy - 1.5, 1, 50)
        sc.query(cx - 10, cy, 3.0, PX_MATCHED, lo=1, hi=2, on=P)
        sc.query(cx - 6, cy, 3.0, PX_MATCHED, lo=1, hi=2, on=Z)
        if case == 1:      # accepted at first (Z is of another level), rejected once W is the second-best: c ends on Y
            sc.query(cx - 1, cy, 3.5, PX_RATIO, qflips=11, lo=1, hi=2, on=Y, tag="withdrawn")
            sc.query(cx + 3, cy - 1.5, 3.5, PX_MATCHED, lo=1, hi=2, on=Y)
        else:              # rejected at first (Z is of Y's level), accepted once W is the second-best: c leaves Y for V
            sc.query(cx - 1, cy, 3.5, PX_MATCHED, qflips=11, lo=1, hi=2, on=Y, tag="mirror")
            sc.query(cx + 3, cy - 1.5, 3.5, PX_MATCHED, lo=1, hi=2, on=V)


def _ties(sc):
    """equal best distances: the first one in GetFeaturesInArea's order wins (grid column, then grid row, then index)"""
    for dx, dy in ((6, 0), (0, 6)):                     # two cells; the later index is enumerated first
        cx, cy = sc.site()
        sc.kp(cx + dx, cy + dy, 1, 30)
        ka = sc.kp(cx - dx, cy - dy, 0, 30)
        sc.query(cx, cy, 8.0, PX_MATCHED, lo=0, hi=1, on=ka, tag="tie_cells")
    cx, cy = sc.site()                                  # one cell: the lower index
    k1 = sc.kp(cx + 1, cy, 0, 30); sc.kp(cx - 1, cy, 1, 30)
    sc.query(cx, cy, 8.0, PX_MATCHED, lo=0, hi=1, on=k1, tag="tie_cell")
    for first in (1, 2):                                # the second-best distance tied between two levels: the first one gives bestLevel2
        cx, cy = sc.site()
        y = sc.kp(cx, cy, 1, 40)
        sc.kp(cx + 1, cy, first, 45); sc.kp(cx - 1, cy, 3 - first, 45)
        sc.query(cx, cy, 8.0, sc.pick(PX_MATCHED, points=PX_RATIO if first == 1 else PX_MATCHED), lo=1, hi=2, on=y, tag="second_tie")


def _thresholds(sc):
    th = sc.th_high
    for d, ex in ((th - 1, PX_MATCHED), (th, PX_MATCHED), (th + 1, PX_TOO_FAR), (th + 2, PX_TOO_FAR), (th + 20, PX_TOO_FAR), (127, PX_TOO_FAR)):
        cx, cy = sc.site()
        sc.kp(cx, cy, 1, d)
        sc.query(cx, cy, 3.0, ex, lo=0, hi=1)
    for n in range(1, 5):       # every keypoint of the window taken before the call
        cx, cy = sc.site()
        for j in range(n):
            sc.kp(cx - 1 + 0.5 * j, cy, 1, 10 + j, blocked=1)
        sc.query(cx, cy, 3.0, PX_ALL_GONE, lo=0, hi=1)
    if sc.form == "points":     # the "cannot matter" cut of the resolver at nnratio 0.8: 0.8f * 124 < 100, 0.8f * 125 is not
        for best, second, ex in ((100, 124, PX_RATIO), (100, 125, PX_MATCHED), (95, 110, PX_RATIO)):
            cx, cy = sc.site()
            kb = sc.kp(cx + 1, cy, 1, best); sc.kp(cx - 1, cy, 1, second)
            sc.query(cx, cy, 3.0, ex, lo=0, hi=1, on=kb)


def _ratio05(sc):
    """mode 0 at nnratio 0.5: bestDist > 0.5 * bestDist2 at equality"""
    for best, second, lvl2, ex in ((40, 80, 1, PX_MATCHED), (41, 80, 1, PX_RATIO), (41, 80, 2, PX_MATCHED)):
        cx, cy = sc.site()
        kb = sc.kp(cx + 1, cy, 1, best); sc.kp(cx - 1, cy, lvl2, second)
        sc.query(cx, cy, 3.0, ex, lo=1, hi=2, on=kb)


def _windows(sc):
    w, h = sc.w, sc.h
    gated = sc.pick(PX_ALL_GONE, keyframe=PX_MATCHED)
    below = lambda v: np.nextafter(_f32(v), _f32(-np.inf))
    above = lambda v: np.nextafter(_f32(v), _f32(np.inf))
    # the box |dx| < r, |dy| < r: a keypoint exactly r away is out, the next float towards the centre is in
    for ax, sign, inside in ((0, 1, False), (0, 1, True), (1, 1, False), (1, 1, True), (0, -1, False), (1, -1, True)):
        cx, cy = sc.site()
        c = [_f32(cx), _f32(cy)]
        edge = c[ax] + _f32(3.0 * sign)
        c[ax] = (below(edge) if sign > 0 else above(edge)) if inside else edge
        sc.kp(c[0], c[1], 1, 10)
        sc.query(cx, cy, 3.0, PX_MATCHED if inside else PX_EMPTY_WINDOW, tag="box")
    # the stereo gate |u_r - mvuRight| <= r, only for mvuRight > 0
    for ur, qur, ex in ((50.0, 53.0, PX_MATCHED), (50.0, above(53.0), gated), (50.0, 47.0, PX_MATCHED), (50.0, below(47.0), gated),
                        (0.0, 1000.0, PX_MATCHED), (-1.0, 1000.0, PX_MATCHED), (1e-30, 1000.0, gated)):
        cx, cy = sc.site()
        sc.kp(cx, cy, 1, 10, ur=ur)
        sc.query(cx, cy, 3.0, ex, u_r=qur, tag="gate")
    # level filters on keypoints of octave 0 .. 5, distance 10 + octave
    for lo, hi, want in ((0, -1, 0), (-1, 0, 0), (3, -1, 3), (2, 2, 2), (5, 3, None)):
        cx, cy = sc.site()
        ks = [sc.kp(cx + 0.5 * o - 1.5, cy, o, 10 + o) for o in range(6)]
        sc.query(cx, cy, 3.0, PX_EMPTY_WINDOW if want is None else PX_MATCHED, lo=lo, hi=hi, on=None if want is None else ks[want], tag="levels")
    # windows the grid clips, and windows wholly outside it
    for kx, ky, qx, qy, r in ((3.0, 200.0, 2.0, 200.0, 5.0), (w - 8.0, 200.0, w - 4.0, 200.0, 6.0), (300.0, 3.0, 300.0, 1.0, 5.0),
                              (300.0, h - 7.0, 300.0, h - 2.0, 6.0)):
        k = sc.kp(kx, ky, 1, 10)
        sc.query(qx, qy, r, PX_MATCHED, on=k, tag="clipped")
    for qx, qy in ((-50.0, 200.0), (w + 60.0, 200.0), (300.0, -50.0), (300.0, h + 60.0)):
        sc.query(qx, qy, 5.0, PX_OUTSIDE_GRID, tag="outside")
    # keypoints without a cell: PosInGrid rounds x = w - 2 to column 64, and one beyond the bounds
    sc.kp(w - 2.0, 240.0, 1, 10); sc.kp(w + 10.0, 100.0, 1, 10)
    sc.query(w - 4.0, 240.0, 6.0, PX_EMPTY_WINDOW, tag="no_cell")
    sc.query(w - 1.0, 100.0, 15.0, PX_EMPTY_WINDOW, tag="no_cell")
    # 17 grid columns (one more than a batch of the candidates kernel), and all 64
    sc.kp(250.0, 60.0, 6, 30); k17 = sc.kp(390.0, 60.0, 6, 20)
    sc.query(320.0, 60.0, 75.0, PX_MATCHED, lo=6, hi=6, on=k17, tag="cols17")
    sc.kp(15.0, 450.0, 7, 50); k64 = sc.kp(320.0, 450.0, 7, 30); sc.kp(600.0, 450.0, 7, 45)
    sc.query(320.0, 240.0, 5000.0, PX_MATCHED, lo=7, hi=7, on=k64, tag="cols64")


def _pile(sc, cx, cy, n, flips, octave):
    """n keypoints in one cell: an 8 x 8 block at half-pixel steps and a 65th four pixels to the right"""
    return [sc.kp(cx - 2 + 0.5 * (j % 8), cy - 2 + 0.5 * (j // 8), octave(j), flips(j)) if j < 64 else sc.kp(cx + 4, cy, octave(j), flips(j))
            for j in range(n)]


def _listlen(sc):
    """the lengths at which the resolver changes its path: 4 / 5 kept candidates (registers / LDS), 64 / 65 in the window (stored list /
    re-enumeration by wave 0), with the truncated query first in its chunk, in the middle, last, and twice in a row"""
    px, py = sc.site()
    pile = _pile(sc, px, py, 65, lambda j: 10 + j, lambda j: j % 2)
    small = []
    cx, cy = sc.site()        # 5 kept: one staged, and it is the best
    ks = [sc.kp(cx - 1 + 0.5 * j, cy, 1, 60 - 10 * j) for j in range(5)]
    small.append(lambda: sc.query(cx, cy, 3.0, PX_MATCHED, lo=0, hi=1, on=ks[4], tag="kept5"))
    cx4, cy4 = sc.site()      # 4 kept
    k4 = [sc.kp(cx4 - 1 + 0.5 * j, cy4, 1, 50 - 10 * j) for j in range(4)]
    small.append(lambda: sc.query(cx4, cy4, 3.0, PX_MATCHED, lo=0, hi=1, on=k4[3], tag="kept4"))
    cx6, cy6 = sc.site()      # a raw window of 6, the two best taken before the call: LDS reserved, nothing staged
    k6 = [sc.kp(cx6 - 1 + 0.4 * j, cy6, 1, f, blocked=int(f < 10)) for j, f in enumerate((5, 6, 50, 40, 30, 20))]
    small.append(lambda: sc.query(cx6, cy6, 3.0, PX_MATCHED, lo=0, hi=1, on=k6[5], tag="raw6"))
    cxu, cyu = sc.site()      # a raw window of 6 with two unrelated keypoints, which cannot matter
    ku = [sc.kp(cxu - 1 + 0.4 * j, cyu, 1, 50 - 10 * j) if j < 4 else sc.kp(cxu - 1 + 0.4 * j, cyu, 1, unrelated=j - 4) for j in range(6)]
    small.append(lambda: sc.query(cxu, cyu, 3.0, PX_MATCHED, lo=0, hi=1, on=ku[3], tag="raw6"))
    # two more piles, one level: the second-best decides the ratio test (mode 0) and sits in the first / second batch of 64 entries
    p2 = sc.site(); pile2 = _pile(sc, *p2, 65, lambda j: 10 if j == 3 else 12 if j == 5 else 50 + j, lambda j: 1)
    p3 = sc.site(); pile3 = _pile(sc, *p3, 65, lambda j: 10 if j == 3 else 12 if j == 64 else 50 + j, lambda j: 1)
    trunc = lambda k, tag: sc.query(px, py, 4.5, PX_MATCHED, lo=0, hi=1, on=pile[k], tag=tag)
    for i in range(1529):
        if i == 0:
            trunc(0, "trunc")
        elif i == 3:           # the pile's best left: taken by a query of the chunk before the truncated one at 500
            sc.query(px - 2 + 0.5, py - 2, 0.2, PX_MATCHED, lo=0, hi=1, on=pile[1])
        elif 10 <= i < 10 + len(small):
            small[i - 10]()
        elif i == 500:
            trunc(2, "trunc_after_chunk")
        elif i in (1524, 1525):
            trunc(i - 1524 + 3, "trunc")
        elif i == 1526:        # 64 in the window: the stored list, complete
            sc.query(px, py, 3.9, PX_MATCHED, lo=0, hi=1, on=pile[5], tag="full64")
        elif i == 1527:
            sc.query(*p2, 4.5, sc.pick(PX_MATCHED, points=PX_RATIO), lo=0, hi=1, on=pile2[3], tag="second_same_batch")
        elif i == 1528:
            sc.query(*p3, 4.5, sc.pick(PX_MATCHED, points=PX_RATIO), lo=0, hi=1, on=pile3[3], tag="second_later_batch")
        else:
            sc.filler()


def _staging(sc):
    """300 queries on one pile of 64: 60 staged entries each, more than RC_LIST_CAP in one run of RC_THREADS queries, so the chunk ends
    early.  Every query takes the best keypoint still free; two of three block."""
    cx, cy = sc.site()
    pile = _pile(sc, cx, cy, 64, lambda j: 10 + j, lambda j: j % 2)
    free = 0
    pending = None
    for k in range(300):
        blocks = 1 if sc.form == "keyframe" else int(k % 3 != 0)
        if free >= 64:
            ex, on = PX_ALL_GONE, None
        elif 10 + free > sc.th_high:
            ex, on = PX_TOO_FAR, pile[free]
        else:
            ex, on = PX_MATCHED, pile[free]
        q = sc.query(cx, cy, 3.0, ex, lo=0, hi=1, blocks=blocks, on=on)
        if pending is not None and ex == PX_MATCHED:
            sc.expect[pending] = PX_OVERWRITTEN
        pending = q if (ex == PX_MATCHED and not blocks) else None
        if ex == PX_MATCHED and blocks:
            free += 1


def _rotation(sc, counts, kept, pairs=False):
    """one keypoint and one query per histogram entry.  counts: {bin: entries}; kept: the bins ComputeThreeMaxima leaves.  The entry of
    bin 1 has rot == 15.0 exactly, bin 12 has 345.0 and 359, bin 11 a negative difference.  pairs (mode 1): a keypoint taken by two
    queries that do not block, one of a kept bin and one of a removed bin, in both orders."""
    def angles(b, n):
        if b == 1 and n == 0:
            return 55.0, 40.0                    # rot == 15.0: 0.5 after the factor, rounds away from zero
        if b == 12:
            return (25.0, 40.0) if n == 0 else (39.0, 40.0)    # -15 + 360 = 345, -1 + 360 = 359
        if b == 11:
            return 10.0, 40.0                    # -30 + 360
        return 40.0 + 30.0 * b + (3.0 if n % 2 else 0.0), 40.0
    ex = lambda b: PX_MATCHED if (b in kept or not sc.check_ori) else PX_ROTATION
    if pairs:
        counts = {**counts, 0: counts[0] - 2}      # the pairs bring two entries of bin 0
    for b in sorted(counts):
        for n in range(counts[b]):
            cx, cy = sc.site()
            aq, ak = angles(b, n)
            k = sc.kp(cx, cy, 1, 10, angle=ak)
            sc.query(cx, cy, 3.0, ex(b), angle=aq, on=k, tag=f"bin{b}")
    if pairs:
        for first, last in ((0, 5), (6, 0)):
            cx, cy = sc.site()
            k = sc.kp(cx, cy, 1, 10, angle=40.0)
            e1 = PX_OVERWRITTEN if (first in kept or not sc.check_ori) else PX_ROTATION
            sc.query(cx, cy, 3.0, e1, blocks=0, angle=40.0 + 30.0 * first, on=k, tag="pair")
            sc.query(cx, cy, 3.0, ex(last), blocks=0, angle=40.0 + 30.0 * last, on=k, tag="pair")


ROTATION_SCENES = {
    # name: (counts, kept bins, pairs)
    "rot_10_1": ({0: 10, 1: 1}, {0, 1}, False),                   # max2 = 1 is not < 0.1f * 10: kept
    "rot_11_1": ({0: 11, 1: 1}, {0}, True),                       # 1 < 0.1f * 11: dropped.  With the pairs {0: 11, 1: 1, 5: 1, 6: 1}
    "rot_10_5_1": ({**{0: 10, 1: 5, 12: 2}, **{b: 1 for b in range(2, 12)}}, {0, 1, 12}, False),   # every bin that can be hit
    "rot_third_kept": ({0: 10, 1: 5, 2: 1}, {0, 1, 2}, False),   # max3 = 1 is not < 0.1f * 10
    "rot_third_dropped": ({0: 11, 1: 5, 2: 1}, {0, 1}, False),
    "rot_equal": ({3: 4, 7: 4, 9: 4, 11: 4}, {3, 7, 9}, False),  # equal maxima: the first three
}


def _counts(sc, nq):
    """nq queries with the real ones spread over them -- the last one, and those on both sides of a chunk boundary, among them --
    between invalid ones and misses.  Each real query has a keypoint at distance 10 and one at 20; on every other site the nearer one
    is taken before the call."""
    for i in range(nq):
        if i % 20 == 0 or i in (nq - 1, 1022, 1023, 1024):
            cx, cy = sc.site()
            taken = sc._site % 2
            ka = sc.kp(cx - 1, cy, 1, 10, blocked=taken); kb = sc.kp(cx + 1, cy, 1, 20)
            sc.query(cx, cy, 3.0, PX_MATCHED, lo=0, hi=1, on=kb if taken else ka, tag="real")
        else:
            sc.filler()


COUNTS = (1, 1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def build_scenes(form, w=640, h=480):
    """the directed scenes of one form ("points": mode 0, "frame": mode 1, "keyframe": mode 1 without the stereo gate, with ORBdist 64
    for TH_HIGH and every match blocking) on bounds 0 .. w x 0 .. h, each walked and checked against the exits it was built for"""
    scenes = []

    def add(name, fn, *args, **kw):
        sc = Scene(name, form, w, h, **kw)
        fn(sc, *args)
        scenes.append(sc.finish())

    add("chain", _chain)
    if form == "points":
        add("withdrawn", _withdrawn)
        add("ratio05", _ratio05, nnratio=0.5)
    add("ties", _ties)
    add("thresholds", _thresholds)
    add("windows", _windows)
    add("listlen", _listlen)
    add("staging", _staging)
    if form != "points":
        for name, (counts, kept, pairs) in ROTATION_SCENES.items():
            add(name, _rotation, counts, kept, pairs and form == "frame")
        add("rot_11_1_off", _rotation, *ROTATION_SCENES["rot_11_1"][:2], form == "frame", check_ori=False)
    for nq in COUNTS:
        add(f"counts_{nq}", _counts, nq)
    return tuple(scenes)


# ---- the census ----------------------------------------------------------------------------------------------------------------
REACHABLE = {"points": (PX_SKIPPED, PX_OUTSIDE_GRID, PX_EMPTY_WINDOW, PX_ALL_GONE, PX_TOO_FAR, PX_RATIO, PX_MATCHED, PX_OVERWRITTEN),
             "frame": (PX_SKIPPED, PX_OUTSIDE_GRID, PX_EMPTY_WINDOW, PX_ALL_GONE, PX_TOO_FAR, PX_MATCHED, PX_OVERWRITTEN, PX_ROTATION),
             # every match of the keyframe form blocks, so no keypoint is taken twice
             "keyframe": (PX_SKIPPED, PX_OUTSIDE_GRID, PX_EMPTY_WINDOW, PX_ALL_GONE, PX_TOO_FAR, PX_MATCHED, PX_ROTATION)}


def chunks(n_window, C=None):
    """How proj_resolve_kernel cuts a call into chunks, from the window counts alone (n_window is 0 for an invalid query): a chunk
    takes up to RC_THREADS queries and ends before the first list longer than ORBFE_MAX_CAND and before the staged entries
    (n_window - RC_REG each) pass RC_LIST_CAP; a truncated query at the head of a chunk is handled alone.
    Returns [(first query, length, staged entries)], length 0 for a truncated query."""
    C = C or kernel_constants()
    out, q0, nq = [], 0, len(n_window)
    while q0 < nq:
        tot = np.asarray(n_window[q0:q0 + C["RC_THREADS"]], np.int64)
        staged = np.cumsum(np.where(tot > C["ORBFE_MAX_CAND"], 0, np.maximum(tot - C["RC_REG"], 0)))
        cut = np.nonzero((tot > C["ORBFE_MAX_CAND"]) | (staged > C["RC_LIST_CAP"]))[0]
        ln = int(cut[0]) if len(cut) else len(tot)
        out.append((q0, ln, int(staged[ln - 1]) if ln else 0))
        q0 += max(ln, 1)
    return out


def truncated_positions(n_window, C=None):
    """where each truncated query stood in the chunk that met it: 'first', 'middle', 'last', and 'twice' behind another truncated one"""
    C = C or kernel_constants()
    pos, prev = set(), None
    for q0, ln, _ in chunks(n_window, C):
        if ln == 0:     # what stood before it: nothing or a full chunk, another truncated query, or the chunk it cut short
            pos.add("first" if prev is None or prev == C["RC_THREADS"] else "twice" if prev == 0 else
                    "last" if prev == C["RC_THREADS"] - 1 else "middle")
        prev = ln
    return pos


def staged_per_run(n_window, C=None):
    """the largest sum of max(n_window - RC_REG, 0) over RC_THREADS consecutive queries"""
    C = C or kernel_constants()
    v = np.maximum(np.asarray(n_window, np.int64) - C["RC_REG"], 0)
    c = np.concatenate([[0], np.cumsum(v)])
    return int(max(c[min(i + C["RC_THREADS"], len(v))] - c[i] for i in range(max(len(v), 1)))) if len(v) else 0


def census(scenes):
    """scenes: the scenes of one form and geometry, walked.  Returns the list of census conditions that do NOT hold."""
    C = kernel_constants()
    T, REG, CAP, MAXC, LANES = C["RC_THREADS"], C["RC_REG"], C["RC_LIST_CAP"], C["ORBFE_MAX_CAND"], C["ORBFE_CAND_LANES"]
    form = scenes[0].form
    missing = []
    res = [(sc,) + sc.result[3:] for sc in scenes]
    allx = np.concatenate([e for _, e, _ in res])
    cat = lambda k: np.concatenate([f[k] for _, _, f in res])
    for x in REACHABLE[form]:
        if (allx == x).sum() < 4:
            missing.append(f"fewer than 4 queries take the exit '{EXIT_NAMES[x]}'")
    for x in set(EXIT_NAMES) - set(REACHABLE[form]):
        if (allx == x).any():
            missing.append(f"a query takes the exit '{EXIT_NAMES[x]}', which the {form} form cannot reach")
    if cat("depth").max() < 200:
        missing.append("no dependency chain of depth 200")
    if not any(((np.arange(len(e)) >= T) & (f["dep_min"] >= 0) & (f["dep_min"] < T)).any() and chunks(f["n_window"], C)[0][1] == T
               for _, e, f in res):
        missing.append(f"no dependency from a query below {T} to one from {T} on, in a call whose first chunk is full")
    if cat("best_tie_out_of_index_order").sum() < 1:
        missing.append("no tie at the best distance that index order would decide otherwise")
    if not ((cat("best_ties") > 0) & ~cat("best_tie_out_of_index_order")).any():
        missing.append("no tie at the best distance that the lower index wins")
    th = scenes[0].th_high
    for d, x in ((th - 1, PX_MATCHED), (th, PX_MATCHED), (th + 1, PX_TOO_FAR)):
        if not ((cat("best_dist") == d) & (allx == x)).any():
            missing.append(f"no best distance {d} at th_high {th}")
    if form == "points":
        for sc, e, f in res:
            later = lambda i, k: any(f["best_idx"][j] == k and e[j] == PX_MATCHED for j in range(i + 1, len(e)))
            wd = [i for i in range(len(e)) if e[i] == PX_RATIO and f["first_accept"][i] and later(i, f["first_choice"][i])]
            mr = [i for i in range(len(e)) if e[i] == PX_MATCHED and not f["first_accept"][i] and f["n_blocked_by_call"][i] > 0 and
                  any(f["first_choice"][j] == f["best_idx"][i] and f["best_idx"][j] != f["best_idx"][i] for j in range(i + 1, len(e)))]
            if sc.name == "withdrawn" and (not wd or not mr):
                missing.append("a withdrawn claim or its mirror case is missing")
        if not any(sc.name == "withdrawn" for sc in scenes):
            missing.append("no withdrawn-claim scene")
        if cat("second_level_tied").sum() < 1:
            missing.append("no second-best distance tied between two levels")
        have = {(round(sc.nnratio, 3), int(b), int(s), int(x)) for sc, e, f in res for b, s, x in zip(f["best_dist"], f["second_dist"], e)}
        for want in ((0.5, 40, 80, PX_MATCHED), (0.5, 41, 80, PX_RATIO), (0.8, 100, 124, PX_RATIO), (0.8, 100, 125, PX_MATCHED),
                     (0.8, 95, 110, PX_RATIO)):
            if want not in have:
                missing.append(f"the ratio case {want} is missing")
        lv = [(sc, i) for sc, e, f in res for i in range(len(e)) if round(sc.nnratio, 3) == 0.5 and f["best_dist"][i] == 41 and
              f["second_dist"][i] == 80 and e[i] == PX_MATCHED]
        if not lv:
            missing.append("41 against 80 on different levels is missing")
        batch = [(int(f["best_pos"][i]) // MAXC, int(f["second_pos"][i]) // MAXC) for _, e, f in res for i in range(len(e))
                 if f["n_window"][i] > MAXC and e[i] == PX_RATIO]
        if (0, 0) not in batch or (0, 1) not in batch:
            missing.append("no truncated query whose second-best (same batch / later batch) decides the ratio test")
    for k in (REG, REG + 1):
        if not (cat("matters_kept") == k).any():
            missing.append(f"matters_kept == {k} does not occur")
    if not ((cat("n_window") == REG + 2) & (cat("matters_kept") == REG) & (cat("n_blocked_before") == 2)).any():
        missing.append("no raw window that reserves staging and stages nothing")
    for k in (MAXC, MAXC + 1):
        if not (cat("n_window") == k).any():
            missing.append(f"n_window == {k} does not occur")
    pos = set().union(*[truncated_positions(f["n_window"], C) for _, _, f in res])
    if pos != {"first", "middle", "last", "twice"}:
        missing.append(f"truncated queries stand only {sorted(pos)} in their chunks")
    if not any((f["n_window"] > MAXC)[i] and f["n_blocked_by_call"][i] > 0 for _, e, f in res for i in range(len(e))):
        missing.append("no truncated query whose best went to an earlier query of the call")
    if not any(staged_per_run(f["n_window"], C) > CAP and f["n_window"].max() <= MAXC and
               any(0 < ln < min(T, len(f["n_window"]) - q0) for q0, ln, _ in chunks(f["n_window"], C)) for _, _, f in res):
        missing.append(f"no call whose staged lists pass {CAP} entries within {T} queries while every window holds <= {MAXC}")
    ncol = cat("ncol")
    if not (ncol == LANES + 1).any() or not (ncol == 64).any():
        missing.append(f"no window of {LANES + 1} grid columns, or none of all 64")
    for n in COUNTS:
        if not any(len(e) == n for _, e, _ in res):
            missing.append(f"no call of {n} queries")
    if form != "points":
        bins = sorted({int(b) for b in cat("rot_bin") if b >= 0})
        if bins != list(range(13)):
            missing.append(f"rotation bins hit: {bins}")      # 13 .. 29 cannot be: rot < 360 and the factor is 1 / 30
        pairs = {(sorted(f["hist"], reverse=True)[0], sorted(f["hist"], reverse=True)[1], f["maxima"][1] >= 0) for _, _, f in res}
        third = {(sorted(f["hist"], reverse=True)[0], sorted(f["hist"], reverse=True)[2], f["maxima"][2] >= 0) for _, _, f in res}
        if (10, 1, True) not in pairs or (11, 1, False) not in pairs or (10, 1, True) not in third or (11, 1, False) not in third:
            missing.append("a pair of the 0.1 rule is missing")
        if not any(sorted(f["hist"], reverse=True)[0] == sorted(f["hist"], reverse=True)[3] > 0 for _, _, f in res):
            missing.append("no histogram with four equal maxima")
        if form == "frame" and sum(f["cleared_but_won_by_kept_bin"] for _, _, f in res) < 1:
            missing.append("no keypoint cleared through an overwritten query's bin while the last taker's bin was kept")
    return missing


def exit_counts(results, th_high=TH_HIGH):
    """results: [(exits, facts)].  The rows of the table in this module's docstring."""
    C = kernel_constants()
    allx = np.concatenate([e for e, _ in results])
    cat = lambda k: np.concatenate([f[k] for _, f in results])
    out = {EXIT_NAMES[x]: int((allx == x).sum()) for x in EXIT_NAMES}
    out.update({"largest depth": int(cat("depth").max()), "largest n_window": int(cat("n_window").max()),
                "largest matters_kept": int(cat("matters_kept").max()), "queries with a tie at the best": int((cat("best_ties") > 0).sum()),
                "won against index order": int(cat("best_tie_out_of_index_order").sum()),
                "second-best tied across levels": int(cat("second_level_tied").sum()),
                "dependency across the first chunk boundary": any(((np.arange(len(e)) >= C["RC_THREADS"]) & (f["dep_min"] >= 0) &
                                                                   (f["dep_min"] < C["RC_THREADS"])).any() for e, f in results),
                "staged entries in one run": max(staged_per_run(f["n_window"], C) for _, f in results),
                "cleared, last taker's bin kept": sum(f["cleared_but_won_by_kept_bin"] for _, f in results),
                "rotation bins hit": sorted({int(b) for b in cat("rot_bin") if b >= 0}),
                "best distance th_high - 1 / th_high / th_high + 1": [int((cat("best_dist") == th_high + d).sum()) for d in (-1, 0, 1)],
                "windows of more than ORBFE_MAX_CAND": int((cat("n_window") > C["ORBFE_MAX_CAND"]).sum()),
                "matters_kept RC_REG / RC_REG + 1": [int((cat("matters_kept") == C["RC_REG"] + d).sum()) for d in (0, 1)],
                "decision changed by a match of the call": int(((cat("n_blocked_by_call") > 0) & (cat("first_choice") == cat("best_idx")) &
                                                                (cat("first_accept") != np.isin(allx, (PX_MATCHED, PX_OVERWRITTEN, PX_ROTATION)))).sum())})
    return out
