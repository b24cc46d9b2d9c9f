"""Frame::ComputeStereoMatches (L/src/Frame.cc:477-646) on DIRECTED input: the instrumented reading, a seeded builder of scenes with
hand-placed keypoints, and the census of what those scenes reach.

  stereo_exits   tests/np_restatement.stereo_walk -- the one body behind ref_compute_stereo_matches -- with its exit code per left
                 keypoint and the per-call facts the census reads
  build_scenes   one image pair per (w, h, seed) and a list of scenes on it; a scene is hand-placed (keysL, descL, keysR, descR),
                 (mbf, mb) and the exit every left keypoint was placed for
  census         the conditions tests/test_stereo_cpu.py asserts on the reading's own exit codes (never on the kernel's output)

Input domain of the stereo entry points beyond the extractor's own keypoints: finite coordinates with 0 <= x < w, 0 <= y < h, octaves
in [0, n_levels).  Rows outside the image and uL < 0 are outside it (SX_OUTSIDE below: never produced here).

The image pair: L is a smoothed random texture in 40 .. 200, R the same texture D = 7 pixels further left plus noise in -3 .. 3, so
that NATURAL pairs (right keypoint D pixels to the left at level 0, round(D / scale) level pixels at level l) match with a small
positive SAD at every level.  EXACT cases are pasted at level 0 into slots of the interior: the left 11 x 11 window copied into R
(SAD 0 at the chosen shift), then k non-centre pixels of the copy raised by d_i (SAD exactly sum d_i), a window mirror-symmetric about
its centre column (deltaR == 0, disparity exactly 0: the 0.01 clamp), horizontal stripes that R holds over 12 columns (two
neighbouring shifts tie at SAD 0: deltaR == 0.5 exactly, or the end-shift exit when the tie is at shifts -5 / -4).  Partners carry
the same random descriptor (distance 0), unrelated keypoints random ones (about 128 bits apart, never below TH_HIGH = 100).

What the extractor's own keypoints reach and what the directed scenes reach, left keypoints per exit:

  exit                                        test_stereo_matches_one_pair_host_api[752x480]    build_scenes(416, 200, 0)
  row list empty                                      1                                           10
  no candidate passes the octave / disparity gates   96                                           6
  best Hamming distance >= 75                        216                                           5
  left 11 x 11 window leaves its level                 0                                           14
  iniu < 0 || endu >= cols                             0                                           4
  right 11 x 21 window leaves its level                0                                           4
  SAD minimum at shift -5 / +5                        19                                           4
  deltaR outside [-1, 1]                               0                                           0 (unreachable, see census)
  disparity outside [0, maxD)                          0                                           8
  matched with disparity <= 0, clamped to 0.01         0                                           4
  matched                                            755                                           87
  removed by the median rule                         117                                           5
  longest candidate run                               25                                           150
"""
from __future__ import annotations

import functools

import numpy as np

from tests import np_restatement as nr
from tests.np_restatement import (SX_OUTSIDE, SX_ROW_EMPTY, SX_NO_CANDIDATE, SX_HAMMING, SX_LEFT_WINDOW, SX_RIGHT_SPAN,  # noqa: F401
                                  SX_RIGHT_WINDOW, SX_END_SHIFT, SX_DELTA, SX_DISPARITY, SX_CLAMPED, SX_MATCHED, SX_MEDIAN)

EXIT_NAMES = {SX_ROW_EMPTY: "row list empty", SX_NO_CANDIDATE: "no candidate passes the gates", SX_HAMMING: "best Hamming distance >= 75",
              SX_LEFT_WINDOW: "left window leaves its level", SX_RIGHT_SPAN: "iniu < 0 || endu >= cols",
              SX_RIGHT_WINDOW: "right window leaves its level", SX_END_SHIFT: "SAD minimum at an end shift",
              SX_DISPARITY: "disparity outside [0, maxD)", SX_CLAMPED: "matched, clamped to 0.01", SX_MATCHED: "matched",
              SX_MEDIAN: "removed by the median rule"}
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
GEOMETRIES = ((416, 200), (421, 203))   # n_buckets * n_levels = 200 < 256 and a level 7 of 116 x 56; a width that is no multiple of 16
N_LEVELS, SCALE = 8, 1.2
D = 7                                   # disparity of the natural content, level-0 pixels
KITTI = (np.float32(386.1448), np.float32(386.1448 / 718.856))   # maxD = 718.9
WIDE = (np.float32(400.0), np.float32(0.5))                      # maxD = 800: every x <= uL passes
NARROW = (np.float32(30.0), np.float32(1.0))                     # maxD = 30
_f32 = np.float32


def stereo_exits(keysL, descL, keysR, descR, pyrL, pyrR, scale_factors, inv_scale_factors, mbf, mb):
    """ref_compute_stereo_matches with its bookkeeping: (mvuRight, mvDepth, exits, facts).  exits: one SX_* code per left keypoint.
    facts, per call: longest_run (entries of octave l - 1 .. l + 1 in the keypoint's row), hamming_ties / hamming_ties_dx (further
    candidates at the winning distance; those among them with another x than the winner's), sad_ties (further shifts at the SAD
    minimum), touching (keypoints whose left or right window has the level's first or last row or column as its own), clipped_top /
    clipped_bottom (right bands the image cuts), at_min_u / at_max_u (candidates with uR == minU / maxU), best_74 / best_75,
    median_in (the sorted SAD list that enters the median rule), median; `per_keypoint` holds the arrays they were summed from."""
    ur, depth, exits, f = nr.stereo_walk(keysL, descL, keysR, descR, pyrL, pyrR, scale_factors, inv_scale_factors, mbf, mb)
    facts = dict(longest_run=int(f["run"].max(initial=0)), hamming_ties=int(f["hamming_ties"].sum()),
                 hamming_ties_dx=int(f["hamming_ties_dx"].sum()), sad_ties=int(f["sad_ties"].sum()), touching=int(f["touches"].sum()),
                 clipped_top=int(f["clipped_top"].sum()), clipped_bottom=int(f["clipped_bottom"].sum()),
                 at_min_u=int(f["at_min_u"].sum()), at_max_u=int(f["at_max_u"].sum()), best_74=int((f["best_dist"] == 74).sum()),
                 best_75=int((f["best_dist"] == 75).sum()), median_in=list(f["median_in"]), median=f["median"], per_keypoint=f)
    return ur, depth, exits, facts


# ---- the builder -------------------------------------------------------------------------------------------------------------------
class Scene:
    """hand-placed keypoints on the builder's image pair; `expect[i]` is the exit left keypoint i was placed for"""

    def __init__(self, b, name, maxd):
        self.b, self.name = b, name
        self.mbf, self.mb = maxd
        self._kL, self._dL, self._kR, self._dR, self.expect, self.tags = [], [], [], [], [], {}

    def _key(self, level, cx, cy, x, y):
        sf, isf = self.b.sf[level], self.b.isf[level]
        x = _f32(cx) * sf if x is None else _f32(x)
        y = _f32(cy) * sf if y is None else _f32(y)
        # the level coordinates the walk will round to are the ones the case was built for
        assert nr.c_round(x * isf) == cx and nr.c_round(y * isf) == cy, (self.name, level, cx, cy, x, y)
        assert 0 <= x < self.b.w and 0 <= y < self.b.h, (self.name, x, y)
        return (x, y, _f32(31.0) * sf, _f32(0), _f32(1), level, -1)

    def right(self, level, cx, cy, desc, x=None, y=None):
        self._kR.append(self._key(level, cx, cy, x, y)); self._dR.append(desc)
        return len(self._kR) - 1

    def left(self, level, cx, cy, desc, expect, x=None, y=None, tag=None):
        self._kL.append(self._key(level, cx, cy, x, y)); self._dL.append(desc); self.expect.append(expect)
        if tag:
            self.tags.setdefault(tag, []).append(len(self._kL) - 1)
        return len(self._kL) - 1

    def pair(self, level, cxL, cy, cxR, expect, flips=0, right_level=None, tag=None, **kw):
        """a left keypoint and its partner on the same image row: the same descriptor with `flips` bits turned"""
        d = self.b.desc()
        rl = level if right_level is None else right_level
        yimg = _f32(cy) * self.b.sf[level]
        cyR = nr.c_round(yimg * self.b.isf[rl])
        ximg = _f32(cxR) * self.b.sf[level]
        self.right(rl, nr.c_round(ximg * self.b.isf[rl]), cyR, self.b.flip(d, flips), x=ximg, y=yimg)
        return self.left(level, cxL, cy, d, expect, tag=tag, **kw)

    def arrays(self):
        mk = lambda k: np.array(k, KP_DTYPE) if k else np.zeros(0, KP_DTYPE)
        md = lambda d: np.array(d, np.uint8).reshape(-1, 32)
        return mk(self._kL), md(self._dL), mk(self._kR), md(self._dR)


class Builder:
    def __init__(self, w, h, seed):
        self.w, self.h, self.seed = w, h, seed
        self.rng = np.random.default_rng([w, h, seed])
        sf, isf, _ = nr.extractor_tables(200, SCALE, N_LEVELS)
        self.sf, self.isf = np.array(sf, np.float32), np.array(isf, np.float32)
        self.sizes = [(int(np.rint(np.float64(_f32(w) * self.isf[l]))), int(np.rint(np.float64(_f32(h) * self.isf[l])))) for l in range(N_LEVELS)]
        t = self.rng.random((h + 2, w + D + 2))
        t = sum(t[dy:dy + h, dx:dx + w + D] for dy in range(3) for dx in range(3))
        t = np.rint(40 + 160 * (t - t.min()) / (t.max() - t.min())).astype(np.int32)
        self.L = t[:, :w].copy()                                   # R[y, x] == L[y, x + D] up to the noise
        self.R = np.clip(t[:, D:] + self.rng.integers(-3, 4, (h, w)), 0, 255).astype(np.int32)
        # slots of the interior for the exact cases: 13 rows x 32 columns, below the natural zone (margins and rows < 67 stay untouched)
        self.y_nat = 28
        xs = list(range(40, w - 40 - 31, 32)); ys = list(range(67 + 6, h - 28 - 6, 13))
        self._slots = [(x0, y) for y in ys for x0 in xs]
        self._per_row = len(xs)
        self._next = 0
        self.scenes = []

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flip(self, d, n):
        d = d.copy()
        for bit in self.rng.permutation(256)[:n]:
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return d

    def scene(self, name, maxd):
        s = Scene(self, name, maxd)
        self.scenes.append(s)
        return s

    def slot(self, wide=False):
        """centre (xL, y) of a left window whose slot nothing else writes: 32 columns (right keypoint up to 7 to the left), or 64"""
        if wide and self._next % self._per_row == self._per_row - 1:
            self._next += 1
        x0, y = self._slots[self._next]
        self._next += 2 if wide else 1
        return (x0 + 45 if wide else x0 + 21), y

    # -- the exact cases, level 0 (level coordinates are image coordinates)
    def copy(self, xL, y, xc):
        """the left window of (xL, y) into R with its centre at column xc: SAD 0 at the shift that lands on xc"""
        self.R[y - 5:y + 6, xc - 5:xc + 6] = self.L[y - 5:y + 6, xL - 5:xL + 6]

    def raise_sad(self, xc, y, s):
        """raise non-centre pixels of R's window at (xc, y) by s in all: the SAD of that shift grows by exactly s"""
        for yy in range(y - 5, y + 6):
            for xx in range(xc - 5, xc + 6):
                if s > 0 and (xx, yy) != (xc, y):
                    d = min(s, 50)
                    self.R[yy, xx] += d; s -= d
        assert s == 0 and self.R.max() <= 255

    def exact_pair(self, sc, sad, expect, d=D, wide=False, tag=None, shift=0):
        """level-0 pair in a slot of its own: right keypoint d to the left, the content `shift` columns to the right of it, SAD `sad`"""
        xL, y = self.slot(wide)
        self.copy(xL, y, xL - d + shift)
        self.raise_sad(xL - d + shift, y, sad)
        desc = self.desc()
        sc.right(0, xL - d, y, desc)
        return sc.left(0, xL, y, desc, expect, tag=tag)

    def reuse(self, sc, src, idx, expect, tag=None):
        """keypoint idx of scene src, and its partner, once more in scene sc (ballast: its SAD is in the images already)"""
        kL, dL = src._kL[idx], src._dL[idx]
        j = [k for k in range(len(src._dR)) if np.array_equal(src._dR[k], dL)][0]
        sc._kR.append(src._kR[j]); sc._dR.append(src._dR[j])
        sc._kL.append(kL); sc._dL.append(dL); sc.expect.append(expect)
        if tag:
            sc.tags.setdefault(tag, []).append(len(sc._kL) - 1)

    def images(self):
        return self.L.astype(np.uint8), self.R.astype(np.uint8)


def _edges(b, level):
    """window guards (Frame.cc:569-590 read unchecked windows; the library gives no match) at `level`, natural content"""
    sc = b.scene(f"edges_l{level}", WIDE)
    W, H = b.sizes[level]
    dl = nr.c_round(D * b.isf[level])                       # the content's disparity in level pixels
    cols = [W // 4 + 13 * i for i in range(4)]
    # left rows: y = 5 touches, 4 leaves, H - 6 touches, H - 5 leaves
    for i, (cy, ex) in enumerate(((5, SX_MATCHED), (4, SX_LEFT_WINDOW), (H - 6, SX_MATCHED), (H - 5, SX_LEFT_WINDOW))):
        for cx in (cols[i], cols[i] + W // 3):
            sc.pair(level, cx, cy, cx - dl, ex, tag="touch" if ex == SX_MATCHED else None)
    rows = [H // 4 + 9 * i for i in range(8)]
    # right x = 10 touches, 9 leaves through the right-window guard
    sc.pair(level, 10 + dl, rows[0], 10, SX_MATCHED, tag="touch")
    sc.pair(level, 10 + dl, rows[1], 10, SX_MATCHED, tag="touch")
    sc.pair(level, 9 + dl, rows[2], 9, SX_RIGHT_WINDOW)
    sc.pair(level, 9 + dl, rows[3], 9, SX_RIGHT_WINDOW)
    # left x = W - 6 touches; right x = W - 12: endu = cols - 1 is kept, W - 11: endu = cols is refused; left x = W - 5 leaves
    sc.pair(level, W - 6, rows[0], W - 12, SX_MATCHED, tag="touch")
    sc.pair(level, W - 6, rows[1], W - 12, SX_MATCHED, tag="touch")
    sc.pair(level, W - 6, rows[2], W - 11, SX_RIGHT_SPAN)
    sc.pair(level, W - 6, rows[3], W - 11, SX_RIGHT_SPAN)
    sc.pair(level, W - 5, rows[4], W - 12, SX_LEFT_WINDOW)
    sc.pair(level, W - 5, rows[5], W - 12, SX_LEFT_WINDOW)
    return sc


def _gates(b):
    """row bands (Frame.cc:493-502), octave gate (:538-539), distance threshold (:555), natural content of the rows below y_nat + 12"""
    sc = b.scene("gates", KITTI)
    w, h = b.w, b.h
    # a right keypoint of octave 0 at an integral y: the band is y - 2 .. y + 2 exactly.  Left keypoints on its first and last row
    # and one row beyond, all with its descriptor
    for k, x in enumerate((60, 130)):
        y = 46 + 10 * k
        d = b.desc()
        sc.right(0, x - D, y, d)
        sc.left(0, x, y - 2, d, SX_MATCHED, tag="band")
        sc.left(0, x, y - 2, d, SX_ROW_EMPTY, y=_f32(y - 3) + _f32(0.9))      # (int)vL is the row
        sc.left(0, x, y + 3, d, SX_MATCHED, y=_f32(y + 2) + _f32(0.9), tag="band")
        sc.left(0, x, y + 3, d, SX_ROW_EMPTY, y=_f32(y + 3))
    # the same at octave 1 with y + r integral: r = 2 * 1.2f
    r = _f32(2.0) * b.sf[1]
    y1 = _f32(_f32(40) - r)
    assert y1 + r == _f32(40)
    for x in (200, 260):
        d = b.desc()
        cxl = nr.c_round(_f32(x) * b.isf[1])
        xi = _f32(cxl) * b.sf[1]
        sc.right(1, nr.c_round((xi - _f32(D)) * b.isf[1]), nr.c_round(y1 * b.isf[1]), d, x=xi - _f32(D), y=y1)
        sc.left(1, cxl, nr.c_round(_f32(40.5) * b.isf[1]), d, SX_MATCHED, y=40.5, tag="band")    # row 40 = maxr
        sc.left(1, cxl, nr.c_round(_f32(41.0) * b.isf[1]), d, SX_ROW_EMPTY, y=41.0)
    # octave differences 0, +-1 (kept) and +-2 (gated) against a left keypoint of level 2, rows of their own
    for k, (ro, ex) in enumerate(((1, SX_MATCHED), (2, SX_MATCHED), (3, SX_MATCHED), (0, SX_NO_CANDIDATE), (4, SX_NO_CANDIDATE))):
        cy = nr.c_round(_f32(90 + 14 * k) * b.isf[2])
        cx = nr.c_round(_f32(330) * b.isf[2])
        sc.pair(2, cx, cy, cx - nr.c_round(D * b.isf[2]), ex, right_level=ro, tag="octave")
    # the partner to the right of the left keypoint: uR > maxU
    sc.pair(0, 300, 111, 303, SX_NO_CANDIDATE)
    sc.pair(0, 296, 125, 299, SX_NO_CANDIDATE)
    # the distance threshold (TH_HIGH + TH_LOW) / 2 = 75: 73, 74 bits match; 75, 76, 99, 100 do not
    for k, (flips, ex) in enumerate(((73, SX_MATCHED), (74, SX_MATCHED), (74, SX_MATCHED), (75, SX_HAMMING), (75, SX_HAMMING),
                                     (76, SX_HAMMING), (99, SX_HAMMING), (100, SX_HAMMING))):
        sc.pair(0, 30 + 8 * k, (70, 76, 82, 150, 156, 162, 168, 174)[k], 30 + 8 * k - D, ex, flips=flips, tag=f"flip{flips}")
    return sc


def _clipped(b):
    """right bands that the image cuts (Frame.cc:497-501 indexes vRowIndices unchecked; the oracle keeps the rows inside), a scene of
    its own: the SADs of level 6 would not survive the median of level-0 matches"""
    sc = b.scene("clipped", KITTI)
    h = b.h
    # octave 7 (r = 7.17) at y = 7 is cut by the top -- its partner of level 6 on row 14 still has its window --
    # and at y = h - 5 by the bottom, where every row of the band is too low for a window
    for x in (100.0, 300.0):
        d = b.desc()
        sc.right(7, nr.c_round(_f32(x - D) * b.isf[7]), nr.c_round(_f32(7.0) * b.isf[7]), d, x=x - D, y=7.0)
        sc.left(6, nr.c_round(_f32(x) * b.isf[6]), 5, d, SX_MATCHED, x=x, y=14.0, tag="clip_top")
        d = b.desc()
        sc.right(7, nr.c_round(_f32(x - D) * b.isf[7]), nr.c_round(_f32(h - 5) * b.isf[7]), d, x=x - D, y=h - 5.0)
        sc.left(6, nr.c_round(_f32(x) * b.isf[6]), nr.c_round(_f32(h - 6) * b.isf[6]), d, SX_LEFT_WINDOW, x=x, y=h - 6.0, tag="clip_bottom")
    return sc


def _long_run(b):
    """150 right keypoints on one row, 120 of octave 0 and 30 of octave 1: the candidate loop of a left keypoint of level 0 or 1 runs
    five trips.  Each left descriptor appears twice at different x; the lower index must win (strict <, Frame.cc:548-552)."""
    sc = b.scene("long_run", WIDE)
    y = b.y_nat + 5
    xs = [31 + 3 * i for i in range(120)]
    order = list(b.rng.permutation(120))
    uA, uB = 31 + 3 * 114 + D, 31 + 3 * 87 + D
    # A: both copies beyond the 64th entry, the true partner (x = uA - D) first; B: both within the first trip
    for true_i, other_i, at, at2 in ((114, 60, 70, 100), (87, 20, 5, 20)):
        for i, pos in ((true_i, at), (other_i, at2)):
            j = order.index(i)
            order[j], order[pos] = order[pos], order[j]
    dA, dB, dC = b.desc(), b.desc(), b.desc()
    for pos, i in enumerate(order):
        sc.right(0, xs[i], y, dA if pos in (70, 100) else dB if pos in (5, 20) else b.desc())
    assert order[70] == 114 and order[100] == 60 and order[5] == 87 and order[20] == 20
    cC = nr.c_round(_f32(200) * b.isf[1]); cyC = nr.c_round(_f32(y) * b.isf[1])
    dl = nr.c_round(D * b.isf[1])
    for k in range(30):
        cx = cC - dl if k == 5 else cC - 40 if k == 20 else 20 + 7 * k + (1 if 20 + 7 * k in (cC - dl, cC - 40) else 0)
        sc.right(1, cx, cyC, dC if k in (5, 20) else b.desc(), y=y)
    sc.left(0, uA, y, dA, SX_MATCHED, tag="tie")
    sc.left(0, uB, y, dB, SX_MATCHED, tag="tie")
    sc.left(1, cC, cyC, dC, SX_MATCHED, y=y, tag="tie")
    # rows without a single band
    for x in (50, 150, 250, 350):
        sc.left(0, x, y + 40, b.desc(), SX_ROW_EMPTY)
    return sc


def _disparity(b, ballast):
    """the disparity gate [0, maxD) and the 0.01 clamp (Frame.cc:617-626) with maxD = 30, exact content"""
    sc = b.scene("disparity", NARROW)
    for _ in range(4):
        # uR == uL (== maxU) with the content 2 to the right: disparity -2
        b.exact_pair(sc, 0, SX_DISPARITY, d=0, shift=2)
        # uR == uL - 29 with the content 3 further left: disparity 32 >= maxD
        b.exact_pair(sc, 0, SX_DISPARITY, d=29, shift=-3, wide=True)
        # uR == uL - 30 == minU with the content 3 to the right: disparity 27, kept
        b.exact_pair(sc, 0, SX_MATCHED, d=30, shift=3, wide=True, tag="min_u")
        # a window mirror-symmetric about its centre column at the same place in both images, uR == uL: deltaR == 0, disparity 0
        xL, y = b.slot()
        p = b.rng.integers(40, 201, (11, 11))
        p = np.concatenate([p[:, :0:-1], p], axis=1)            # 21 columns, p[:, 10 - k] == p[:, 10 + k]
        b.L[y - 5:y + 6, xL - 10:xL + 11] = p; b.R[y - 5:y + 6, xL - 10:xL + 11] = p
        d = b.desc()
        sc.right(0, xL, y, d)
        sc.left(0, xL, y, d, SX_CLAMPED, tag="clamp")
    # beyond minU: no candidate
    b.exact_pair(sc, 0, SX_NO_CANDIDATE, d=31, wide=True)
    b.exact_pair(sc, 0, SX_NO_CANDIDATE, d=31, wide=True)
    for i in ballast:
        b.reuse(sc, b.scenes[0], i, SX_MATCHED)
    return sc


def _sad_ties(b, ballast):
    """horizontal stripes that R holds over 12 columns: the 11-column windows of two neighbouring shifts lie inside them, both with
    SAD 0.  The first one is the minimum (strict <, Frame.cc:595-599): shifts 1 / 2 give deltaR = d1 / (2 d1) = 0.5 exactly, shifts
    -5 / -4 the end-shift exit (:607-608)."""
    sc = b.scene("sad_ties", KITTI)
    for k, ex in ((1, SX_MATCHED), (-5, SX_END_SHIFT)) * 4:
        xL, y = b.slot()
        g = b.rng.permutation(np.arange(40, 201, 12))[:11][:, None]
        b.L[y - 5:y + 6, xL - 5:xL + 6] = g
        uR = xL - D
        b.R[y - 5:y + 6, uR + k - 5:uR + k + 7] = g
        d = b.desc()
        sc.right(0, uR, y, d)
        sc.left(0, xL, y, d, ex, tag="sad_tie" if ex == SX_MATCHED else "sad_tie_end")
    for i in ballast:
        b.reuse(sc, b.scenes[0], i, SX_MATCHED)
    return sc


MEDIAN_POPULATIONS = {
    # name: the SADs of the scene's matches, level 0, exact.  What the median rule keeps is the reading's to say.
    "median_one": [40],
    "median_zeros": [0, 0, 0],                       # median 0: thDist 0, everything goes, n_matched == 0
    "median_two": [3, 9],
    "median_equal": [17, 17, 17, 17],
    "median_bin_256": [255, 256, 257],               # the rank falls into the second coarse bin of the radix select, after a full one
    "median_bin_512": [100, 511, 512, 600],          # ... and into the third
    "median_cut_100": [100, 100, 100, 100, 209, 210, 211],   # floor(2.1 * 100) - 1 .. + 1
}


@functools.lru_cache(maxsize=None)
def build_scenes(w, h, seed=0):
    """-> (L, R, scenes, builder): the uint8 image pair and the directed scenes on it"""
    b = Builder(w, h, seed)
    bal = b.scene("ballast", KITTI)                # nine exact pairs of SAD 30 that keep other scenes' medians above 0
    for _ in range(9):
        b.exact_pair(bal, 30, SX_MATCHED)
    ballast = range(9)
    _edges(b, 0)
    _edges(b, 3)
    _gates(b)
    _clipped(b)
    _long_run(b)
    _disparity(b, ballast)
    _sad_ties(b, ballast)
    for name, sads in MEDIAN_POPULATIONS.items():
        sc = b.scene(name, KITTI)
        for s in sads:
            b.exact_pair(sc, s, None, tag="median")   # kept or removed: test_stereo_cpu states it from the reading
    L, R = b.images()
    return L, R, tuple(b.scenes), b


# ---- the census --------------------------------------------------------------------------------------------------------------------
TABLE_EXITS = (SX_ROW_EMPTY, SX_NO_CANDIDATE, SX_HAMMING, SX_LEFT_WINDOW, SX_RIGHT_SPAN, SX_RIGHT_WINDOW, SX_END_SHIFT, SX_DISPARITY,
               SX_CLAMPED, SX_MATCHED, SX_MEDIAN)
# SX_DELTA (deltaR < -1 || deltaR > 1, Frame.cc:613-614) is exempt: it cannot fire.  The minimum is the FIRST one under a strict <
# and shift -5 is excluded, so with a = d1 - d2 and b = d3 - d2: a > 0 and b >= 0, and deltaR = (a - b) / (2 (a + b)) lies in
# (-0.5, 0.5]; the denominator is never 0, so deltaR is never NaN; the sums are integers below 2^16, exact as floats.  The kernel
# keeps its test because it mirrors the reference.


def census(results):
    """results: [(scene, exits, facts)] of one geometry's scene set.  Returns the list of census conditions that do NOT hold."""
    missing = []
    allx = np.concatenate([e for _, e, _ in results])
    lev = np.concatenate([s.arrays()[0]["octave"] for s, _, _ in results])
    touch = np.concatenate([f["per_keypoint"]["touches"] for _, _, f in results])
    total = lambda k: sum(f[k] for _, _, f in results)
    for x in TABLE_EXITS:
        if (allx == x).sum() < 4:
            missing.append(f"fewer than 4 left keypoints take the exit '{EXIT_NAMES[x]}'")
    if (allx == SX_DELTA).any() or (allx == SX_OUTSIDE).any():
        missing.append("a keypoint took the unreachable deltaR exit or lies outside the input domain")
    for x in (SX_LEFT_WINDOW, SX_RIGHT_SPAN, SX_RIGHT_WINDOW):
        for name, sel in (("level 0", lev == 0), ("a level >= 3", lev >= 3)):
            if not ((allx == x) & sel).any():
                missing.append(f"the exit '{EXIT_NAMES[x]}' is not taken at {name}")
    for name, sel in (("level 0", lev == 0), ("a level >= 3", lev >= 3)):
        if not (touch & sel & np.isin(allx, (SX_MATCHED, SX_CLAMPED))).any():
            missing.append(f"no window that touches its level's border is kept at {name}")
    delta = np.concatenate([f["per_keypoint"]["delta"] for _, _, f in results])
    ties = np.concatenate([f["per_keypoint"]["sad_ties"] for _, _, f in results])
    if not (allx == SX_DISPARITY).any() or not (allx == SX_CLAMPED).any() or not (allx == SX_MATCHED).any():
        missing.append("the disparity gate is not taken on both sides, or the 0.01 clamp never")
    if max(f["longest_run"] for _, _, f in results) <= 64:
        missing.append("no candidate run is longer than 64")
    if total("hamming_ties_dx") < 1:
        missing.append("no Hamming tie between candidates of different x")
    if not ((ties > 0) & (allx == SX_MATCHED)).any() or not ((ties > 0) & (allx == SX_END_SHIFT)).any():
        missing.append("no SAD tie that is kept, or none at an end shift")
    if not ((ties > 0) & (delta == _f32(0.5))).any():
        missing.append("no SAD tie with deltaR == 0.5")
    if total("clipped_top") < 1 or total("clipped_bottom") < 1:
        missing.append("no right band clipped at the top, or none at the bottom")
    if total("at_min_u") < 1 or total("at_max_u") < 1:
        missing.append("uR == minU or uR == maxU does not occur")
    if total("best_74") < 1 or total("best_75") < 1:
        missing.append("a best distance of 74 or of 75 does not occur")
    pops = [f["median_in"] for _, _, f in results]
    for name, p in MEDIAN_POPULATIONS.items():
        if sorted(p) not in pops:
            missing.append(f"the median population {name} does not occur")
    return missing


def exit_counts(results):
    allx = np.concatenate([e for _, e, _ in results])
    return {EXIT_NAMES[x]: int((allx == x).sum()) for x in TABLE_EXITS}
