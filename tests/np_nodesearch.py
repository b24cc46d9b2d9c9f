"""The searches over common vocabulary nodes -- SearchByBoW(KeyFrame*, Frame&) (L/src/ORBmatcher.cc:161-273, form "frame"),
SearchByBoW(KeyFrame*, KeyFrame*) (:494-612, form "kf"), SearchForTriangulation (:614-764, form "tri") -- and SearchForInitialization
(:388-492, form "init") on DIRECTED input: a builder of scenes with hand-placed features, and the census of what those scenes reach.

  bow_walk / tri_walk / init_walk   tests/np_restatement -- the one body behind each ref_search_* reading -- with an exit per visit of
                 a first-side feature and the facts the census reads
  build_scenes   the scenes of one form; a scene holds descriptors, angles, keypoints, masks, the two FeatureVectors (or the second
                 frame and vbPrevMatched) and the parameters, and the exit every placed feature was placed for.  Building a scene walks
                 it and asserts those exits.  Every scene with proper FeatureVectors has a twin (Scene.twin) that the device takes on
                 its one-wave sequential path and whose result is the same by construction (asserted).
  census         the conditions tests/test_nodesearch_cpu.py asserts on the walk's own exits and facts (never on a kernel's output)

Descriptors follow tests/np_projection.py: the base pattern with chosen bits turned -- first-side features in bits 255 downwards,
second-side features in bits 0 upwards -- so that every distance is the size of a known set; the taken-chain turns named bits.

What the undirected inputs reach and what the directed scenes reach, visits per exit and facts of the walk.  "before" is the input of
tests/test_matcher_gpu.py::test_search_by_bow_grouped (both SearchByBoW forms, ratio 0.7), ::test_search_for_triangulation
(only_stereo False, mono False) and ::test_search_for_initialization (window 30, ratio 0.9), each with the rotation check, rebuilt with
the C oracle's extractor (previous_inputs() below; test_nodesearch_cpu.py prints both columns):

  exit / fact                                KF-Frame            KF-KF               triangulation       initialisation
                                             before  directed    before  directed    before  directed    before  directed
  never visited (no common node)                  0        14         0        14         0        14         -         -
  skipped as invalid                            210         4       210         4       299         4       787         2
  empty list or window                            0         1         0         1         0         2         2         4
  every candidate taken or gated                  0         2         0         3        63        12         3         2
  over the distance threshold                   347         3       429         5       386         4        85         3
  rejected by the ratio test                    114        60        84        60         -         -         0         7
  matched                                       325       312       270       305       255       255       125       194
  matched, then stolen or overwritten             -         -         0         4         0         4         1        10
  removed by the rotation check                   8        53        11        53         1        53         1        54
  list lengths hit of 1, 63, 64, 65, 128, 129  none       all      none       all      none       all         1  1, 64, 65
  best at place 64 or later                      32        23        38        23        11        11         0         1
  second-best in the winner's lane, 64 on         0        19         0        19         -         -         0         0
  second-best equal to the best                  22         6        20         6         -         -         2         1
  single candidate                                0       254         0       254         -         -        41       253
  ties at the winning distance / 64 apart         -         -         -         -     0 / 0    11 / 6         -         -
  best distance 49 / 50 / 51               10/9/7     6/3/2   6/10/6     5/2/2    1/3/-     2/2/-   2/0/1     2/2/2
  rotation bins hit                     0 1 6 11 12   0 .. 12  7 of 13   0 .. 12   0 3 12   0 .. 12  0 5 12   0 .. 12
  calls with an empty histogram                   0         2         0         2         0         3         0         1
  most pushes of one feature                      1         3         1         3         1         3         1         1
  calls with more pushes than features            0         2         0         2         0         2         -         -
  longest run of visits skipping a taken one      5        70         4        70         -         -         -         -
  candidates removed by the epipole disc          -         -         -         -         0         6         -         -
  ... by den == 0                                 -         -         -         -         0         4         -         -
  ... by the epipolar distance                    -         -         -         -       176         7         -         -
  deepest steal chain                             -         -         -         -         -         -         1         3
  steals refused at equal distance                -         -         -         -         -         -         0         1
  histogram entries of stolen matches             -         -         -         -         -         -         1        10
  windows outside the grid                        -         -         -         -         -         -         0         2

The directed columns leave the twins out (they repeat every row) and are what test_nodesearch_cpu.py asserts through census().  The
undirected inputs never list a feature twice, never hit one of the six list lengths at which the lane striding changes (KF-Frame,
KF-KF, triangulation), never tie a triangulation candidate, never meet the epipole disc or a degenerate line, never steal twice from
one keypoint or refuse a steal at equal distance, never leave the histogram empty, and fill 3 to 7 of the 13 reachable bins.

Three comparisons cannot be told apart by any input and have no scene (test_nodesearch_cpu.EQUIVALENT says why): `<` against `<=` for
the best and for the second-best of SearchByBoW and SearchForInitialization, and the `den == 0` test of CheckDistEpipolarLine.
Bins 13 .. 29 of the rotation histogram are unreachable, as in tests/np_projection.py.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import np_projection as npj
from tests import np_restatement as nr
from tests.np_projection import BASE, SCALE_FACTORS, bits
from tests.np_restatement import (NX_UNVISITED, NX_INVALID, NX_EMPTY, NX_ALL_GONE, NX_TOO_FAR, NX_RATIO, NX_MATCHED, NX_STOLEN,  # noqa: F401
                                  NX_ROTATION, TG_INVALID, TG_FAR, TG_WORSE, TG_EPIPOLE, TG_DEN, TG_EPIPOLAR, TG_PASSED, TH_LOW)
from tests.oracle_lib import EPIPOLAR_DTYPE, KP_DTYPE

EXIT_NAMES = {NX_UNVISITED: "never visited (no common node)", NX_INVALID: "skipped as invalid", NX_EMPTY: "empty list or window",
              NX_ALL_GONE: "every candidate taken or gated", NX_TOO_FAR: "over the distance threshold", NX_RATIO: "rejected by the ratio test",
              NX_MATCHED: "matched", NX_STOLEN: "matched, then stolen or overwritten", NX_ROTATION: "removed by the rotation check"}
FORMS = ("frame", "kf", "tri", "init")
RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)            # the mfNNratio values the reference's callers construct ORBmatcher with
LIST_LENGTHS = (1, 63, 64, 65, 128, 129)
TWIN_NODES = (1 << 20, (1 << 20) + 1)
_f32 = np.float32
# SearchForTriangulation: l = x1' F12 = [0, x1, 0], so the epipolar line of every first-side keypoint is y = 0 with den = x1 * x1 and
# num = x1 * y2; the epipole sits at (100, -8), so a second-side keypoint on the line at x = 100 +- 6 is exactly 10 pixels from it
TRI_F12 = ((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
TRI_EX, TRI_EY = 100.0, -8.0
TRI_SIGMA2 = (SCALE_FACTORS * SCALE_FACTORS).astype(np.float32)
TRI_SIGMA2[7] = 150.0                          # 3.84 * 150.0 == 576.0 in double: the one level at which dsqr can EQUAL the bound
assert 3.84 * float(TRI_SIGMA2[7]) == 576.0


def _next(v, up=True):
    return np.nextafter(_f32(v), _f32(np.inf if up else -np.inf))


def _run(start, n):
    """n consecutive floats from `start` upwards and n downwards"""
    i = np.array([start], np.float32).view(np.int32)[0]
    return (i + np.arange(-n, n + 1, dtype=np.int32)).astype(np.int32).view(np.float32)


@functools.lru_cache(maxsize=None)
def ratio_pairs(ratio, limit):
    """(best, second) with float32(ratio) * float32(second) == float32(best) EXACTLY and best + 1 <= limit, so that the step above the
    equality is still a distance the form accepts; plus such a pair on which the float product and the double product decide
    differently if there is one (else None)"""
    r, eq, fd = _f32(ratio), None, None
    for s in range(2, 128):
        p = r * _f32(s)
        b = int(round(float(p)))
        if 2 <= b < limit and p == _f32(b):
            eq = (b, s)                      # the largest such pair: distances of the size matches have
            if (float(b) < float(r) * s) != bool(_f32(b) < p):
                fd = (b, s)
    assert eq, ratio
    return eq, fd


class Scene:
    """hand-placed features of one call of a node search (forms "frame", "kf", "tri"); expect[i]: the exit first-side feature i was
    placed for (None: not stated), on[i]: the second-side feature it ends on"""

    def __init__(self, name, form, nnratio=0.7, check_ori=True, only_stereo=False, with_u_right=True, F12=TRI_F12):
        self.name, self.form, self.nnratio, self.check_ori = name, form, float(_f32(nnratio)), bool(check_ori)
        self.only_stereo, self.with_u_right, self.F12 = only_stereo, with_u_right, F12
        self.A, self.B = [], []
        self.fvA, self.fvB = {}, {}
        self.expect, self.on, self.tags = [], {}, {}
        self._nid = 0
        self.sequential_only = False

    def pick(self, default, **by_form):
        return by_form.get(self.form, default)

    @staticmethod
    def _feat(desc, angle, valid, x, y, octave, ur):
        return dict(desc=desc, angle=_f32(angle), valid=int(valid), x=_f32(x), y=_f32(y), octave=int(octave), ur=_f32(ur))

    def a(self, flips=0, expect=None, angle=0.0, valid=1, x=1.0, y=0.0, octave=0, ur=-1.0, tag=None):
        """a first-side feature: an int turns that many bits from 255 downwards, an iterable the bits it names"""
        self.A.append(self._feat(BASE ^ bits(flips, top=True), angle, valid, x, y, octave, ur))
        self.expect.append(expect)
        if tag:
            self.tags.setdefault(tag, []).append(len(self.A) - 1)
        return len(self.A) - 1

    def b(self, flips=0, angle=0.0, valid=1, x=500.0, y=0.0, octave=0, ur=-1.0, unrelated=None):
        d = (~BASE ^ bits([128 + 9 * j for j in range(unrelated)])) if unrelated is not None else BASE ^ bits(flips)
        self.B.append(self._feat(d, angle, valid, x, y, octave, ur))
        return len(self.B) - 1

    def node(self, la, lb, nid=None, side="both"):
        if nid is None:
            self._nid += 1
            nid = self._nid
        if side in ("both", "A"):
            self.fvA[nid] = list(la)
        if side in ("both", "B"):
            self.fvB[nid] = list(lb)
        return nid

    def case(self, dists, expect, on=None, af=0, tag=None, a_kw=None, b_kw=None):
        """one node: one first-side feature with `af` bits turned and second-side features at the distances given, in list order"""
        ia = self.a(af, expect, tag=tag, **(a_kw or {}))
        lb = [self.b(d - af, **((b_kw or {}).get(p, {}))) for p, d in enumerate(dists)]
        self.node([ia], lb)
        if on is not None:
            self.on[ia] = lb[on]
        return ia, lb

    def _arrays(self, feats):
        keys = np.zeros(len(feats), KP_DTYPE)
        for f, k in zip(feats, keys):
            k["x"], k["y"], k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = f["x"], f["y"], f["octave"], f["angle"], 31.0, 1.0, -1
        desc = np.array([f["desc"] for f in feats], np.uint8).reshape(-1, 32)
        return keys, desc, np.array([f["valid"] for f in feats], np.uint8), np.array([f["ur"] for f in feats], np.float32)

    def finish(self, check=True):
        self.keysA, self.descA, self.validA, self.urA = self._arrays(self.A)
        self.keysB, self.descB, self.validB, self.urB = self._arrays(self.B)
        self.angleA, self.angleB = self.keysA["angle"].copy(), self.keysB["angle"].copy()
        self.hasA, self.hasB = (1 - self.validA).astype(np.uint8), (1 - self.validB).astype(np.uint8)   # tri: "has a map point"
        self.ep = np.zeros(1, EPIPOLAR_DTYPE)
        self.ep["F12"][0] = np.array(self.F12, np.float32).reshape(9)
        self.ep["ex"], self.ep["ey"] = TRI_EX, TRI_EY
        self.ep["scale_factors"][0, :len(SCALE_FACTORS)] = SCALE_FACTORS
        self.ep["level_sigma2"][0, :len(TRI_SIGMA2)] = TRI_SIGMA2
        self.result = self.walk()
        if check:
            nm, res, exits, facts = self.result
            for i, want in enumerate(self.expect):
                assert want is None or exits[i] == want, (self.name, self.form, i, EXIT_NAMES[want], EXIT_NAMES[int(exits[i])])
            for i, j in self.on.items():
                if exits[i] == NX_MATCHED:
                    assert (res[j] == i) if self.form == "frame" else (res[i] == j), (self.name, self.form, i, j)
            assert nm == int((res >= 0).sum()) or facts["dup_a"], (self.name, self.form)
        return self

    def walk(self, rules=None, check_ori=None):
        """(n_matches, result, exits, facts): result is matchB in the form "frame", matchA otherwise"""
        check = self.check_ori if check_ori is None else check_ori
        if self.form == "tri":
            ur = (self.urA, self.urB) if self.with_u_right else (None, None)
            return nr.tri_walk(self.keysA, self.descA, ur[0], self.hasA, self.fvA, self.keysB, self.descB, ur[1], self.hasB, self.fvB,
                               self.F12, TRI_EX, TRI_EY, SCALE_FACTORS, TRI_SIGMA2, self.only_stereo, check, rules)
        return nr.bow_walk(self.descA, self.angleA, self.validA, self.fvA, self.descB, self.angleB, self.validB, self.fvB,
                           self.nnratio, check, self.form == "kf", rules)

    def twin(self):
        """the same call with one more first-side feature, invalid, listed under two more common nodes whose second-side lists repeat a
        feature already listed: a feature recurs on either side, so every form replays sequentially, and nothing else changes"""
        t = Scene(self.name + "+twin", self.form, self.nnratio, self.check_ori, self.only_stereo, self.with_u_right, self.F12)
        t.A, t.B = list(self.A), list(self.B)
        t.fvA, t.fvB = {k: list(v) for k, v in self.fvA.items()}, {k: list(v) for k, v in self.fvB.items()}
        t.expect, t.on, t.tags = list(self.expect), dict(self.on), self.tags
        z = t.a(0, NX_INVALID, valid=0)
        listed = [j for _, _, lb in nr._featvec_pairs(self.fvA, self.fvB) for j in lb]
        b0 = listed[0] if listed else t.b(0)
        for nid in TWIN_NODES:
            t.fvA[nid], t.fvB[nid] = [z], [b0, b0] if not listed else [b0]
        t.finish()
        assert t.result[0] == self.result[0], t.name
        n = len(self.result[1])
        assert t.result[1][:n].tobytes() == self.result[1].tobytes() and (t.result[1][n:] == -1).all(), t.name
        assert t.result[2][:len(self.A)].tobytes() == self.result[2].tobytes(), t.name
        return t


class InitScene(npj.Scene):
    """SearchForInitialization: the second frame is placed with the helpers of tests/np_projection.py (kp, site), the keypoints of the
    first frame with k1(); vbPrevMatched[i1] is where k1 puts it"""

    def __init__(self, name, nnratio=0.9, check_ori=True, window=5, w=640, h=480):
        super().__init__(name, "frame", w, h, check_ori=check_ori)
        self.form, self.nnratio, self.window = "init", float(_f32(nnratio)), int(window)
        self._k1, self._d1, self._prev = [], [], []

    def k1(self, x, y, flips=0, expect=None, octave=0, angle=0.0, on=None, tag=None):
        self._k1.append((_f32(x), _f32(y), _f32(31.0), _f32(angle), _f32(1), octave, -1))
        self._d1.append(BASE ^ bits(flips, top=True)); self._prev.append((_f32(x), _f32(y)))
        self.expect.append(expect)
        i = len(self._k1) - 1
        if on is not None:
            self.on[i] = on
        if tag:
            self.tags.setdefault(tag, []).append(i)
        return i

    def finish(self):
        self.keys = np.array(self._k, KP_DTYPE) if self._k else np.zeros(0, KP_DTYPE)
        self.desc = np.array(self._d, np.uint8).reshape(-1, 32)
        self.keys1 = np.array(self._k1, KP_DTYPE)
        self.desc1 = np.array(self._d1, np.uint8).reshape(-1, 32)
        self.prev = np.array(self._prev, np.float32).reshape(-1, 2)
        self.result = self.walk()
        nm, m12, prev, exits, facts = self.result
        for i, want in enumerate(self.expect):
            assert want is None or exits[i] == want, (self.name, i, EXIT_NAMES[want], EXIT_NAMES[int(exits[i])])
        for i, k in self.on.items():
            if exits[i] in (NX_MATCHED, NX_STOLEN, NX_ROTATION):
                assert facts["visits"][i]["match"] == k, (self.name, i, k, facts["visits"][i]["match"])
        assert nm == int((m12 >= 0).sum()), self.name
        return self

    def ref_frame(self):
        return nr.RefFrame(self.keys, self.desc, 0, self.w, 0, self.h, None)

    def walk(self, rules=None, check_ori=None):
        """(n_matches, vnMatches12, vbPrevMatched as an (n1, 2) float32 array, exits, facts)"""
        nm, m12, prev, exits, facts = nr.init_walk(self.keys1, self.desc1, self.ref_frame(), self.prev, self.window, self.nnratio,
                                                   self.check_ori if check_ori is None else check_ori, rules)
        return nm, m12, np.array(prev, np.float32).reshape(-1, 2), exits, facts


# ---- scenes of the two SearchByBoW forms --------------------------------------------------------------------------------------------
def _lanes(sc, n):
    """one list length at which the lane striding changes (1, 63, 64, 65, 128, 129) with the best first, last and in between, and the
    second-best -- which alone decides the ratio test: 22 against 30 fails at 0.7, 22 against the fill of 48 would pass -- in the
    winner's own lane (positions 3 and 67), in another lane (3 and 4), first and last; and the same with 20 for 22, matched."""
    spots = {(0, n - 1), (n - 1, 0), (3, 4), (4, 3), (3, 67), (67, 3), (n - 1, n - 2)}
    for bp, sp in sorted(p for p in spots if max(p) < n and min(p) >= 0 and p[0] != p[1]):
        for best, ex in ((22, NX_RATIO), (20, NX_MATCHED)):
            d = [48] * n
            d[bp], d[sp] = best, 30
            sc.case(d, ex, on=bp, tag=f"len{n}")
    if n == 1:
        for _ in range(4):
            sc.case([20], NX_MATCHED, on=0, tag="single")       # a single candidate: second-best 256


def _ties(sc):
    """equal best distances inside one lane and across lanes: the second-best equals the best and the ratio test rejects; equal
    SECOND-best distances leave the decision alone"""
    for n, pos in ((70, (3, 67)), (70, (3, 4)), (129, (0, 128)), (129, (64, 128)), (2, (0, 1))):
        d = [48] * n
        for p in pos:
            d[p] = 20
        sc.case(d, NX_RATIO, tag="best_tie")
    for pos in ((3, 67), (3, 4)):
        d = [48] * 70
        d[10] = 20
        for p in pos:
            d[p] = 30
        sc.case(d, NX_MATCHED, on=10, tag="second_tie")


def _thresholds(sc):
    """49, 50 and 51 against TH_LOW, alone in the list and with a far second-best"""
    for d in (49, 50, 51):
        ex = sc.pick(NX_MATCHED if d <= 50 else NX_TOO_FAR, kf=NX_MATCHED if d < 50 else NX_TOO_FAR)
        sc.case([d], ex, on=0, tag=f"dist{d}")
        sc.case([120, d, 127], ex, on=1, tag=f"dist{d}")


def _ratio(sc, ratio):
    """best == ratio * second exactly in float32 (rejected: the test is a strict <), one below (matched), one above (rejected); the
    decimal equalities 0.6 * 50 .. 0.9 * 50, which float32 decides one way or the other; a pair the double product decides otherwise"""
    limit = sc.pick(50, kf=49)
    (b, s), fd = ratio_pairs(ratio, limit)
    verdict = lambda b_, s_: NX_MATCHED if _f32(b_) < _f32(ratio) * _f32(s_) else NX_RATIO
    sc.case([s, b], NX_RATIO, on=1, tag="ratio_eq")
    sc.case([s, b - 1], NX_MATCHED, on=1, tag="ratio_below")
    assert b + 1 <= limit
    sc.case([b + 1, s], NX_RATIO, on=0, tag="ratio_above")
    for s_ in (50, 40, 20):
        b_ = int(round(ratio * s_))
        if abs(ratio * s_ - b_) < 1e-9 and b_ <= limit:
            sc.case([b_, s_], verdict(b_, s_), on=0, tag="ratio_decimal")
    if fd:
        sc.case([fd[1], fd[0]], NX_RATIO, on=1, tag="ratio_float_not_double")


CHAIN = 70


def _chain(sc):
    """70 keyframe features and 70 frame features in one node (ratio 0.9).  F(j) turns bits 3j .. 3j + 2.  K(0) turns F(0)'s bits
    (distance 0); K(i) turns F(0)'s three bits, two of F(i - 1)'s and one of F(i)'s: 3 from F(0), 5 from F(i - 1), 7 from F(i), 9 from
    every other.  So EVERY keyframe feature is nearest to F(0), which K(0) takes; K(i) then ends on F(i) only if F(0) and F(i - 1) --
    taken one step earlier -- are out of both its best (else it would take them) and its second-best (7 against 3 or 5 fails the
    ratio test, against 9 it passes): a dependency chain as long as the node, across the lane boundary at 64."""
    U = lambda j: [3 * j, 3 * j + 1, 3 * j + 2]
    la, lb = [], []
    for j in range(CHAIN):
        sc.B.append(sc._feat(BASE ^ bits(U(j)), 0.0, 1, 500.0, 0.0, 0, -1.0))
        lb.append(len(sc.B) - 1)
    for i in range(CHAIN):
        turned = U(0) if i == 0 else sorted(set(U(0) + U(i - 1)[:2] + U(i)[:1]))
        sc.A.append(sc._feat(BASE ^ bits(turned), 0.0, 1, 1.0, 0.0, 0, -1.0))
        sc.expect.append(NX_MATCHED)
        la.append(len(sc.A) - 1)
        sc.on[la[-1]] = lb[i]
    sc.node(la, lb)


def _invalid(sc):
    """invalid features on the first side (skipped), on the second side (KF-KF: never a candidate; KF-Frame reads no such mask), and
    nodes whose features are all invalid on one side"""
    ia = sc.a(0, NX_INVALID, valid=0)
    ib = sc.a(0, NX_MATCHED)
    b = [sc.b(10), sc.b(30)]
    sc.node([ia, ib], b); sc.on[ib] = b[0]
    # the nearest second-side feature is invalid: KF-KF goes on to the next (distance 30, second-best 48)
    ic = sc.a(0, sc.pick(NX_MATCHED))
    b = [sc.b(10, valid=0), sc.b(30), sc.b(48)]
    sc.node([ic], b); sc.on[ic] = sc.pick(b[0], kf=b[1])
    # all invalid on the first side; all invalid on the second side
    sc.node([sc.a(0, NX_INVALID, valid=0) for _ in range(3)], [sc.b(10), sc.b(20)])
    sc.node([sc.a(0, sc.pick(NX_MATCHED, kf=NX_ALL_GONE))], [sc.b(10, valid=0), sc.b(30, valid=0)])
    # one second-side feature for two first-side ones: the second finds everything taken
    sc.node([sc.a(0, NX_MATCHED), sc.a(0, NX_ALL_GONE), sc.a(3, NX_ALL_GONE)], [sc.b(10)])
    # an empty second-side list, and an empty first-side list
    sc.node([sc.a(0, NX_EMPTY)], [])
    sc.node([], [sc.b(10)])


LAYOUTS = {
    # name: (node ids of the first side, of the second side)
    "layout_mixed": ((1, 2, 3, 10, 11, 20, 30, 31, 32, 40), (1, 5, 6, 7, 10, 20, 21, 22, 40)),   # first and last shared, runs of misses
    "layout_one": ((2, 4, 9, 12), (1, 3, 9, 10, 11, 13)),                                          # one shared node
    "layout_none": ((1, 3, 5), (2, 4, 6)),                                                          # no shared node
    "layout_tail": ((7, 8, 9), (1, 2, 3, 4, 5, 9)),                                                 # only the last shared, after a run
}


def _layout(sc, idsA, idsB):
    """one feature per node and side, at distance 10; a feature of a node only one side holds is never visited"""
    for nid in sorted(set(idsA) | set(idsB)):
        both = nid in idsA and nid in idsB
        la = [sc.a(0, NX_MATCHED if both else NX_UNVISITED)] if nid in idsA else []
        lb = [sc.b(10)] if nid in idsB else []
        if nid in idsA:
            sc.fvA[nid] = la
        if nid in idsB:
            sc.fvB[nid] = lb
        if both:
            sc.on[la[0]] = lb[0]


# ---- rotation scenes, every form ----------------------------------------------------------------------------------------------------
ROTATION_SCENES = {
    # name: ({bin: entries}, the bins ComputeThreeMaxima keeps)
    "rot_10_1": ({0: 10, 1: 1}, {0, 1}),                        # max2 = 1 is not < 0.1f * 10: kept
    "rot_11_1": ({0: 11, 1: 1}, {0}),                           # 1 < 0.1f * 11: dropped
    "rot_third_kept": ({0: 10, 1: 5, 2: 1}, {0, 1, 2}),         # max3 = 1 is not < 0.1f * 10
    "rot_third_dropped": ({0: 11, 1: 5, 2: 1}, {0, 1}),
    "rot_every_bin": ({**{0: 10, 1: 5, 12: 2}, **{b: 1 for b in range(2, 12)}}, {0, 1, 12}),
    "rot_one_bin": ({4: 3}, {4}),
    "rot_tie2": ({3: 4, 7: 4, 9: 1}, {3, 7, 9}),                # two equal maxima
    "rot_tie3": ({3: 4, 7: 4, 9: 4, 11: 1}, {3, 7, 9}),
    "rot_tie4": ({3: 4, 7: 4, 9: 4, 11: 4}, {3, 7, 9}),         # four equal maxima: the first three
    "rot_tie_second": ({0: 10, 3: 4, 7: 4, 9: 4}, {0, 3, 7}),   # equal second and third places: the earlier bins
    "rot_tie_third": ({0: 10, 1: 5, 3: 4, 7: 4}, {0, 1, 3}),
}


def _entry(sc, angle_a, angle_b, expect, tag=None):
    """one match with the two angles given, alone in its node or window"""
    if sc.form == "init":
        cx, cy = sc.site()
        k = sc.kp(cx, cy, 0, 10, angle=angle_b)
        return sc.k1(cx, cy, 0, expect, angle=angle_a, on=k, tag=tag)
    return sc.case([10], expect, on=0, tag=tag, a_kw=dict(angle=angle_a), b_kw={0: dict(angle=angle_b)})[0]


def _rotation(sc, counts, kept):
    for b in sorted(counts):
        for n in range(counts[b]):
            rot = 30.0 * b + (3.0 if n % 2 else 0.0) if b < 12 else 350.0 + 5.0 * (n % 2)
            _entry(sc, 40.0 + rot if 40.0 + rot < 360 else rot, 40.0 if 40.0 + rot < 360 else 0.0,
                   NX_MATCHED if (b in kept or not sc.check_ori) else NX_ROTATION, tag=f"bin{b}")


def _rot_bounds(sc):
    """every reachable half-bin boundary: rot = 15 + 30 k exactly and the float to each side (rot * (1 / 30.f) sits on k + .5 or beside
    it, and round() goes away from zero); a negative difference so small that rot + 360 rounds to 360.0f (bin 12, not the wrap)."""
    for k in range(12):
        r0 = _f32(15.0 + 30.0 * k)
        for r in (_next(r0, False), r0, _next(r0)):
            _entry(sc, r, 0.0, None, tag="bound")
    _entry(sc, 0.0, 1e-6, None, tag="neg360")
    _entry(sc, 10.0, 40.0, None, tag="negative")


def _empty_hist(sc):
    """the rotation check on an empty histogram: nothing matches"""
    if sc.form == "init":
        cx, cy = sc.site()
        sc.kp(cx, cy, 0, 60)
        sc.k1(cx, cy, 0, NX_TOO_FAR)
    else:
        sc.case([60], NX_TOO_FAR)


# ---- scenes of SearchForTriangulation ----------------------------------------------------------------------------------------------
def _tri_lists(sc):
    """list lengths and the last-wins rule: equal distances inside one lane (3 and 67), across lanes (3 and 4), at both ends of a list,
    and with the later candidate removed by a gate (off the epipolar line; holding a map point)"""
    for n in LIST_LENGTHS:
        for bp in sorted({0, n - 1, min(3, n - 1)}):
            d = [45] * n
            d[bp] = 20
            sc.case(d, NX_MATCHED, on=bp, tag=f"len{n}")
        sc.case([45] * n, NX_MATCHED, on=n - 1, tag="tie_all")          # every candidate tied: the last one
    for n, pos in ((70, (3, 67)), (70, (3, 4)), (129, (0, 128)), (129, (64, 128))):
        d = [45] * n
        for p in pos:
            d[p] = 20
        sc.case(d, NX_MATCHED, on=pos[1], tag="tie")
        sc.case(d, NX_MATCHED, on=pos[0], tag="tie_gated", b_kw={pos[1]: dict(y=5.0)})
        sc.case(d, NX_MATCHED, on=pos[0], tag="tie_has_mp", b_kw={pos[1]: dict(valid=0)})
    for d, ex in ((49, NX_MATCHED), (50, NX_MATCHED), (51, NX_TOO_FAR)):
        sc.case([d], ex, on=0, tag=f"dist{d}")
        sc.case([d, 60], ex, on=0, tag=f"dist{d}")


def disc_floats(octave):
    """x offsets from the epipole of a keypoint on the line y = 0 (8 pixels from the epipole in y) whose float distance**2 is the
    nearest reachable below 100 * scaleFactor, the nearest at or above it, and one on which the double form decides otherwise (None)"""
    lim = _f32(100) * SCALE_FACTORS[octave]
    dx0 = _f32(np.sqrt(float(lim) - 64.0))
    ex, ey = _f32(TRI_EX), _f32(TRI_EY)
    xs = _run(ex + dx0, 20000)
    dex = ex - xs
    d2 = dex * dex + (ey - _f32(0)) * (ey - _f32(0))
    assert d2.dtype == np.float32
    below, above = xs[d2 < lim], xs[d2 >= lim]
    x_in = below[np.argmax(d2[d2 < lim])]
    x_out = above[np.argmin(d2[d2 >= lim])]
    dd = dex.astype(np.float64) ** 2 + 64.0
    differ = xs[(d2 < lim) != (dd < 100.0 * float(SCALE_FACTORS[octave]))]
    return x_in, x_out, (differ[0] if len(differ) else None)


def _tri_disc(sc):
    """the epipole disc (two monocular keypoints only): exactly 10 pixels away on level 0 (100 < 100 fails: kept), the nearest floats to
    each side of 100 * 1.2f on level 1, all four stereo combinations well inside it, u_right 0.0 and -0.0 (stereo: >= 0)"""
    sc.case([20], NX_MATCHED, on=0, tag="disc_eq", b_kw={0: dict(x=TRI_EX + 6.0)})
    sc.case([20], NX_MATCHED, on=0, tag="disc_eq", b_kw={0: dict(x=TRI_EX - 6.0)})
    sc.case([20], NX_ALL_GONE, tag="disc_in", b_kw={0: dict(x=_next(TRI_EX + 6.0, False))})
    x_in, x_out, _ = disc_floats(1)
    sc.case([20], NX_ALL_GONE, tag="disc_l1_in", b_kw={0: dict(x=x_in, octave=1)})
    sc.case([20], NX_MATCHED, on=0, tag="disc_l1_out", b_kw={0: dict(x=x_out, octave=1)})
    differ = disc_floats(4)[2]       # level 4: the float sum equals the float bound 207.36003 (not inside: kept); in double it is inside
    assert differ is not None
    dex = _f32(TRI_EX) - differ
    inside = dex * dex + _f32(64) < _f32(100) * SCALE_FACTORS[4]
    sc.case([20], NX_ALL_GONE if inside else NX_MATCHED, on=0, tag="disc_float_not_double", b_kw={0: dict(x=differ, octave=4)})
    for ua, ub in ((-1.0, -1.0), (5.0, -1.0), (-1.0, 5.0), (5.0, 5.0), (0.0, -1.0), (-0.0, -1.0), (-1.0, 0.0), (-1.0, -0.0)):
        mono = ua == -1.0 and ub == -1.0
        sc.case([20, 30], NX_ALL_GONE if mono else NX_MATCHED, on=0, tag="disc_stereo",
                a_kw=dict(ur=ua), b_kw={0: dict(x=TRI_EX + 1.0, ur=ub), 1: dict(x=TRI_EX + 2.0, ur=ub)})


@functools.lru_cache(maxsize=None)
def epipolar_floats(octave):
    """(x1, y2 below, y2 above): dsqr = (x1 * y2)**2 / (x1 * x1), all in float, is the largest float below 3.84 * sigma2 for the first
    y2 and the smallest float at or above it for the second"""
    T = 3.84 * float(TRI_SIGMA2[octave])
    lo = _f32(T)
    if float(lo) >= T:
        lo = _next(lo, False)
    hi = _next(lo)
    assert float(lo) < T <= float(hi)
    for x1 in (1.0, 1.25, 1.5, 3.0, 0.75, 1.1, 1.3, 1.7, 2.3, 0.9, 7.0, 1.05):
        x1 = _f32(x1)
        ys = _run(_f32(np.sqrt(T)), 4000)
        num = x1 * ys
        dsqr = (num * num) / (x1 * x1)
        assert dsqr.dtype == np.float32
        a, b = ys[dsqr == lo], ys[dsqr == hi]
        if len(a) and len(b):
            return x1, a[0], b[0], lo, hi
    raise AssertionError(("no bracket found", octave))


def _tri_epipolar(sc):
    """the epipolar gate at the two floats that bracket 3.84 * sigma2 on levels 0 and 1 (on level 0 the lower one IS 3.84f: a float
    comparison would refuse it), at equality on the level whose bound 3.84 * 150 is a float, and a degenerate line (den == 0)"""
    for octave in (0, 1):
        x1, y_in, y_out, lo, hi = epipolar_floats(octave)
        sc.case([20], NX_MATCHED, on=0, tag=f"epi{octave}_in", a_kw=dict(x=x1), b_kw={0: dict(y=y_in, octave=octave)})
        sc.case([20], NX_ALL_GONE, tag=f"epi{octave}_out", a_kw=dict(x=x1), b_kw={0: dict(y=y_out, octave=octave)})
        sc.case([20], NX_MATCHED, on=0, tag=f"epi{octave}_in", a_kw=dict(x=x1), b_kw={0: dict(y=-y_in, octave=octave)})
    sc.case([20], NX_ALL_GONE, tag="epi_equal", b_kw={0: dict(y=24.0, octave=7)})
    sc.case([20], NX_MATCHED, on=0, tag="epi_equal_in", b_kw={0: dict(y=_next(24.0, False), octave=7)})
    sc.case([20, 30], NX_ALL_GONE, tag="den0", a_kw=dict(x=0.0))


def _tri_masks(sc):
    """has_mp on either side, monocular and stereo keypoints (the scene runs with and without only_stereo)"""
    mono_out = NX_INVALID if sc.only_stereo else NX_MATCHED
    sc.case([20], NX_INVALID, a_kw=dict(valid=0))
    sc.case([20, 30], NX_MATCHED, on=1, b_kw={0: dict(valid=0), 1: dict(ur=4.0)}, a_kw=dict(ur=3.0))
    sc.case([20], NX_ALL_GONE, b_kw={0: dict(valid=0)}, a_kw=dict(ur=3.0))
    sc.case([20], mono_out, on=0, b_kw={0: dict(ur=4.0)})
    sc.case([20, 30], NX_MATCHED, on=1 if sc.only_stereo else 0, a_kw=dict(ur=3.0), b_kw={1: dict(ur=4.0)})
    sc.case([20], NX_ALL_GONE if sc.only_stereo else NX_MATCHED, on=0, a_kw=dict(ur=3.0))
    sc.case([20], NX_MATCHED, on=0, a_kw=dict(ur=0.0), b_kw={0: dict(ur=-0.0)})
    sc.case([20], mono_out, on=0)
    sc.node([sc.a(0, NX_EMPTY, ur=3.0)], [])


# ---- scenes that only make sense on the sequential path ---------------------------------------------------------------------------------
def _dup_b(sc):
    """a second-side feature listed under two nodes -- once matched it is gone in the later node, wherever it is listed (SearchByBoW) --
    and twice within one node: the two listings tie, so the ratio test rejects.  In SearchForTriangulation nothing is ever taken and
    the last listing wins."""
    tri = sc.form == "tri"
    a1, a2, a3, a4 = sc.a(0, NX_MATCHED), sc.a(5, NX_MATCHED), sc.a(0, NX_MATCHED), sc.a(0, NX_MATCHED if tri else NX_RATIO)
    b = [sc.b(10), sc.b(30), sc.b(45)]
    c = sc.b(31)
    sc.node([a1, a2], [b[0], b[1], b[2], b[2]])                  # a2: 35 against 50, 0.9 passes
    sc.node([a3], [b[0], b[1], c, b[0]])                         # b[0] and b[1] went in the node before
    sc.node([a4], [b[2], b[2]])
    sc.on.update({a1: b[0], a2: b[0] if tri else b[1], a3: b[0] if tri else c, a4: b[2]})
    sc.sequential_only = True


def _dup_a(sc):
    """a first-side feature listed under three common nodes: visited three times.  KF-Frame: it matches three frame features, so the
    histogram takes more entries than there are first-side features.  KF-KF and triangulation: vpMatches12 is overwritten, every visit
    counts; the entry of the middle visit falls to the rotation check, which clears the slot whatever it holds."""
    a1 = sc.a(0, NX_MATCHED, angle=40.0)
    b = [sc.b(10, angle=40.0), sc.b(12, angle=40.0 - 150.0 + 360.0), sc.b(14, angle=40.0)]
    for j in b:
        sc.node([a1], [j])
    others = [sc.case([10], NX_MATCHED, on=0, a_kw=dict(angle=40.0), b_kw={0: dict(angle=40.0)})[0] for _ in range(10)]
    sc.tags["dup_a"] = [a1]; sc.tags["others"] = others
    sc.sequential_only = True


def _dup_a_only(sc):
    """as above without the rotation reject, and nothing else in the call: two first-side features, five pushes"""
    a1 = sc.a(0, NX_MATCHED)
    for d in (10, 12, 14):
        sc.node([a1], [sc.b(d)])
    a2 = sc.a(0, NX_MATCHED)
    for d in (10, 12):
        sc.node([a2], [sc.b(d)])
    sc.tags["dup_a"] = [a1, a2]
    sc.sequential_only = True


# ---- scenes of SearchForInitialization --------------------------------------------------------------------------------------------
def _init_basic(sc):
    """octave above 0, a window outside the grid, an empty window, a window that holds only another level, 49 / 50 / 51 against TH_LOW,
    the ratio test at float equality and to each side"""
    cx, cy = sc.site()
    sc.kp(cx, cy, 0, 10)
    sc.k1(cx, cy, 0, NX_INVALID, octave=1)
    sc.k1(cx, cy, 0, NX_INVALID, octave=7)
    sc.k1(-500.0, 200.0, 0, NX_EMPTY, tag="outside")
    sc.k1(sc.w + 500.0, 200.0, 0, NX_EMPTY, tag="outside")
    sc.k1(600.0, 465.0, 0, NX_EMPTY, tag="empty")
    cx, cy = sc.site()
    sc.kp(cx, cy, 1, 10)
    sc.k1(cx, cy, 0, NX_EMPTY, tag="other_level")
    for d, ex in ((49, NX_MATCHED), (50, NX_MATCHED), (51, NX_TOO_FAR)):
        cx, cy = sc.site()
        k = sc.kp(cx, cy, 0, d)
        sc.k1(cx, cy, 0, ex, on=k, tag=f"dist{d}")
        cx, cy = sc.site()
        k = sc.kp(cx - 1, cy, 0, d); sc.kp(cx + 1, cy, 0, 120)
        sc.k1(cx, cy, 0, ex, on=k, tag=f"dist{d}")
    (b, s), fd = ratio_pairs(sc.nnratio, 50)
    for best, second, ex in ((b, s, NX_RATIO), (b - 1, s, NX_MATCHED), (b + 1, s, NX_RATIO)) + (((fd[0], fd[1], NX_RATIO),) if fd else ()):
        assert best <= 50
        cx, cy = sc.site()
        sc.kp(cx + 1, cy, 0, second); k = sc.kp(cx - 1, cy, 0, best)
        sc.k1(cx, cy, 0, ex, on=k, tag="ratio")
    cx, cy = sc.site()          # equal best distances: rejected by the ratio test
    sc.kp(cx + 1, cy, 0, 20); sc.kp(cx - 1, cy, 0, 20)
    sc.k1(cx, cy, 0, NX_RATIO, tag="best_tie")


def _init_lists(sc):
    """windows of ORBFE_MAX_CAND and ORBFE_MAX_CAND + 1 candidates (the second is enumerated again from the grid): the second-best, in the
    first or the later batch of 64, decides the ratio test; then the best at the last place, and a second keypoint of the first frame
    that finds it kept by a closer match"""
    maxc = npj.kernel_constants()["ORBFE_MAX_CAND"]
    for n in (maxc, maxc + 1):
        for second_at in (5, n - 1):
            cx, cy = sc.site()
            npj._pile(sc, cx, cy, n, lambda j: 11 if j == 3 else 12 if j == second_at else 60 + j % 40, lambda j: 0)
            sc.k1(cx, cy, 0, NX_RATIO, tag=f"pile{n}")                  # 11 against 12 fails at 0.9; against the fill it would pass
        cx, cy = sc.site()
        pile = npj._pile(sc, cx, cy, n, lambda j: 10 if j == n - 1 else 20 if j == 3 else 60 + j % 40, lambda j: 0)
        sc.k1(cx, cy, 0, NX_MATCHED, on=pile[n - 1], tag=f"pile{n}")
        sc.k1(cx, cy, 5, NX_MATCHED, on=pile[3], tag=f"pile{n}")        # 15 from the last one, which is held at 10: kept


def _init_steal(sc):
    """a keypoint of the second frame taken by ever closer keypoints of the first: a chain three steals deep; an equal distance does
    not steal; a thief whose entry falls to the rotation check leaves its victim unmatched"""
    cx, cy = sc.site()
    K = sc.kp(cx, cy, 0, 0, angle=40.0)
    for flips, ex in ((20, NX_STOLEN), (10, NX_STOLEN), (5, NX_STOLEN), (2, NX_MATCHED), (2, NX_ALL_GONE), (3, NX_ALL_GONE)):
        sc.k1(cx, cy, flips, ex, angle=40.0, on=K if ex != NX_ALL_GONE else None, tag="chain")
    for _ in range(11):         # bin 0 holds 11 + 4 entries, so the one entry of bin 5 below falls
        _entry(sc, 40.0, 40.0, NX_MATCHED)
    cx, cy = sc.site()
    K2 = sc.kp(cx, cy, 0, 0, angle=40.0)
    sc.k1(cx, cy, 20, NX_STOLEN, angle=40.0, on=K2, tag="victim")
    sc.k1(cx, cy, 10, NX_ROTATION if sc.check_ori else NX_MATCHED, angle=190.0, on=K2, tag="thief")


def _init_hist_stolen(sc):
    """six matches of bin 0 stolen by six closer ones of bin 0: the histogram holds 12 entries there although 6 matches live, and the
    single match of bin 3 falls (1 < 0.1f * 12) where 6 live entries would have kept it"""
    for _ in range(6):
        cx, cy = sc.site()
        K = sc.kp(cx, cy, 0, 0, angle=40.0)
        sc.k1(cx, cy, 20, NX_STOLEN, angle=40.0, on=K)
        sc.k1(cx, cy, 10, NX_MATCHED, angle=43.0, on=K)
    _entry(sc, 130.0, 40.0, NX_ROTATION if sc.check_ori else NX_MATCHED, tag="lone")


@functools.lru_cache(maxsize=None)
def build_scenes(form):
    """the directed scenes of one form, each walked and checked against the exits it was built for; twins and the scenes that need
    the sequential path included (Scene.sequential_only / a name ending in "+twin")"""
    scenes = []

    def add(name, fn, *args, twin=True, **kw):
        sc = InitScene(name, **kw) if form == "init" else Scene(name, form, **kw)
        fn(sc, *args)
        scenes.append(sc.finish())
        if form != "init" and twin and not sc.sequential_only:
            scenes.append(sc.twin())

    if form in ("frame", "kf"):
        for n in LIST_LENGTHS:
            add(f"lanes_{n}", _lanes, n, nnratio=0.7)
        add("ties", _ties, nnratio=0.7)
        add("thresholds", _thresholds, nnratio=0.7)
        for r in RATIOS:
            add(f"ratio_{r}", _ratio, r, nnratio=r)
        add("chain", _chain, nnratio=0.9)
        add("invalid", _invalid, nnratio=0.7)
        for name, (idsA, idsB) in LAYOUTS.items():
            add(name, _layout, idsA, idsB)
    if form == "tri":
        add("tri_lists", _tri_lists)
        add("tri_disc", _tri_disc)
        add("tri_epipolar", _tri_epipolar)
        add("tri_masks", _tri_masks)
        add("tri_only_stereo", _tri_masks, only_stereo=True)
        add("tri_no_u_right", _tri_disc_mono, with_u_right=False)
        add("tri_zero_F12", _tri_zero, F12=((0.0,) * 3,) * 3)
        for name, (idsA, idsB) in LAYOUTS.items():
            add(name, _layout, idsA, idsB)
    if form == "init":
        add("init_basic", _init_basic)
        add("init_lists", _init_lists)
        add("init_steal", _init_steal)
        add("init_hist_stolen", _init_hist_stolen)
    for name, (counts, kept) in ROTATION_SCENES.items():
        add(name, _rotation, counts, kept)
    add("rot_11_1_off", _rotation, *ROTATION_SCENES["rot_11_1"], check_ori=False)
    add("rot_bounds", _rot_bounds)
    add("rot_empty", _empty_hist)
    if form != "init":
        add("dup_b", _dup_b, nnratio=0.9)
        add("dup_a", _dup_a, nnratio=0.9)
        add("dup_a_only", _dup_a_only, nnratio=0.9)
    return tuple(scenes)


def _tri_disc_mono(sc):
    """mvuRight absent on both sides: every keypoint is monocular, the disc applies to all"""
    sc.case([20, 30], NX_MATCHED, on=1, b_kw={0: dict(x=TRI_EX + 1.0)})
    sc.case([20], NX_ALL_GONE, a_kw=dict(ur=5.0), b_kw={0: dict(x=TRI_EX + 1.0, ur=5.0)})       # the values are not read
    sc.case([20], NX_MATCHED, on=0)


def _tri_zero(sc):
    """F12 == 0: den == 0 for every pair, CheckDistEpipolarLine refuses all"""
    sc.case([20, 30], NX_ALL_GONE)
    sc.case([51], NX_TOO_FAR)


# ---- the census ------------------------------------------------------------------------------------------------------------------------
REACHABLE = {"frame": (NX_UNVISITED, NX_INVALID, NX_EMPTY, NX_ALL_GONE, NX_TOO_FAR, NX_RATIO, NX_MATCHED, NX_ROTATION),
             "kf": (NX_UNVISITED, NX_INVALID, NX_EMPTY, NX_ALL_GONE, NX_TOO_FAR, NX_RATIO, NX_MATCHED, NX_STOLEN, NX_ROTATION),
             "tri": (NX_UNVISITED, NX_INVALID, NX_EMPTY, NX_ALL_GONE, NX_TOO_FAR, NX_MATCHED, NX_STOLEN, NX_ROTATION),
             "init": (NX_INVALID, NX_EMPTY, NX_ALL_GONE, NX_TOO_FAR, NX_RATIO, NX_MATCHED, NX_STOLEN, NX_ROTATION)}


def _half_bin_hits(angle_pairs):
    """how many (angle a, angle b) have rot * (1 / 30.f) exactly on a half"""
    n = 0
    for a, b in angle_pairs:
        rot = _f32(a) - _f32(b)
        if rot < 0:
            rot = rot + _f32(360.0)
        v = rot * (_f32(1.0) / _f32(30))
        n += float(v) % 1.0 == 0.5
    return n


def exit_counts(results, form):
    """results: [(exits, facts)] of the walks of one form (rotation check on).  The rows of the table in this module's docstring."""
    visits = [v for _, f in results for v in f["visits"]]
    allx = np.concatenate([e for e, _ in results] + [np.zeros(0, np.int32)])
    vx = np.array([v["exit"] for v in visits], np.int32)
    out = {EXIT_NAMES[x]: int((vx == x).sum()) + (int((allx == x).sum()) if x == NX_UNVISITED else 0) for x in EXIT_NAMES}
    seen = [v for v in visits if "n_list" in v]
    out["list or window lengths among 1, 63, 64, 65, 128, 129"] = sorted({v["n_list"] for v in seen} & set(LIST_LENGTHS))
    out["best at place >= 64"] = sum(v["best_pos"] >= 64 for v in seen)
    if form != "tri":
        out["second-best from the winner's lane, 64 places on"] = sum(v["second_same_lane"] and v["second_pos"] != v["best_pos"] and
                                                                      abs(v["second_pos"] - v["best_pos"]) >= 64 for v in seen)
        out["second-best equal to the best"] = sum(v["best"] == v["second"] < 256 for v in seen)
        out["single candidate (second-best none)"] = sum(v["n_free"] == 1 for v in seen)
    else:
        out["ties at the winning distance"] = sum(len(v["tie_pos"]) > 1 for v in seen)
        out["... 64 places apart"] = sum(len(v["tie_pos"]) > 1 and v["tie_pos"][-1] - v["tie_pos"][0] >= 64 for v in seen)
        out["candidates per gate (invalid, far, worse, epipole, den, epipolar, passed)"] = [
            sum(g.count(t) for v in visits for g in [v.get("gates", [])]) for t in range(7)]
    out["best distance 49 / 50 / 51"] = [sum(v["best"] == d for v in seen) for d in (49, 50, 51)]
    out["rotation bins hit"] = sorted({v["bin"] for v in visits if v["bin"] >= 0})
    out["calls with an empty histogram"] = sum(sum(f["hist"]) == 0 for _, f in results)
    out["largest pushes of one feature"] = max([int(f["pushes"].max()) for _, f in results if len(f["pushes"])] + [0])
    out["calls with more pushes than first-side features"] = sum(int(f["pushes"].sum()) > len(f["pushes"]) for _, f in results)
    if form in ("frame", "kf"):
        out["longest run of visits that each skip a taken feature"] = _taken_run(results)
    if form == "init":
        out["deepest steal chain"] = max([v["depth"] for v in visits] + [0])
        out["steals refused at equal distance"] = sum(v["n_kept_equal"] for v in visits)
        out["histogram entries of stolen matches"] = sum(f["hist_stolen"] for _, f in results)
        out["windows outside the grid"] = sum(v["outside"] for v in visits)
    return out


def _taken_run(results):
    best = 0
    for _, f in results:
        run, node = 0, None
        for v in f["visits"]:
            if v.get("n_list") and v["node"] == node and v["n_free"] < v["n_list"] and v["exit"] == NX_MATCHED:
                run += 1
            else:
                run = 1 if v.get("n_list") and v["exit"] == NX_MATCHED else 0
            node = v["node"]
            best = max(best, run)
    return best


def census(scenes):
    """scenes: the scenes of one form, walked.  Returns the list of census conditions that do NOT hold."""
    form = scenes[0].form
    missing = []
    res = [(sc,) + tuple(sc.result[-2:]) for sc in scenes]
    c = exit_counts([r[1:] for r in res], form)
    visits = [v for _, _, f in res for v in f["visits"]]
    seen = [v for v in visits if "n_list" in v]
    for x in REACHABLE[form]:
        if c[EXIT_NAMES[x]] < 2:
            missing.append(f"fewer than 2 visits take the exit '{EXIT_NAMES[x]}'")
    for x in set(EXIT_NAMES) - set(REACHABLE[form]):
        if c[EXIT_NAMES[x]]:
            missing.append(f"a visit takes the exit '{EXIT_NAMES[x]}', which the form {form} cannot reach")
    if form != "init":
        if c["list or window lengths among 1, 63, 64, 65, 128, 129"] != sorted(LIST_LENGTHS):
            missing.append("a list length among 1, 63, 64, 65, 128, 129 is missing")
        for n in LIST_LENGTHS:
            if not any(v["n_list"] == n and v["best_pos"] == n - 1 for v in seen) or not any(v["n_list"] == n and v["best_pos"] == 0 for v in seen):
                missing.append(f"no list of {n} with the best first, or none with the best last")
        if not any(sc.name.endswith("+twin") for sc in scenes) or not any(sc.sequential_only for sc in scenes):
            missing.append("no twin, or no scene for the sequential path alone")
        if c["largest pushes of one feature"] < 3 or c["calls with more pushes than first-side features"] < 1:
            missing.append("no feature visited three times with a push each, or no call with more pushes than first-side features")
        if not any(f["dup_b"] for _, _, f in res) and form != "tri":
            missing.append("no second-side feature listed twice")
    if form in ("frame", "kf"):
        pairs = {(v["best_pos"], v["second_pos"]) for v in seen if v["exit"] in (NX_RATIO, NX_MATCHED)}
        for want in ((3, 67), (67, 3), (3, 4), (4, 3)):
            if want not in pairs:
                missing.append(f"best and second-best at places {want} are missing")
        if c["second-best equal to the best"] < 4 or c["single candidate (second-best none)"] < 4:
            missing.append("ties at the best distance or single candidates are missing")
        if not any(v["tie_pos"][:2] == [3, 67] for v in seen) or not any(v["tie_pos"][:2] == [3, 4] for v in seen):
            missing.append("no tie inside one lane (3, 67) or across lanes (3, 4)")
        if c["longest run of visits that each skip a taken feature"] < 65:
            missing.append("no taken-chain of 65 in one node")
        for r in RATIOS:
            tg = next(sc for sc in scenes if sc.name == f"ratio_{r}").tags
            sc_r = next(sc for sc in scenes if sc.name == f"ratio_{r}")
            last = {v["a"]: v for v in sc_r.result[3]["visits"]}
            got = {t: [(last[i]["best"], last[i]["second"], last[i]["exit"]) for i in tg.get(t, [])] for t in ("ratio_eq", "ratio_below", "ratio_above")}
            if not all(len(got[t]) == 1 for t in got):
                missing.append(f"ratio {r}: equality, the step below or the step above is missing")
                continue
            (b, s_, x), (b0, s0, x0), (b1, s1, x1) = got["ratio_eq"][0], got["ratio_below"][0], got["ratio_above"][0]
            if not (_f32(r) * _f32(s_) == _f32(b) and x == NX_RATIO and (b0, s0, x0) == (b - 1, s_, NX_MATCHED) and (b1, s1, x1) == (b + 1, s_, NX_RATIO)):
                missing.append(f"ratio {r}: {got} is not an equality in float32 with one step to each side")
    for d, n in zip((49, 50, 51), c["best distance 49 / 50 / 51"]):
        if form == "tri" and d == 51:
            continue        # a candidate over TH_LOW is never the best of SearchForTriangulation: counted as a gate below
        if n < 1:
            missing.append(f"no best distance {d}")
    if form == "tri":
        g = c["candidates per gate (invalid, far, worse, epipole, den, epipolar, passed)"]
        if min(g) < 2:
            missing.append(f"a gate of SearchForTriangulation removes fewer than 2 candidates: {g}")
        if c["... 64 places apart"] < 2:
            missing.append("no last-wins tie inside one lane")
        tags = set().union(*[set(sc.tags) for sc in scenes])
        for t in ("disc_eq", "disc_l1_in", "disc_l1_out", "disc_float_not_double", "disc_stereo", "epi0_in", "epi0_out", "epi1_in", "epi1_out",
                  "epi_equal", "den0", "tie_gated", "tie_has_mp"):
            if t not in tags:
                missing.append(f"the case {t} is missing")
    if form == "init":
        maxc = npj.kernel_constants()["ORBFE_MAX_CAND"]
        for n in (maxc, maxc + 1):
            if not any(v.get("n_list") == n for v in visits):
                missing.append(f"no window of {n} candidates")
        if c["deepest steal chain"] < 3 or c["steals refused at equal distance"] < 1 or c["histogram entries of stolen matches"] < 6:
            missing.append("the steal chain, the refused steal or the stolen histogram entries are missing")
        if c["windows outside the grid"] < 2:
            missing.append("no window outside the grid")
    if c["rotation bins hit"] != list(range(13)):
        missing.append(f"rotation bins hit: {c['rotation bins hit']}")      # 13 .. 29 cannot be: rot < 360 and the factor is 1 / 30
    if c["calls with an empty histogram"] < 1:
        missing.append("no call with an empty histogram")
    hists = [f["hist"] for sc, _, f in res if sc.check_ori]
    top = lambda h, k: sorted(h, reverse=True)[k]
    if not any(top(h, 0) == top(h, 1) > top(h, 2) for h in hists) or not any(top(h, 0) == top(h, 2) > top(h, 3) for h in hists) or \
            not any(top(h, 0) == top(h, 3) > 0 for h in hists):
        missing.append("a two-way, three-way or four-way tie for the maximum is missing")
    for k in (1, 2):
        if not any(top(h, 0) == 10 and top(h, k) == 1 for h in hists) or not any(top(h, 0) == 11 and top(h, k) == 1 for h in hists):
            missing.append(f"10 against 1 or 11 against 1 is missing for maximum {k + 1}")
    if not any(sum(x > 0 for x in h) == 1 for h in hists):
        missing.append("no histogram with one bin")
    bounds = next(sc for sc in scenes if sc.name == "rot_bounds")
    ang = ([(a["angle"], b["angle"]) for a, b in zip(bounds.A, bounds.B)] if form != "init" else
           list(zip(bounds.keys1["angle"], bounds.keys["angle"])))
    if _half_bin_hits(ang) < 6:
        missing.append("fewer than 6 angle differences sit exactly on a half bin")
    if not any(_f32(a) - _f32(b) < 0 and (_f32(a) - _f32(b)) + _f32(360.0) == _f32(360.0) for a, b in ang):
        missing.append("no negative difference that rounds up to 360")
    return missing


# ---- the inputs of the undirected tests, for the table ---------------------------------------------------------------------------------
def previous_inputs(form):
    """(exits, facts) of the walk on what tests/test_matcher_gpu.py feeds the search of this form (see the module docstring), rebuilt with
    the C oracle's extractor"""
    from refactored_orb_slam2_amd import synth
    from tests import oracle_lib as ol
    w, h, nf = 640, 480, 1000
    a, b = synth.sequence(w, h, 2, seq=1)
    orc = ol.OracleExtractor(nf, 1.2, 8, 20, 7)
    (k0, d0), (k1, d1) = orc(a), orc(b)
    sf = np.array([np.float32(1.2) ** i for i in range(8)], np.float32)
    grp = lambda desc: {k: [i for i, d in enumerate(desc) if int(d[1]) % 24 == k] for k in set(int(d[1]) % 24 for d in desc)}
    if form in ("frame", "kf"):
        rng = np.random.default_rng(31)
        valid = (rng.random(len(k0)) < 0.8).astype(np.uint8)
        validB = (rng.random(len(k1)) < 0.8).astype(np.uint8)
        return nr.bow_walk(d0, k0["angle"], valid, grp(d0), d1, k1["angle"], validB, grp(d1), 0.7, True, form == "kf")[2:]
    if form == "tri":
        rng = np.random.default_rng(41)
        F12 = (np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32) * np.float32(0.37)).reshape(3, 3)
        urA = np.where(rng.random(len(k0)) < 0.5, k0["x"] - np.float32(20), -1).astype(np.float32)
        urB = np.where(rng.random(len(k1)) < 0.5, k1["x"] - np.float32(20), -1).astype(np.float32)
        hasA = (rng.random(len(k0)) < 0.3).astype(np.uint8); hasB = (rng.random(len(k1)) < 0.3).astype(np.uint8)
        return nr.tri_walk(k0, d0, urA, hasA, grp(d0), k1, d1, urB, hasB, grp(d1), F12, 9000.0, 240.0, sf, (sf * sf).astype(np.float32),
                           False, True)[2:]
    F2 = nr.RefFrame(k1, d1, 0, w, 0, h)
    prev = np.stack([k0["x"], k0["y"]], 1)
    return nr.init_walk(k0, d0, F2, prev, 30, 0.9, True)[3:]
