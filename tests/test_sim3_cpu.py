"""CPU suite of the Sim3Solver: the numpy reading of tests/np_sim3.py against a noise-free scene, the conditions that make the GPU
comparison meaningful (margins, R32 == R64 on parity decisions, coverage) ASSERTED on the whole case list, the arithmetic of
csrc/sim3_internal.h compiled for the host against the reading, the pure-host pieces (orbfe_sim3_ransac_iterations, draw_triples,
iterate_replay) and the C ABI without a device: struct sizes, exports, every validation boundary on both sides, ORBFE_ERR_NO_DEVICE
from both solve entry points."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, sim3
from tests import np_sim3 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_sim3", "_build", "libsim3_host.so")
NON_PARITY_CAP = 0.03


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in S.CASES:
        s = S.case_scene(name)
        out[name] = (s, S.run(s, "R64"), S.run(s, "R32"))
    return out


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_struct_sizes_and_exports(L):
    assert _lib.SIM3_VIEW_DTYPE.itemsize == 64 and _lib.SIM3_PAIR_DTYPE.itemsize == 32
    assert _lib.SIM3_HYPOTHESIS_DTYPE.itemsize == 64 and _lib.SIM3_RESULT_DTYPE.itemsize == 128
    assert S.VIEW_DTYPE == _lib.SIM3_VIEW_DTYPE and S.PAIR_DTYPE == _lib.SIM3_PAIR_DTYPE
    assert _lib.SIM3_HYPOTHESIS_DTYPE.fields["n_inliers"][1] == 52 and _lib.SIM3_RESULT_DTYPE.fields["T12"][1] == 16
    assert _lib.SIM3_RESULT_DTYPE.fields["s"][1] == 64
    for sym in ("orbfe_sim3_ransac_iterations", "orbfe_sim3_solve", "orbfe_sim3_solve_batch_device"):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for text in ("} orbfe_sim3_view;", "} orbfe_sim3_pair;", "/* 32 bytes */", "} orbfe_sim3_hypothesis;", "} orbfe_sim3_result;",
                 "/* 128 bytes */", f"#define ORBFE_SIM3_MAX_PAIRS {_lib.SIM3_MAX_PAIRS}",
                 f"#define ORBFE_SIM3_MAX_HYPOTHESES {_lib.SIM3_MAX_HYPOTHESES}"):
        assert text in hdr, text
    internal = open(os.path.join(ROOT, "refactored_orb_slam2_amd", "csrc", "sim3_internal.h")).read()
    assert f"#define SIM3_WAVES {_lib.SIM3_WAVES} " in internal


# ---- orbfe_sim3_ransac_iterations ----------------------------------------------------------------------------------------------------
def _closed_form(N, p, m, max_its):
    """SetRansacParameters (:123-133) written out: epsilon is a float, pow / log are double"""
    if m == N:
        return max(1, min(1, max_its))
    eps = float(np.float32(m) / np.float32(N))
    return max(1, min(int(math.ceil(math.log(1 - p) / math.log(1 - eps ** 3))), max_its))


def test_ransac_iterations_against_the_closed_form(L):
    f = L.orbfe_sim3_ransac_iterations
    assert f(20, 0.99, 20, 300) == 1 and f(7, 0.5, 7, 0) == 1                       # N == minInliers; max(1, .)
    for N in (21, 40, 100, 1000):
        want = _closed_form(N, 0.99, 20, 300)
        assert f(N, 0.99, 20, 300) == want, N
    assert _closed_form(21, 0.99, 20, 300) == 3 and _closed_form(40, 0.99, 20, 300) == 35      # ceil(4.6 / 1.99), ceil(4.6 / 0.1335)
    assert f(100, 0.99, 20, 300) == 300 and f(1000, 0.99, 20, 300) == 300           # 574 and 575 644 before the clamp
    assert f(100, 0.99, 20, 1000) == _closed_form(100, 0.99, 20, 1000) == 574
    assert f(100, 0.99, 20, 5) == 5 and f(100, 0.99, 0, 300) == 1                    # the clamp; epsilon 0: -inf, max(1, .)
    assert sim3.ransac_iterations(40, 0.99, 20, 300) == 35
    for bad in ((0, 0.99, 0, 300), (10, 0.99, -1, 300), (10, 0.99, 11, 300), (10, 0.99, 5, -1), (10, 0.0, 5, 300), (10, 1.0, 5, 300),
                (10, float("nan"), 5, 300)):
        assert f(*bad) == _lib.ERR_INVALID, bad
    with pytest.raises(_lib.OrbfeError):
        sim3.ransac_iterations(10, 0.99, 11, 300)


# ---- the reading -------------------------------------------------------------------------------------------------------------------
def test_noise_free_scene_returns_the_true_similarity():
    """Without noise the only errors are the roundings to float of what the ABI carries: the world positions, nine rotation entries
    and the translation of each pose, so a camera-frame point is off by at most delta = 8 x 2^-24 x the largest coordinate (three
    inputs, the three products of a row, each relative 2^-24, doubled for slack).  Horn's rotation from three points turns with the
    triangle: an in-plane displacement delta of a vertex turns it by delta / sigma2, sigma2 = the smaller non-zero singular value of
    the centred triple (its extent across its thin direction), and both triangles move.  The bounds asserted for R64 on parity
    hypotheses: |R - R*|_F <= 8 delta / sigma2, |s - s*| / s* <= 8 delta / sigma2, |t - t*| <= 8 delta (1 + s |O2| / sigma2) (the rotation
    error times the lever arm of the centroid).  R32 computes in float: its delta is 64 x 2^-24 x the largest coordinate (camera-frame
    points, centroid, Pr, M and P3 each round at the size of the uncentred coordinates), and the float eigenvector adds 2^-22 /
    gap to the rotation (perturbation of an eigenvector: eps x |N| / gap, times two for the angle)."""
    for fix, scale in ((True, 1.0), (False, 1.31)):
        sc = S.make_scene(31, H=200, fix_scale=fix, true_scale=scale, noise=False, outliers=0.0)
        s_true, R_true, t_true = sc["truth"]
        truth = dict(s=np.full(200, s_true), R=np.broadcast_to(R_true, (200, 3, 3)), t=np.broadcast_to(t_true, (200, 3)))
        for mode, k in (("R64", 8.0), ("R32", 64.0)):
            r = S.run(sc, mode)
            ref = S.run(sc, "R64")
            ph = ref["parity_h"]
            assert ph.sum() >= 190
            big = max(np.abs(sc["pairs"]["Xw1"]).max(), np.abs(sc["pairs"]["Xw2"]).max(), 60.0)
            delta = k * 2.0 ** -24 * big
            sig2 = np.linalg.svd(ref["Pr1"], compute_uv=False)[:, 1]
            lever = s_true * np.linalg.norm(ref["O2"], axis=1)
            extra = 2.0 ** -22 / ref["gap"] if mode == "R32" else 0.0
            e_s = np.abs(r["s"].astype(np.float64) - s_true) / s_true
            e_R = np.sqrt(((r["R"].astype(np.float64) - R_true) ** 2).sum((1, 2)))
            e_t = np.linalg.norm(r["t"].astype(np.float64) - t_true, axis=1)
            b_R = 8 * delta / sig2 + extra
            b_t = 8 * delta * (1 + lever / sig2) + extra * lever
            print(f"noise-free fix={fix} {mode}: worst error / bound: R {np.max(e_R[ph] / b_R[ph]):.3f} s {np.max(e_s[ph] / b_R[ph]):.3f} "
                  f"t {np.max(e_t[ph] / b_t[ph]):.3f}")
            assert (e_R[ph] <= b_R[ph]).all() and (e_s[ph] <= b_R[ph]).all() and (e_t[ph] <= b_t[ph]).all()
            assert (r["count"][ph] == 130).all()                            # every correspondence is an inlier of every good hypothesis
        del truth


def test_case_list_margins_stability_and_coverage(runs):
    """What makes the GPU comparison meaningful, on the yardstick alone: few decisions and few hypotheses are too close to call, the
    float reading takes the decisions of the double one on all the others, every case keeps 50 hypotheses to compare, and the case
    list reaches a return at position 0, one behind it and no return at all."""
    returned = []
    for name, (s, r64, r32) in runs.items():
        par, par_h = r64["parity"], r64["parity_h"]
        ret, best = S.select(r32["count"], s["min_inliers"])
        print(f"{name}: non-parity decisions {100 * (~par).mean():.2f} %, hypotheses {100 * (~par_h).mean():.2f} %, R32 returned {ret} "
              f"best {best}, counts up to {r32['count'].max()}, smallest |imag q| {r64['imag'].min():.3g}")
        assert np.array_equal(r32["inl"][par], r64["inl"][par])
        assert (~par).mean() <= NON_PARITY_CAP and (~par_h).mean() <= NON_PARITY_CAP
        assert par_h.sum() >= 50
        assert S.select(r64["count"], s["min_inliers"]) == (ret, best)
        returned.append(ret)
    assert any(r == -1 for r in returned) and any(r >= 0 for r in returned) and any(r > 0 for r in returned)
    assert S.NON_PARITY_CAP == NON_PARITY_CAP and (S.EIG_GAP, S.ERR_MARGIN) == (1e-3, 1e-2)
    assert runs["small_rotation"][1]["imag"].min() < 5e-3                     # the atan2 form near its singular end, not on it
    assert len(S.case_scene("twelve_levels")["pairs"]) and S.CASES["twelve_levels"]["n_levels"] == 12
    assert S.bounds(np.array([0, 1, 7, 11]), 12).tolist() == [9.0, 13.0, 118.0, 508.0]     # floor(9.21 * 1.2^(2 * octave))


def test_select_reading():
    assert S.select([], 20) == (-1, -1)
    assert S.select([0, 0, 0], 20) == (-1, 2)                                 # `>=` from mnBestInliers = 0: the last zero
    assert S.select([3, 7, 7, 2], 20) == (-1, 2)
    assert S.select([3, 20, 21, 50], 20) == (2, 2)                            # == min_inliers does not return; the first above does
    assert S.select([25, 50], 20) == (0, 0)


# ---- csrc/sim3_internal.h on the host -------------------------------------------------------------------------------------------------
def _host_lib():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_sim3"), "_build/libsim3_host.so"], check=True, capture_output=True)
    H = C.CDLL(HOST_LIB)
    vp, ci = C.c_void_p, C.c_int
    H.sim3_host_solve.argtypes = [vp, vp, vp, ci, vp, ci, ci, vp, vp]
    H.sim3_host_solve.restype = None
    return H


def host_solve(scene):
    H = _host_lib()
    n, nh = len(scene["pairs"]), len(scene["triples"])
    hyps, words = np.zeros(nh, _lib.SIM3_HYPOTHESIS_DTYPE), np.zeros((nh, (n + 63) // 64), np.uint64)
    H.sim3_host_solve(_lib.ptr(scene["view1"]), _lib.ptr(scene["view2"]), _lib.ptr(scene["pairs"]), n, _lib.ptr(scene["triples"]), nh,
                      int(scene["fix_scale"]), _lib.ptr(hyps), _lib.ptr(words))
    return hyps, words


@pytest.mark.parametrize("name", list(S.CASES))
def test_host_arithmetic_against_the_reading(runs, name):
    """csrc/sim3_internal.h is host- and device-callable; compiled for the host with the library's flags it must already meet the
    criteria the kernel is held to on the GPU."""
    s, r64, r32 = runs[name]
    hyps, words = host_solve(s)
    S.check_against_yardstick(name, s, r64, r32, hyps, words)


def test_host_arithmetic_degenerate_triples_stay_local():
    """Collinear points and two identical points: whatever these hypotheses hold, they have few or no inliers, nothing traps and
    the other hypotheses are unchanged."""
    s = S.case_scene("fixed_stereo")
    base, _ = host_solve(s)
    p = s["pairs"].copy()
    c = np.array([1.0, 0.5, 20.0])
    for k, i in enumerate((0, 1, 2)):                                         # three collinear points, the same in both maps
        p["Xw1"][i] = p["Xw2"][i] = c + k * np.array([1.0, 0.2, 0.5])
    p["Xw1"][4], p["Xw2"][4] = p["Xw1"][3], p["Xw2"][3]                      # two indices, one point
    tr = s["triples"].copy()
    tr[10], tr[11] = (0, 1, 2), (3, 4, 5)
    hyps, words = host_solve({**s, "pairs": p, "triples": tr})
    keep = np.ones(len(tr), bool)
    keep[[10, 11]] = False
    untouched = ~np.isin(tr, (0, 1, 2, 3, 4)).any(1) & keep
    assert untouched.sum() > 40
    for f in ("s", "R", "t"):
        assert np.array_equal(hyps[f][untouched], base[f][untouched])
    assert np.isfinite(hyps["R"][keep]).all()
    assert (hyps["n_inliers"] >= 0).all() and (hyps["n_inliers"] <= len(p)).all()


# ---- draw_triples and iterate_replay -------------------------------------------------------------------------------------------------
def test_draw_triples_swap_with_back_order():
    script = iter([0, 0, 0, 4, 3, 0, 2, 2, 2])
    got = sim3.draw_triples(5, 3, lambda k: next(script))
    # [0 1 2 3 4]: r = 0 takes 0, slot 0 <- 4: [4 1 2 3]; r = 0 takes 4, slot 0 <- 3: [3 1 2]; r = 0 takes 3
    # r = 4 takes 4: [0 1 2 3]; r = 3 takes 3: [0 1 2]; r = 0 takes 0
    # r = 2 takes 2, slot 2 <- 4: [0 1 4 3]; r = 2 takes 4, slot 2 <- 3: [0 1 3]; r = 2 takes 3
    assert got.tolist() == [[0, 4, 3], [4, 3, 0], [2, 4, 3]] and got.dtype == np.int32
    seen = []

    def rec(k):
        seen.append(k)
        return k - 1
    sim3.draw_triples(7, 2, rec)
    assert seen == [7, 6, 5, 7, 6, 5]                                          # RandomInt(0, size - 1) on a list that shrinks
    t = sim3.draw_triples(3, 200, np.random.default_rng(5))
    assert (np.sort(t, 1) == [0, 1, 2]).all()                                  # n == 3: always a permutation of all three
    t = sim3.draw_triples(40, 500, np.random.default_rng(6))
    assert t.min() == 0 and t.max() == 39
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    with pytest.raises(ValueError):
        sim3.draw_triples(2, 1, np.random.default_rng(0))
    with pytest.raises(ValueError):
        sim3.draw_triples(5, 1, lambda k: k)


def _sequential(counts, min_inliers, chunk, max_its):
    """Sim3Solver::iterate called until bNoMore, as the reference's loop reads (:155-199)"""
    it, calls = 0, []
    while True:
        cur, ret, n_in = 0, -1, 0
        while it < max_its and cur < chunk:
            cur += 1
            it += 1
            if counts[it - 1] > min_inliers:
                ret, n_in = it - 1, counts[it - 1]
                break
        no_more = ret < 0 and it >= max_its
        calls.append((ret, n_in, no_more, it))
        if no_more:
            return calls


def test_iterate_replay_is_the_sequential_loop():
    rng = np.random.default_rng(9)
    for H in (1, 5, 10, 13, 64):                                               # multiples of the chunk and not
        for _ in range(20):
            counts = rng.integers(0, 30, H).tolist()
            for chunk in (1, 5, H, H + 3):
                assert sim3.iterate_replay(counts, 20, chunk) == _sequential(counts, 20, chunk, H)
    # bNoMore arrives with the call that consumes the last iteration, not one later
    assert sim3.iterate_replay([1] * 10, 20, 5) == [(-1, 0, False, 5), (-1, 0, True, 10)]
    assert sim3.iterate_replay([1] * 12, 20, 5) == [(-1, 0, False, 5), (-1, 0, False, 10), (-1, 0, True, 12)]
    # a return in the middle of a chunk; the next call continues behind it; == min_inliers is not a return
    assert sim3.iterate_replay([0, 20, 25, 0, 0, 0, 30, 0], 20, 5) == [(2, 25, False, 3), (6, 30, False, 7), (-1, 0, True, 8)]
    # a return on the very last iteration leaves bNoMore to the next call
    assert sim3.iterate_replay([0, 0, 21], 20, 5) == [(2, 21, False, 3), (-1, 0, True, 3)]
    # mRansacMaxIts below the evaluated hypotheses: the rest is never served
    assert sim3.iterate_replay([0, 0, 0, 50], 20, 2, max_iterations=3) == [(-1, 0, False, 2), (-1, 0, True, 3)]
    with pytest.raises(ValueError):
        sim3.iterate_replay([0], 20, 5, max_iterations=2)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
def _solve(L, n=6, H=2, min_inliers=3, triples=None, null=None, hyps=True, words=True):
    v1, v2 = S.make_view(np.eye(3), np.zeros(3)), S.make_view(np.eye(3), [0, 0, 1.0])
    a, b = max(n, 1), max(H, 1)
    pairs = np.zeros(a, _lib.SIM3_PAIR_DTYPE)
    pairs["Xw1"] = pairs["Xw2"] = np.arange(3 * a).reshape(a, 3) % 7 + 5.0
    pairs["max_err1"] = pairs["max_err2"] = 9
    tr = np.tile(np.array([0, 1, 2], np.int32), (b, 1)) if triples is None else np.asarray(triples, np.int32).reshape(-1, 3)
    nw = (a + 63) // 64
    hy, wd = np.zeros(b, _lib.SIM3_HYPOTHESIS_DTYPE), np.zeros((b, nw), np.uint64)
    res, mask = np.zeros(1, _lib.SIM3_RESULT_DTYPE), np.zeros(nw, np.uint64)
    args = dict(view1=v1, view2=v2, pairs=pairs, triples=tr, result=res, mask=mask)
    if null:
        args[null] = None
    g = lambda k: _lib.ptr(args[k])
    return L.orbfe_sim3_solve(g("view1"), g("view2"), g("pairs"), n, g("triples"), H, 0, min_inliers, _lib.ptr(hy) if hyps else None,
                              _lib.ptr(wd) if words else None, g("result"), g("mask"))


def test_sim3_solve_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    assert _solve(L) == good
    assert _solve(L, n=-1, H=0) == _lib.ERR_INVALID and _solve(L, n=0, H=0) == good
    assert _solve(L, n=_lib.SIM3_MAX_PAIRS) == good and _solve(L, n=_lib.SIM3_MAX_PAIRS + 1) == _lib.ERR_INVALID
    assert _solve(L, H=-1) == _lib.ERR_INVALID and _solve(L, H=0) == good
    assert _solve(L, H=_lib.SIM3_MAX_HYPOTHESES) == good and _solve(L, H=_lib.SIM3_MAX_HYPOTHESES + 1) == _lib.ERR_INVALID
    assert _solve(L, min_inliers=-1) == _lib.ERR_INVALID and _solve(L, min_inliers=0) == good
    assert _solve(L, n=2, H=0) == good and _solve(L, n=5, H=0, min_inliers=6) == good      # nothing to evaluate is not an error
    for tr in ([[0, 1, 6]], [[-1, 1, 2]], [[0, 0, 2]], [[0, 1, 0]], [[3, 1, 1]]):        # outside [0, n), repeated
        assert _solve(L, H=1, triples=tr) == _lib.ERR_INVALID, tr
    assert _solve(L, H=1, triples=[[5, 0, 3]]) == good
    assert _solve(L, n=2, H=1, triples=[[0, 1, 2]]) == _lib.ERR_INVALID                     # n < 3 has no valid triple at all
    for null in ("view1", "view2", "pairs", "triples", "result", "mask"):
        assert _solve(L, null=null) == _lib.ERR_INVALID, null
    assert _solve(L, n=0, H=0, null="pairs") == good and _solve(L, H=0, null="triples") == good
    assert _solve(L, hyps=False, words=False) == good                                       # the optional outputs


def _batch(L, P=0, cap=8, h_cap=8, null=None, misalign=None):
    """Nothing is launched for P == 0, so the pointers only have to look like device pointers."""
    names = ["view1", "view2", "pairs", "n", "triples", "H", "fix", "min", "hyps", "words", "result", "mask"]
    ptrs = {k: 0x10000 + 0x1000 * i for i, k in enumerate(names)}
    if null:
        ptrs[null] = 0
    if misalign:
        ptrs[misalign[0]] += misalign[1]
    a = [C.c_void_p(ptrs[k] or None) for k in names]
    return L.orbfe_sim3_solve_batch_device(P, a[0], a[1], a[2], a[3], cap, a[4], a[5], h_cap, a[6], a[7], a[8], a[9], a[10], a[11], None)


def test_sim3_batch_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    assert _batch(L) == good
    assert _batch(L, P=-1) == _lib.ERR_INVALID and _batch(L, P=_lib.SIM3_MAX_PROBLEMS + 1) == _lib.ERR_INVALID
    assert _batch(L, cap=0) == _lib.ERR_INVALID and _batch(L, cap=1) == good
    assert _batch(L, cap=_lib.SIM3_MAX_PAIRS) == good and _batch(L, cap=_lib.SIM3_MAX_PAIRS + 1) == _lib.ERR_INVALID
    assert _batch(L, h_cap=0) == _lib.ERR_INVALID and _batch(L, h_cap=1) == good
    assert _batch(L, h_cap=_lib.SIM3_MAX_HYPOTHESES) == good and _batch(L, h_cap=_lib.SIM3_MAX_HYPOTHESES + 1) == _lib.ERR_INVALID
    for k in ("view1", "view2", "pairs", "n", "triples", "H", "fix", "min", "hyps", "words", "result", "mask"):
        assert _batch(L, null=k) == _lib.ERR_INVALID, k
        assert _batch(L, misalign=(k, 2)) == _lib.ERR_INVALID, k
    assert _batch(L, misalign=("words", 4)) == _lib.ERR_INVALID and _batch(L, misalign=("mask", 4)) == _lib.ERR_INVALID
    assert _batch(L, misalign=("hyps", 4)) == good


def test_no_device_is_an_error_not_a_fallback(L):
    """Through the Python mirror: without a device the host form raises ORBFE_ERR_NO_DEVICE (with one it simply runs)."""
    s = S.case_scene("fixed_stereo", n=30, H=8)
    args = (s["view1"], s["view2"], s["pairs"], s["triples"], s["fix_scale"], 5)
    if _gpu_present(L):
        assert len(sim3.sim3_solve(*args)[2]) == 8
        return
    with pytest.raises(_lib.OrbfeError) as e:
        sim3.sim3_solve(*args)
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    assert _batch(L, P=1) == _lib.ERR_NO_DEVICE
