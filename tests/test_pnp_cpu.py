"""PnPsolver without a device: SetRansacParameters against a literal reading, the draws, iterate_replay on engineered sequences, the
host build of csrc/pnp_internal.h (tests/cpp_pnp/host_arith.cpp) against the numpy yardstick (tests/np_pnp.py) on every case, the
non-parity cap of the cases under the reading alone, and the C ABI: struct sizes, exports, every validation boundary,
ORBFE_ERR_NO_DEVICE from both solve entry points."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, pnp
from tests import np_pnp as Y
from tests import pnp_host

LIVE = [c for c in Y.CASES if c != "too_few"]


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_struct_sizes_and_exports(L):
    assert (_lib.PNP_POINT_DTYPE.itemsize, _lib.PNP_CAMERA_DTYPE.itemsize, _lib.PNP_HYPOTHESIS_DTYPE.itemsize, _lib.PNP_REFINE_DTYPE.itemsize,
            _lib.PNP_RESULT_DTYPE.itemsize, _lib.PNP_DIAG_DTYPE.itemsize) == (24, 16, 112, 112, 80, 640)
    for s in ("orbfe_pnp_ransac_parameters", "orbfe_pnp_solve", "orbfe_pnp_solve_batch_device"):
        assert s in _lib.EXPORTS and hasattr(L, s)
    assert Y.POINT_DTYPE == _lib.PNP_POINT_DTYPE


def test_ransac_parameters_against_the_literal_reading(L):
    assert pnp.ransac_parameters(60, 0.99, 10, 300, 4, 0.5) == (30, 35, np.float32(0.5))          # Tracking.cc:1262 with N >= 20
    assert pnp.ransac_parameters(20, 0.99, 10, 300, 4, 0.5)[:2] == (10, 35)
    assert pnp.ransac_parameters(10, 0.99, 10, 300, 4, 0.5)[:2] == (10, 1)                          # nMinInliers == N
    assert pnp.ransac_parameters(3, 0.99, 0, 300, 4, 0.5)[0] == 4                                   # min_set is a floor
    seen_edges = 0
    for N in list(range(1, 41)) + [59, 60, 61, 100, 127, 128, 500, 1024]:
        for eps in (0.0, 0.1, 0.3, 0.4, 0.5, 0.6, 0.7, 0.9, 1.0):
            for mi in (0, 4, 8, 10, 20):
                for mx in (0, 1, 35, 300):
                    got = pnp.ransac_parameters(N, 0.99, mi, mx, 4, eps)
                    want = Y.ransac_parameters(N, 0.99, mi, mx, 4, eps)
                    assert got[:2] == want[:2] and got[2].tobytes() == want[2].tobytes(), (N, eps, mi, mx, got, want)
                    seen_edges += int(np.float32(N) * np.float32(eps)) != int(N * float(np.float32(eps)))   # a double product would truncate lower
    assert seen_edges > 0
    for p in (0.5, 0.9, 0.999):
        assert pnp.ransac_parameters(77, p, 8, 300, 4, 0.4) == Y.ransac_parameters(77, p, 8, 300, 4, 0.4)
    bad = [(0, 0.99, 8, 300, 4, 0.4), (10, 0.0, 8, 300, 4, 0.4), (10, 1.0, 8, 300, 4, 0.4), (10, 0.99, -1, 300, 4, 0.4),
           (10, 0.99, 8, -1, 4, 0.4), (10, 0.99, 8, 300, 3, 0.4), (10, 0.99, 8, 300, 5, 0.4), (10, 0.99, 8, 300, 4, -0.1),
           (10, 0.99, 8, 300, 4, 1.5), (10, 0.99, 8, 300, 4, float("nan"))]
    for a in bad:
        with pytest.raises(_lib.OrbfeError) as e:
            pnp.ransac_parameters(*a)
        assert e.value.code == _lib.ERR_INVALID
    out = C.c_int32(0)
    assert L.orbfe_pnp_ransac_parameters(10, 0.99, 8, 300, 4, 0.4, None, C.byref(out), C.byref(out)) == _lib.ERR_INVALID


def test_draw_minimal_sets_is_the_list_walk():
    for n, H, seed in ((4, 9, 1), (5, 30, 2), (60, 35, 3), (1024, 12, 4)):
        a = pnp.draw_minimal_sets(n, H, np.random.default_rng(seed))
        r = np.random.default_rng(seed)
        b = Y.draw_sets_literal(n, H, lambda k: int(r.integers(k)))
        assert a.dtype == np.int32 and a.shape == (H, 4) and np.array_equal(a, b)
        assert all(len(set(row)) == 4 for row in a.tolist()) and a.min() >= 0 and a.max() < n
    seq = iter([0, 0, 0, 0, 5, 4, 3, 2])                 # the swap with the back: 0, then 5 (moved to 0), then 4, 3; then 5, 4, 3, 2
    assert pnp.draw_minimal_sets(6, 2, lambda k: next(seq)).tolist() == [[0, 5, 4, 3], [5, 4, 3, 2]]
    with pytest.raises(ValueError):
        pnp.draw_minimal_sets(3, 1, np.random.default_rng(0))
    with pytest.raises(ValueError):
        pnp.draw_minimal_sets(6, 1, lambda k: k)


def test_iterate_replay_on_engineered_sequences():
    IC = pnp.IterateCall
    # the loop condition is an OR: the first iterate(5) runs until mnIterations reaches mRansacMaxIts
    assert pnp.iterate_replay([0] * 35, [0] * 35, 10, 5, 35) == [IC(-1, -1, 0, True, 35)]
    assert pnp.iterate_replay([9] * 40, [99] * 40, 10, 5, 35) == [IC(-1, -1, 0, True, 35)]        # 9 < min_inliers never qualifies
    # >= qualifies, only > makes a new best; the refine runs on the best in either case
    c, r = [10, 10, 12, 30], [10, 77, 11, 99]
    calls = pnp.iterate_replay(c + [0] * 5, r + [0] * 5, 10, 5, 4)
    assert calls[0] == IC(2, 2, 11, False, 3) and calls[1] == IC(3, 3, 99, False, 4) and calls[2] == IC(3, -1, 30, True, 9)
    # a refine of exactly min_inliers fails (strict >), and the equal count at 1 re-runs the refine of 0, not its own
    assert pnp.iterate_replay([10, 10, 0], [10, 99, 0], 10, 3, 3) == [IC(0, -1, 10, True, 3)]
    # after a returning call a later qualifying hypothesis returns the same refine again; beyond mRansacMaxIts a call runs `chunk`
    c, r = [0, 15, 0, 12, 0, 0, 0, 0], [0, 14, 0, 99, 0, 0, 0, 0]
    assert pnp.iterate_replay(c, r, 10, 2, 4) == [IC(1, 1, 14, False, 2), IC(3, 1, 14, False, 4), IC(1, -1, 15, True, 6)]
    # exhaustion with a best whose refine failed, and without one
    assert pnp.iterate_replay([0, 10, 0], [0, 10, 0], 10, 3, 3) == [IC(1, -1, 10, True, 3)]
    assert pnp.iterate_replay([0, 10, 0, 0, 0], [0, 10, 0, 0, 0], 10, 5, 3) == [IC(1, -1, 10, True, 5)]   # iterate(5) runs five even then
    assert pnp.iterate_replay([3, 9, 0], [50, 50, 50], 10, 1, 3) == [IC(-1, -1, 0, True, 3)]
    # the walk past the evaluated hypotheses
    with pytest.raises(IndexError):
        pnp.iterate_replay([0, 0, 0, 15], [0, 0, 0, 14], 10, 2, 4)
    with pytest.raises(IndexError):
        pnp.iterate_replay([0] * 3, [0] * 3, 10, 5, 4)
    # find() is the first call with chunk == max_iterations, and it is the yardstick's rule
    rng = np.random.default_rng(5)
    for _ in range(200):
        c, r = rng.integers(0, 16, 12), rng.integers(8, 14, 12)
        first = pnp.iterate_replay(list(c) + [0] * 12, list(r) + [0] * 12, 10, 12, 12)[0]
        ret, refined, best, bc = Y.find_rule(c, r, 10)
        assert (first.returned, first.refine >= 0) == (ret, refined) and (not refined or first.refine == best)
        assert first.n_inliers == (r[best] if refined else bc)


def test_prefix_maxima_and_find_rule():
    assert Y.prefix_maxima([0, 10, 10, 9, 12, 12, 30], 10) == [1, 4, 6]
    assert Y.prefix_maxima([11, 5, 10], 10) == [0] and Y.prefix_maxima([5, 9], 10) == []
    assert Y.find_rule([0, 10, 12], [0, 10, 10], 10) == (2, False, 2, 12)
    assert Y.find_rule([0, 10, 12, 11], [0, 10, 11, 0], 10) == (2, True, 2, 12)


@pytest.mark.parametrize("name", Y.CASES)
def test_host_arithmetic_against_the_yardstick(name):
    case = pnp_host.case(name)
    sol = pnp_host.host_solve(case["cam"], case["points"], case["sets"], case["min_inliers"])
    fig = Y.check_against_yardstick(case, sol)
    for k, v in fig.items():
        print(f"  {name}: {k} = {v}")
    res = sol.result
    if name == "kitti":
        assert len(case["sets"]) == 35 and case["min_inliers"] == 30 and res["refined"] == 1 and res["n_inliers"] > 35
    elif name == "single_iteration":
        assert len(case["sets"]) == 1 and case["min_inliers"] == len(case["points"])
    elif name == "too_few":
        assert res["returned"] == -1 and not sol.hyps["n_inliers"].any()
    elif name == "best_at_exhaustion":
        assert res["refined"] == 0 and res["returned"] == res["best"] == 2 and res["n_inliers"] == 10 and not sol.refines["success"].any()
    elif name == "second_best_refines":
        assert sol.hyps["refine"][0] == 0 and sol.refines["success"][0] == 0 and sol.refines["n_inliers"][0] == 20
        assert res["returned"] > 0 and res["refined"] == 1 and res["best_inliers"] > 20
    elif name == "degenerate_sets":
        for h in case["planted"]:
            assert sol.hyps["n_inliers"][h] == 0 and not sol.words[h].any()
    # the truth of the scene: the returned pose is the camera's
    if res["refined"]:
        R, t = case["truth"]
        T = res["Tcw"].reshape(3, 4)
        assert np.abs(T[:, :3] - R).max() < 2e-2 and np.abs(T[:, 3] - t).max() < 0.3


@pytest.mark.parametrize("name", LIVE)
def test_non_parity_cap_under_the_reading_alone(name):
    """The cap is a condition on the scenes: with LAPACK's own conventions, at most NON_PARITY_CAP of a case's solves (hypotheses and
    the refines of the reading's own best-so-far hypotheses) and of its decisions are outside the margins."""
    case = pnp_host.case(name)
    cam, pts = case["cam"], case["points"]
    sl = [list(map(int, s)) for s in case["sets"]]
    vd = Y.verdicts(cam, pts, sl, Y.lapack_conventions(cam, pts, sl))
    solves, bad, dec, dec_bad = len(sl), int((~vd["parity"] & ~vd["degenerate"]).sum()), vd["decisions"].size, int((~vd["decisions"]).sum())
    pm = Y.prefix_maxima(vd["count"], case["min_inliers"])
    if pm:
        rl = [list(np.flatnonzero(vd["inl"][h])) for h in pm]
        vr = Y.verdicts(cam, pts, rl, Y.lapack_conventions(cam, pts, rl))
        solves, bad = solves + len(rl), bad + int((~vr["parity"] & ~vr["degenerate"]).sum())
        dec, dec_bad = dec + vr["decisions"].size, dec_bad + int((~vr["decisions"]).sum())
    print(f"  {name}: {bad} of {solves} solves, {dec_bad} of {dec} decisions outside the margins; largest move under basis noise "
          f"{np.nanmax(np.where(vd['parity'], vd['move'], np.nan)):.2e}")
    assert bad <= Y.NON_PARITY_CAP * solves and dec_bad <= Y.NON_PARITY_CAP * dec
    assert int(vd["degenerate"].sum()) == (2 if name == "degenerate_sets" else 0)


def test_host_arithmetic_invalid_sets_stay_local():
    case = pnp_host.case("kitti")
    sets = case["sets"].copy()
    sets[3] = [1, 2, 2, 5]
    sets[7] = [0, 1, 2, 60]
    sets[8] = [-1, 1, 2, 3]
    a = pnp_host.host_solve(case["cam"], case["points"], case["sets"], case["min_inliers"])
    b = pnp_host.host_solve(case["cam"], case["points"], sets, case["min_inliers"])
    for h in (3, 7, 8):
        assert not b.words[h].any() and b.hyps[h]["n_inliers"] == 0 and b.hyps[h]["refine"] == -1 and not b.hyps[h]["R"].any()
    keep = np.setdiff1d(np.arange(35), [3, 7, 8])
    assert a.hyps[keep][["R", "t", "n_inliers", "winner"]].tobytes() == b.hyps[keep][["R", "t", "n_inliers", "winner"]].tobytes()
    assert np.array_equal(a.words[keep], b.words[keep])


def _solve_rc(L, cam, pts, n, sets, min_set, H, min_inliers, result=True, mask=True):
    res, msk = np.zeros(1, _lib.PNP_RESULT_DTYPE), np.zeros(32, np.uint64)
    return L.orbfe_pnp_solve(_lib.ptr(cam), _lib.ptr(pts), n, _lib.ptr(sets), min_set, H, min_inliers, None, None, None, None, None, None,
                             _lib.ptr(res) if result else None, _lib.ptr(msk) if mask else None)


def test_pnp_solve_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    case = pnp_host.case("kitti")
    cam, pts, sets = pnp_host.camera(case["cam"]), np.array(case["points"]), np.array(case["sets"][:4])
    big_p, big_s = np.zeros(_lib.PNP_MAX_POINTS + 1, _lib.PNP_POINT_DTYPE), np.zeros((_lib.PNP_MAX_HYPOTHESES + 1, 4), np.int32)
    big_s[:] = [0, 1, 2, 3]
    assert _solve_rc(L, cam, pts, 60, sets, 4, 4, 30) == good
    assert _solve_rc(L, cam, big_p, _lib.PNP_MAX_POINTS, sets, 4, 4, 2000) == good              # n < min_inliers: nothing is launched
    assert _solve_rc(L, cam, pts, 60, big_s, 4, 0, 30) == good and _solve_rc(L, cam, None, 0, None, 4, 0, 4) == good
    inv = _lib.ERR_INVALID
    assert _solve_rc(L, None, pts, 60, sets, 4, 4, 30) == inv and "camera" in L.orbfe_last_error().decode()
    assert _solve_rc(L, cam, pts, 60, sets, 4, 4, 30, result=False) == inv and _solve_rc(L, cam, pts, 60, sets, 4, 4, 30, mask=False) == inv
    assert _solve_rc(L, cam, pts, -1, sets, 4, 4, 30) == inv and _solve_rc(L, cam, big_p, _lib.PNP_MAX_POINTS + 1, sets, 4, 4, 30) == inv
    assert _solve_rc(L, cam, pts, 60, sets, 4, -1, 30) == inv and _solve_rc(L, cam, pts, 60, big_s, 4, _lib.PNP_MAX_HYPOTHESES + 1, 30) == inv
    assert _solve_rc(L, cam, pts, 60, sets, 4, 4, 3) == inv and _solve_rc(L, cam, pts, 60, sets, 3, 4, 30) == inv
    assert _solve_rc(L, cam, pts, 60, sets, 5, 4, 30) == inv
    assert _solve_rc(L, cam, None, 60, sets, 4, 4, 30) == inv and _solve_rc(L, cam, pts, 60, None, 4, 4, 30) == inv
    for row in ([0, 1, 2, 60], [-1, 1, 2, 3], [5, 5, 6, 7], [5, 6, 7, 5], [5, 6, 6, 7], [4, 5, 6, 6]):
        s = sets.copy()
        s[2] = row
        assert _solve_rc(L, cam, pts, 60, s, 4, 4, 30) == inv and "set 2" in L.orbfe_last_error().decode()


def _batch_rc(L, P=0, cap=8, h_cap=8, drop=None, shift=None):
    """fake but aligned device addresses and P == 0: every check runs, nothing can be launched"""
    a = [0x1000 * (i + 1) for i in range(14)]                     # camera points n sets H min hyps words refines rwords diag rdiag result mask
    if drop is not None:
        a[drop] = None
    if shift is not None:
        a[shift[0]] += shift[1]
    vp = [C.c_void_p(x) for x in a]
    return L.orbfe_pnp_solve_batch_device(P, vp[0], vp[1], vp[2], cap, vp[3], vp[4], h_cap, vp[5], vp[6], vp[7], vp[8], vp[9], vp[10], vp[11],
                                          vp[12], vp[13], None)


def test_pnp_batch_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    inv = _lib.ERR_INVALID
    assert _batch_rc(L) == good and _batch_rc(L, drop=10) == good and _batch_rc(L, drop=11) == good      # the diagnostics are optional
    assert _batch_rc(L, cap=_lib.PNP_MAX_POINTS, h_cap=_lib.PNP_MAX_HYPOTHESES) == good
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13):
        assert _batch_rc(L, drop=k) == inv
    assert _batch_rc(L, P=-1) == inv and _batch_rc(L, P=_lib.PNP_MAX_PROBLEMS + 1) == inv
    assert _batch_rc(L, cap=0) == inv and _batch_rc(L, cap=_lib.PNP_MAX_POINTS + 1) == inv
    assert _batch_rc(L, h_cap=0) == inv and _batch_rc(L, h_cap=_lib.PNP_MAX_HYPOTHESES + 1) == inv
    for k in (0, 1, 2, 3, 4, 5, 12):
        assert _batch_rc(L, shift=(k, 2)) == inv and _batch_rc(L, shift=(k, 4)) == good
    for k in (6, 7, 8, 9, 10, 11, 13):
        assert _batch_rc(L, shift=(k, 4)) == inv and _batch_rc(L, shift=(k, 8)) == good


def test_no_device_is_an_error_not_a_fallback(L):
    """Through the Python mirror: without a device the host form raises ORBFE_ERR_NO_DEVICE (with one it simply runs)."""
    case = pnp_host.case("kitti")
    if _gpu_present(L):
        assert pnp.pnp_solve(pnp_host.camera(case["cam"]), case["points"], case["sets"], case["min_inliers"]).result["returned"] >= 0
        return
    with pytest.raises(_lib.OrbfeError) as e:
        pnp.pnp_solve(pnp_host.camera(case["cam"]), case["points"], case["sets"], case["min_inliers"])
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
