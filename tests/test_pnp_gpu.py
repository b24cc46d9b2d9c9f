"""PnPsolver on the device (pnp_kernels.hip) against the numpy yardstick (tests/np_pnp.py): every case in host form, the correspondence
and hypothesis counts at which the kernels change their shape, refine sets around a word, the degenerate sets, and the device form
against the host form byte for byte with sentinels around everything it must not touch."""
import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, pnp
from tests import np_pnp as Y
from tests import pnp_host

pytestmark = pytest.mark.gpu
SENTINEL64 = np.uint64(0xA5A5A5A5A5A5A5A5)


def _solve(case, points=None, sets=None, min_inliers=None, **kw):
    return pnp.pnp_solve(pnp_host.camera(case["cam"]), case["points"] if points is None else points, case["sets"] if sets is None else sets,
                         case["min_inliers"] if min_inliers is None else min_inliers, **kw)


@pytest.mark.parametrize("name", Y.CASES)
def test_every_case_against_the_yardstick(name):
    case = pnp_host.case(name)
    sol = _solve(case)
    for k, v in Y.check_against_yardstick(case, sol).items():
        print(f"  {name}: {k} = {v}")
    # the host build of the same header: the same selection, and poses far inside the yardstick's tolerance
    ref = pnp_host.host_solve(case["cam"], case["points"], case["sets"], case["min_inliers"])
    assert np.array_equal(sol.hyps["n_inliers"], ref.hyps["n_inliers"]) and np.array_equal(sol.words, ref.words)
    assert sol.result["returned"] == ref.result["returned"] and sol.result["refined"] == ref.result["refined"]
    again = _solve(case)                                                     # deterministic over two runs
    for a, b in zip(sol, again):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    lean = _solve(case, want_diag=False)                                     # the diagnostics change nothing else
    assert lean.diag is None and lean.refine_diag is None
    for a, b in zip(sol[:6], lean[:6]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    bare = _solve(case, want_records=False, want_diag=False)
    assert bare.result.tobytes() == sol.result.tobytes() and bare.mask.tobytes() == sol.mask.tobytes() and bare.hyps is None


@pytest.fixture(scope="module")
def sweep():
    """129 correspondences and 40 fixed sets: four on the first four points, eight each on the first 29, 30, 63, 64 and 65, the rest
    anywhere.  One full run."""
    sc = Y.make_scene(90, 39, 0.5, 21)
    rng = np.random.default_rng(3)
    perm = rng.permutation(129)
    sc["points"] = sc["points"][perm]                                       # outliers anywhere
    sets = np.concatenate([[[0, 1, 2, 3], [3, 1, 0, 2], [2, 3, 1, 0], [1, 0, 3, 2]]] +
                          [pnp.draw_minimal_sets(k, 6, rng) for k in (29, 30, 63, 64, 65)] + [pnp.draw_minimal_sets(129, 6, rng)]).astype(np.int32)
    case = dict(sc, sets=sets, min_inliers=30)
    return case, _solve(case)


@pytest.mark.parametrize("n", [4, 29, 30, 63, 64, 65, 128, 129])
def test_correspondence_counts(sweep, n):
    """A verdict depends on its own row and its set only: the first n correspondences with the sets that fit give the full run's poses
    and the first n verdicts."""
    case, full = sweep
    fit = np.flatnonzero((case["sets"] < n).all(1))
    assert len(fit) >= 4
    mi = 30 if n >= 30 else 4
    if n < 30:                                                               # n < min_inliers: nothing is evaluated
        dead = _solve(case, points=case["points"][:n], sets=case["sets"][fit])
        assert dead.result["returned"] == -1 and dead.result["best"] == -1 and not dead.hyps.view(np.uint8).any() and not dead.words.any()
    sol = _solve(case, points=case["points"][:n], sets=case["sets"][fit], min_inliers=mi)
    for f in ("R", "t", "winner"):
        assert sol.hyps[f].tobytes() == full.hyps[f][fit].tobytes(), f
    bits = Y.unpack_bits(full.words, 129)[fit][:, :n]
    assert np.array_equal(Y.unpack_bits(sol.words, n), bits) and np.array_equal(sol.hyps["n_inliers"], bits.sum(1))
    assert sol.diag.tobytes() == full.diag[fit].tobytes()
    Y.check_against_yardstick(dict(case, points=case["points"][:n], sets=case["sets"][fit], min_inliers=mi), sol)


@pytest.mark.parametrize("H", [1, _lib.PNP_WAVES - 1, _lib.PNP_WAVES, _lib.PNP_WAVES + 1, 35, 300])
def test_hypothesis_counts(H):
    case = pnp_host.case("kitti")
    sets = pnp.draw_minimal_sets(60, 300, np.random.default_rng(17))
    full = _hyp_full(case, sets)
    sol = _solve(case, sets=sets[:H])
    assert sol.hyps.tobytes() == full.hyps[:H].tobytes() and sol.words.tobytes() == full.words[:H].tobytes()
    assert sol.refines.tobytes() == full.refines[:H].tobytes() and sol.diag.tobytes() == full.diag[:H].tobytes()
    ret, refined, best, bc = Y.find_rule(sol.hyps["n_inliers"], sol.refines["n_inliers"], case["min_inliers"])
    assert (sol.result["returned"], bool(sol.result["refined"]), sol.result["best"], sol.result["best_inliers"]) == (ret, refined, best, bc)
    if H == 300:
        Y.check_against_yardstick(dict(case, sets=sets), sol)


_FULL = {}


def _hyp_full(case, sets):
    if "run" not in _FULL:
        _FULL["run"] = _solve(case, sets=sets)
    return _FULL["run"]


@pytest.mark.parametrize("k", [11, 64, 65])
def test_refine_set_sizes(k):
    """Exactly k consistent correspondences among gross outliers, twelve sets drawn from them: the first hypothesis that finds all k
    is a best so far and its refine solves on k -- a list shorter than a word, one word, one bit into the second."""
    sc = Y.make_scene(k, 24, 0.02, 40 + k)
    sets = np.concatenate([[[k, k + 1, k + 2, k + 3]], pnp.draw_minimal_sets(k, 12, np.random.default_rng(k))]).astype(np.int32)
    case = dict(sc, sets=sets, min_inliers=10)
    sol = _solve(case)
    c = sol.hyps["n_inliers"]
    assert c.max() == k and (c == k).sum() >= 2
    h = int(np.argmax(c == k))
    assert sol.hyps["refine"][h] == h and sol.refines["n_used"][h] == k and sol.refines["n_inliers"][h] == k and sol.refines["success"][h] == 1
    assert (sol.hyps["refine"][h + 1:] == -1).all()                          # an equal count behind it is not a new best
    assert sol.result["refined"] == 1 and sol.result["best"] <= h
    Y.check_against_yardstick(case, sol)


def test_degenerate_sets_stay_local():
    """The coplanar set and the set with a repeated point: no inliers, the run ends, and the other hypotheses keep their bytes when the
    two are replaced."""
    case = pnp_host.case("degenerate_sets")
    sol = _solve(case)
    planted = sorted(case["planted"])
    for h in planted:
        assert sol.hyps["n_inliers"][h] == 0 and not sol.words[h].any() and sol.hyps["refine"][h] == -1
    sets = case["sets"].copy()
    sets[planted[0]], sets[planted[1]] = [10, 20, 30, 40], [11, 21, 31, 41]
    other = _solve(case, sets=sets)
    keep = np.setdiff1d(np.arange(len(sets)), planted)
    for f in ("R", "t", "n_inliers", "winner"):
        assert sol.hyps[f][keep].tobytes() == other.hyps[f][keep].tobytes()
    assert np.array_equal(sol.words[keep], other.words[keep]) and sol.diag[keep].tobytes() == other.diag[keep].tobytes()
    assert np.isfinite(sol.hyps["R"][keep]).all()


# ---- the device form -----------------------------------------------------------------------------------------------------------------
def _batch(problems, cap, h_cap, with_diag=True):
    """orbfe_pnp_solve_batch_device for a list of (case, n, H); returns the raw buffers"""
    import torch
    P, Wd = len(problems), (cap + 63) // 64
    cam = np.zeros(P, _lib.PNP_CAMERA_DTYPE)
    pts = np.zeros((P, cap), _lib.PNP_POINT_DTYPE)
    pts["Xw"], pts["u"], pts["v"] = np.nan, np.nan, np.nan                   # rows behind the counts must not be read
    sets = np.full((P, h_cap, 4), -7, np.int32)
    n, H, mi = (np.zeros(P, np.int32) for _ in range(3))
    for k, (c, nk, Hk) in enumerate(problems):
        cam[k] = pnp_host.camera(c["cam"])[0]
        pts[k, :nk], sets[k, :Hk] = c["points"][:nk], c["sets"][:Hk]
        n[k], H[k], mi[k] = nk, Hk, c["min_inliers"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d = [dev(x) for x in (cam, pts, n, sets, H, mi)]
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    out = dict(hyps=fill(P * h_cap * 112), words=fill(P * h_cap * Wd * 8), refines=fill(P * h_cap * 112), rwords=fill(P * h_cap * Wd * 8),
               diag=fill(P * h_cap * 640), rdiag=fill(P * h_cap * 640), res=fill(P * 80), mask=fill(P * Wd * 8))
    st = torch.cuda.Stream()
    _lib.check(_lib.lib().orbfe_pnp_solve_batch_device(P, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), cap, _lib.ptr(d[3]), _lib.ptr(d[4]),
                                                       h_cap, _lib.ptr(d[5]), _lib.ptr(out["hyps"]), _lib.ptr(out["words"]),
                                                       _lib.ptr(out["refines"]), _lib.ptr(out["rwords"]),
                                                       _lib.ptr(out["diag"]) if with_diag else None,
                                                       _lib.ptr(out["rdiag"]) if with_diag else None, _lib.ptr(out["res"]),
                                                       _lib.ptr(out["mask"]), _lib.stream_handle(st)), "orbfe_pnp_solve_batch_device")
    st.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return dict(hyps=host["hyps"].view(_lib.PNP_HYPOTHESIS_DTYPE).reshape(P, h_cap), words=host["words"].view(np.uint64).reshape(P, h_cap, Wd),
                refines=host["refines"].view(_lib.PNP_REFINE_DTYPE).reshape(P, h_cap), rwords=host["rwords"].view(np.uint64).reshape(P, h_cap, Wd),
                diag=host["diag"].view(_lib.PNP_DIAG_DTYPE).reshape(P, h_cap), rdiag=host["rdiag"].view(_lib.PNP_DIAG_DTYPE).reshape(P, h_cap),
                res=host["res"].view(_lib.PNP_RESULT_DTYPE).reshape(P), mask=host["mask"].view(np.uint64).reshape(P, Wd))


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == 0xA5).all()


def _check_batch(problems, cap, h_cap):
    b = _batch(problems, cap, h_cap)
    again = _batch(problems, cap, h_cap)
    for k in b:
        assert b[k].tobytes() == again[k].tobytes(), k                       # a second run is byte-identical
    lean = _batch(problems, cap, h_cap, with_diag=False)
    for k in b:
        assert "diag" in k or b[k].tobytes() == lean[k].tobytes(), k
    assert _untouched(lean["diag"]) and _untouched(lean["rdiag"])
    for k, (c, nk, Hk) in enumerate(problems):
        nw = (nk + 63) // 64
        live = Hk if nk >= 4 and nk >= c["min_inliers"] else 0               # a dead problem gets its result record and nothing else
        s = pnp.pnp_solve(pnp_host.camera(c["cam"]), c["points"][:nk], c["sets"][:live], c["min_inliers"])
        assert b["res"][k].tobytes() == s.result.tobytes(), k
        assert b["mask"][k, :nw].tobytes() == s.mask.tobytes() and (b["mask"][k, nw:] == SENTINEL64).all()
        assert b["hyps"][k, :live].tobytes() == s.hyps.tobytes() and b["words"][k, :live, :nw].tobytes() == s.words.tobytes(), k
        assert b["diag"][k, :live].tobytes() == s.diag.tobytes(), k
        ref = np.flatnonzero(s.hyps["refine"] >= 0)                          # refine rows exist for the best-so-far hypotheses only
        assert b["refines"][k, ref].tobytes() == s.refines[ref].tobytes() and b["rwords"][k, ref, :nw].tobytes() == s.refine_words[ref].tobytes()
        assert b["rdiag"][k, ref].tobytes() == s.refine_diag[ref].tobytes()
        rest = np.setdiff1d(np.arange(h_cap), ref)
        for name in ("refines", "rwords", "rdiag"):
            assert _untouched(b[name][k, rest]), name
        for name in ("hyps", "words", "diag"):                               # rows and words behind the counts are untouched
            assert _untouched(b[name][k, live:]), name
        assert (b["words"][k, :, nw:] == SENTINEL64).all() and (b["rwords"][k, :, nw:] == SENTINEL64).all()
    return b["res"]


def _sub(case, n, H, seed, min_inliers=None):
    sets = pnp.draw_minimal_sets(n, H, np.random.default_rng(seed)) if n >= 4 else np.full((H, 4), 1, np.int32)
    return dict(case, points=case["points"][:n].copy(), sets=sets, min_inliers=case["min_inliers"] if min_inliers is None else min_inliers), n, H


def test_batch_form_is_the_host_form_byte_for_byte():
    a, b, c = pnp_host.case("kitti"), pnp_host.case("second_best_refines"), pnp_host.case("best_at_exhaustion")
    _check_batch([(a, 60, 35)], 60, 35)                                      # P = 1, caps == counts
    _check_batch([_sub(a, 50, 9, 1, 25)], 70, 12)                            # cap > n, h_cap > H
    pa, pb, pc, pd = (b, 50, 70), _sub(a, 0, 0, 2), _sub(a, 29, 6, 3), (c, 20, 35)   # ragged, an empty problem and one with n < min_inliers
    r1 = _check_batch([pa, pb, pc, pd], 64, 70)
    r2 = _check_batch([pd, pa, pb, pc], 64, 70)                              # permuted
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 0)):
        assert r1[i].tobytes() == r2[j].tobytes()
    assert r1[1]["returned"] == -1 and r1[1]["best"] == -1 and r1[2]["returned"] == -1 and r1[0]["refined"] == 1 and r1[3]["refined"] == 0


def test_batch_form_rejects_bad_sets_locally():
    """Device form: a set with an index outside [0, n) or a repeated one is an all-zero record (refine -1) and word row; its
    neighbours keep their bytes."""
    case = pnp_host.case("kitti")
    sets = case["sets"][:12].copy()
    sets[3], sets[5], sets[8] = (0, 1, 2, 60), (-1, 4, 5, 6), (7, 9, 7, 11)
    b = _batch([(dict(case, sets=sets), 60, 12)], 60, 12)
    base = _solve(case, sets=case["sets"][:12])
    good = np.ones(12, bool)
    good[[3, 5, 8]] = False
    for f in ("R", "t", "n_inliers", "winner"):
        assert b["hyps"][0][f][good].tobytes() == base.hyps[f][good].tobytes()
    assert b["words"][0][good].tobytes() == base.words[good].tobytes()
    bad = b["hyps"][0][~good]
    assert not bad["R"].any() and not bad["t"].any() and not bad["n_inliers"].any() and (bad["refine"] == -1).all() and not b["words"][0][~good].any()
    ret, refined, best, bc = Y.find_rule(b["hyps"][0]["n_inliers"], np.where(b["hyps"][0]["refine"] >= 0, b["refines"][0]["n_inliers"], 0), 30)
    assert (b["res"][0]["returned"], bool(b["res"][0]["refined"]), b["res"][0]["best"]) == (ret, refined, best)
