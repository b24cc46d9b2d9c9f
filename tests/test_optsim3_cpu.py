"""CPU suite of the Sim3 optimisation: the numpy reading of tests/np_optsim3.py against closed-form answers, the three conditions that
make a case a parity case (margin, stability, coverage) ASSERTED on the whole case list, csrc/optsim3_internal.h compiled for the
host against the reading with the criterion of the GPU test, the solve it shares with the pose kernel (csrc/lm_internal.h) against
numpy, and the C ABI without a device: struct sizes, exports, every validation boundary, ORBFE_ERR_NO_DEVICE from both entry
points."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from refactored_orb_slam2_amd._lib import OPTSIM3_PAIR_DTYPE, OPTSIM3_RESULT_DTYPE, SIM3_VIEW_DTYPE
from tests import np_optsim3 as Q
from tests import np_pose as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4   # the value the pose tests use


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_optsim3")], check=True, capture_output=True)
    return C.CDLL(os.path.join(ROOT, "tests", "cpp_optsim3", "_build", "liboptsim3_host.so"))


@pytest.fixture(scope="module")
def runs():
    return {name: (Q.case_scene(name), Q.run_case(Q.case_scene(name))) for name in Q.CASES}


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def _view(v):
    return optimizer.sim3_view(v["Rcw"], v["tcw"], v["fx"], v["fy"], v["cx"], v["cy"])


def _skew(o):
    return np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], np.float64)


# ---- the reading against closed forms -------------------------------------------------------------------------------------------
def test_exp_closed_forms():
    q, t, s = Q.sim3_exp([0] * 7)                                        # Sim3(0) = identity
    assert q == [0.0, 0.0, 0.0, 1.0] and t == [0.0, 0.0, 0.0] and s == 1.0
    q, t, s = Q.sim3_exp([0, 0, 0, 0.25, -2.0, 3.5, 0])                  # a pure translation: W = I
    assert q == [0.0, 0.0, 0.0, 1.0] and t == [0.25, -2.0, 3.5] and s == 1.0
    sg = 0.3                                                             # a pure scale: s = e^sigma, W = (s - 1) / sigma * I
    q, t, s = Q.sim3_exp([0, 0, 0, 1.0, -2.0, 0.5, sg])
    c = (math.exp(sg) - 1) / sg
    assert q == [0.0, 0.0, 0.0, 1.0] and s == math.exp(sg) and np.allclose(t, [c, -2 * c, 0.5 * c], rtol=0, atol=4e-16)
    th = 0.3                                                             # rotation about z, no scale: the SE3 closed form
    q, t, s = Q.sim3_exp([0, 0, th, 1.0, 0, 0, 0])
    assert np.allclose(q, [0, 0, math.sin(th / 2), math.cos(th / 2)], rtol=0, atol=2e-16) and s == 1.0
    assert np.allclose(t, [math.sin(th) / th, (1 - math.cos(th)) / th, 0.0], rtol=0, atol=2e-16)
    # rotation about z with a scale: t = W e_x with W = int_0^1 e^(sigma a) R(theta a) da, whose first column is the real and
    # imaginary part of (e^(sigma + i theta) - 1) / (sigma + i theta)
    w = (np.exp(complex(sg, th)) - 1) / complex(sg, th)
    q, t, s = Q.sim3_exp([0, 0, th, 1.0, 0, 0, sg])
    assert np.allclose(t, [w.real, w.imag, 0.0], rtol=0, atol=4e-16)


def _w(sigma, theta):
    """(e^z - 1) / z for z = sigma + i theta: the first column of W for a rotation about one axis (real part along the translation's
    axis, imaginary part along the third one); its series where e^z - 1 would cancel"""
    z = complex(sigma, theta)
    return 1 + z / 2 + z * z / 6 + z ** 3 / 24 + z ** 4 / 120 if abs(z) < 1e-3 else (np.exp(z) - 1) / z


def test_exp_on_both_sides_of_each_branch():
    """theta and |sigma| just below and just above eps = 1e-5, in every combination with the other one small, at the branch and large:
    the quaternion and the translation are the closed form -- of sigma = 0 where |sigma| < eps, because the reference drops sigma
    from W there (C = 1, A and B those of a pure rotation; s = e^sigma is kept), a step of sigma / 2 = 5e-6 across that branch.  The
    bound on t is 1e-10: (1 - cos th) / th^2 is only good to ~1e-6 relative at th = 1e-5, where it multiplies th."""
    near = (0.99999e-5, 1.00001e-5)
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for th in near + (0.5e-5, 0.3):
            for sigma in near + tuple(-x for x in near) + (0.0, 0.2):
                if th not in near and abs(sigma) not in near:
                    continue
                u = [0.0] * 7
                u[axis], u[3 + b], u[6] = th, 1.0, sigma
                q, t, s = Q.sim3_exp(u)
                want = [0.0] * 4
                want[axis], want[3] = math.sin(th / 2), math.cos(th / 2)
                assert np.allclose(q, want, rtol=0, atol=1e-15) and s == math.exp(sigma), (axis, th, sigma)
                w = _w(sigma if abs(sigma) >= Q.EPS else 0.0, th)
                assert abs(t[axis]) == 0.0 and abs(t[b] - w.real) <= 1e-10 and abs(t[c] - w.imag) <= 1e-10, (axis, th, sigma, t, w)


def test_inverse_product_and_fixed_scale():
    S = Q.sim3_oplus(Q.sim3_from_floats(np.array([1.07, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, -1, 2], np.float32)),
                     [0.2, -0.1, 0.3, 0.4, 0.5, -0.6, 0.05], False)
    q, t, s = Q.sim3_mul(S, Q.sim3_inverse(S))                           # S * S^-1 = identity
    assert np.allclose(np.abs(q), [0, 0, 0, 1], rtol=0, atol=4e-16) and np.allclose(t, 0, rtol=0, atol=2e-15) and abs(s - 1) <= 4e-16
    p = (1.0, -2.0, 3.0)
    back = Q.sim3_map(Q.sim3_inverse(S), Q.sim3_map(S, p))
    assert np.allclose(back, p, rtol=0, atol=1e-14)
    # exp(u) * S moves a point as exp(u) moves S p
    E = Q.sim3_exp([0.02, -0.01, 0.03, 0.1, 0.2, -0.3, 0.04])
    assert np.allclose(Q.sim3_map(Q.sim3_mul(E, S), p), Q.sim3_map(E, Q.sim3_map(S, p)), rtol=0, atol=1e-14)
    # oplus with a fixed scale: update[6] is zeroed before it is used, s stays bit for bit
    for x6 in (0.3, -2.0, 1e-9):
        assert Q.sim3_oplus(S, [0.01, 0.02, -0.01, 0.1, 0.0, 0.2, x6], True)[2] == S[2]
    assert Q.sim3_oplus(S, [0, 0, 0, 0, 0, 0, 0.3], False)[2] == math.exp(0.3) * S[2]
    # ... and column 6 of the numeric Jacobian is exactly zero then
    s = Q.case_scene("pairs_24")
    E_ = Q._Edges(s["view1"], s["view2"], s["pairs"])
    J = E_.jacobians(Q.sim3_from_floats(s["sRt_in"]), True, 1e-9)
    assert not J[:, :, 6].any() and J[:, :, :6].any()
    assert E_.jacobians(Q.sim3_from_floats(s["sRt_in"]), False, 1e-9)[:, :, 6].any()


def test_numeric_jacobian_against_the_analytic_one():
    """d e12 / d upsilon at the estimate is -s-independent: -(fx / z, 0, -fx x / z^2; 0, fy / z, -fy y / z^2) for the translation
    columns; the central difference with step 1e-6 reproduces it to ~1e-6 relative"""
    s = Q.case_scene("pairs_24")
    E_ = Q._Edges(s["view1"], s["view2"], s["pairs"])
    S = Q.sim3_from_floats(s["sRt_in"])
    J = E_.jacobians(S, False, 1e-6)[0::2]
    x, y, z = Q.sim3_map(S, (E_.P12[:, 0], E_.P12[:, 1], E_.P12[:, 2]))
    fx, fy = E_.K1[0], E_.K1[1]
    want = np.zeros((len(x), 2, 3))
    want[:, 0, 0], want[:, 0, 2] = -fx / z, fx * x / z ** 2
    want[:, 1, 1], want[:, 1, 2] = -fy / z, fy * y / z ** 2
    assert np.allclose(J[:, :, 3:6], want, rtol=1e-5, atol=1e-4)


def test_ldlt_against_numpy():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(11, 7))
    Hm = A.T @ A + 1e-3 * np.eye(7)
    b = rng.normal(size=7)
    ok, x = Q.ldlt_solve(Hm.tolist(), b.tolist())
    assert ok and np.allclose(x, np.linalg.solve(Hm, b), rtol=1e-9, atol=0)
    Hm[2, 2] = -1.0
    assert Q.ldlt_solve(Hm.tolist(), b.tolist())[0] is False


def test_scenes_are_pulled_to_the_truth_and_flag_the_planted_outliers(runs):
    """A planted offset of >= 4 px on both axes at level 0 is chi2 >= 32 against a bound of 10; at level l the offset is not scaled,
    so a high-level outlier can pass: the floor asserted is 60 % of the planted ones, and no more than 2 % false alarms"""
    for name in ("fixed_scale", "free_scale", "outliers_40", "beyond_cache", "levels_12"):
        s, r = runs[name]
        e_in = np.abs(s["sRt_in"].astype(np.float64) - s["sRt_true"]).max()
        e_out = np.abs(r["sRt64"] - s["sRt_true"]).max()
        bad, planted = r["bad"].astype(bool), s["planted"]
        print(f"{name}: error {e_in:.3g} -> {e_out:.3g}, planted flagged {int((bad & planted).sum())}/{int(planted.sum())}, "
              f"others flagged {int((bad & ~planted).sum())}/{int((~planted).sum())}")
        assert e_out < 0.25 * e_in
        assert (bad & planted).sum() >= 0.6 * planted.sum() and (bad & ~planted).sum() <= 0.02 * (~planted).sum() + 1


# ---- the conditions a parity case must meet --------------------------------------------------------------------------------------
def test_condition_margin(runs):
    """no correspondence sits on the bound: |chi2 - th2| / th2 >= 1e-4 at both classifications, so that a reading and a kernel that
    differ in the last bits decide alike"""
    for name, (s, r) in runs.items():
        m = Q.min_margin(r, s["th2"])
        print(f"margin {name}: {m:.3g}")
        assert m >= MARGIN, name


def test_condition_stability(runs):
    """the reading at Jacobian steps 1e-9 and 1e-6, and in 4 random summation orders (half of them with relative noise 1e-13 on every
    reduction): same flags, same counts, the unrounded result within HALF the tolerance of the GPU test"""
    for name, (s, r) in runs.items():
        tol = Q.tolerance(r["sRt64"])
        worst = {}
        variants = [("step 1e-6", dict(jac_step=1e-6))] + [(f"order {k}", dict(order_seed=1000 + k, noise=1e-13 if k % 2 else 0.0)) for k in range(4)]
        for what, kw in variants:
            q = Q.run_case(s, **kw)
            assert np.array_equal(q["bad"], r["bad"]), (name, what)
            assert (q["n_pairs"], q["n_bad"], q["n_inliers"]) == (r["n_pairs"], r["n_bad"], r["n_inliers"]), (name, what)
            d = float((np.abs(q["sRt64"] - r["sRt64"]) / tol).max())
            worst[what.split()[0]] = max(worst.get(what.split()[0], 0.0), d)
            assert d <= 0.5, (name, what, d)
        print(f"stability {name}: worst diff / tolerance: Jacobian step {worst['step']:.3f}, summation {worst['order']:.3f}")


def test_condition_coverage(runs):
    """the case list exercises what the kernel has to get right"""
    r = {name: v[1] for name, v in runs.items()}
    assert any(x["n_bad"] > 0 and x["n_inliers"] > 0 for x in r.values())
    assert r["clean"]["n_bad"] == 0 and r["clean"]["n_inliers"] == 60 and r["clean"]["iterations"][1] <= 5   # nBad == 0: optimize(5)
    assert any(x["iterations"][1] > 5 for x in r.values())                                                 # nBad > 0: optimize(10)
    for name in ("pairs_12_return_0", "pairs_9"):                     # return 0 with bad flags set, g2oS12 not written
        assert r[name]["n_inliers"] == 0 and r[name]["bad"].sum() == r[name]["n_bad"] > 0 and r[name]["iterations"][1] == 0
        assert r[name]["sRt"].tobytes() == runs[name][0]["sRt_in"].tobytes()
    assert r["pairs_12_return_0"]["n_bad"] in (3, 4) and r["pairs_9"]["n_pairs"] == 9
    assert r["survivors_10"]["n_pairs"] - r["survivors_10"]["n_bad"] == 10 and r["survivors_10"]["iterations"][1] > 0
    assert r["pairs_0"]["n_pairs"] == 0 and r["pairs_0"]["sRt"].tobytes() == runs["pairs_0"][0]["sRt_in"].tobytes()
    assert r["beyond_cache"]["n_pairs"] > 2048 and len(runs["levels_12"][0]["inv_level_sigma2"]) == 12
    assert {runs[n][0]["fix_scale"] for n in runs} == {True, False} and abs(float(runs["free_scale"][0]["sRt_true"][0]) - 1) > 0.05
    assert any(t["rejected"] > 0 for x in r.values() for t in x["trace"])                                  # rejected trials occur
    assert any((x["bad"].sum() > x["n_bad"]) for x in r.values())                                           # ... and second-round drops


# ---- csrc/optsim3_internal.h compiled for the host -------------------------------------------------------------------------------
def test_host_build_of_the_exponential(H):
    rng = np.random.default_rng(5)
    us = [np.zeros(7), np.array([0, 0, 0, 1, 2, 3, 0.0]), np.array([0, 0, 0.99999e-5, 1, 0, 0, 0.2]), np.array([0, 1.00001e-5, 0, 0, 0, 1, 1e-6])]
    us += [rng.normal(size=7) * 0.1 for _ in range(8)]
    for u in us:
        u = np.ascontiguousarray(u, np.float64)
        out = np.zeros(8)
        H.optsim3_host_exp(_lib.ptr(u), _lib.ptr(out))
        q, t, s = Q.sim3_exp(u)
        assert np.allclose(out, q + t + [s], rtol=0, atol=4e-16), u


def test_host_build_against_the_reading(H, runs):
    """the GPU test's criterion: flags and counts equal, every entry within one float ulp at the scale of its block"""
    for name, (s, ref) in runs.items():
        n = len(s["pairs"])
        res, bad = np.zeros(1, OPTSIM3_RESULT_DTYPE), np.zeros(max(n, 1), np.uint8)
        v1, v2 = _view(s["view1"]), _view(s["view2"])
        H.optsim3_host(_lib.ptr(v1), _lib.ptr(v2), _lib.ptr(s["pairs"]), n, _lib.ptr(s["sRt_in"]), C.c_float(float(s["th2"])),
                       int(s["fix_scale"]), _lib.ptr(res), _lib.ptr(bad))
        res = res[0]
        v = np.concatenate([[res["s"]], res["R"], res["t"]]).astype(np.float64)
        d = np.abs(v - ref["sRt"].astype(np.float64)) / Q.tolerance(ref["sRt"])
        print(f"host build {name}: max diff / tolerance {d.max():.3f}, iterations {list(res['iterations'])} (reading {ref['iterations']})")
        assert np.array_equal(bad[:n], ref["bad"]), name
        assert (int(res["n_pairs"]), int(res["n_bad"]), int(res["n_inliers"])) == (ref["n_pairs"], ref["n_bad"], ref["n_inliers"]), name
        assert np.all(d <= 1.0), (name, d)


@pytest.mark.parametrize("n, rows", [(6, 9), (7, 11)])
def test_host_build_of_the_shared_solve(H, n, rows):
    """csrc/lm_internal.h's lm_ldlt_solve<6> and <7> themselves (the pose and the Sim3 kernel's solve), on the matrices of the two
    test_ldlt_against_numpy tests: against numpy at their rtol, lambda added as the diagonal it is, a non-positive pivot reported"""
    H.optsim3_host_ldlt.restype = C.c_int
    iu = np.triu_indices(n)   # row-major, i <= j

    def solve(Hm, lam, b):
        x = np.zeros(n)
        rc = H.optsim3_host_ldlt(n, _lib.ptr(np.ascontiguousarray(Hm[iu])), C.c_double(lam), _lib.ptr(b), _lib.ptr(x))
        return rc, x

    rng = np.random.default_rng(3)
    A = rng.normal(size=(rows, n))
    Hm = A.T @ A + 1e-3 * np.eye(n)
    b = rng.normal(size=n)
    rc, x = solve(Hm, 0.0, b)
    assert rc == 1 and np.allclose(x, np.linalg.solve(Hm, b), rtol=1e-9, atol=0)
    rc_l, x_l = solve(Hm, 0.37, b)
    rc_d, x_d = solve(Hm + 0.37 * np.eye(n), 0.0, b)
    assert rc_l == 1 and rc_d == 1 and x_l.tobytes() == x_d.tobytes()
    Hm[2, 2] = -1.0
    assert solve(Hm, 0.0, b)[0] == 0
    assert H.optsim3_host_ldlt(5, _lib.ptr(np.zeros(15)), C.c_double(0.0), _lib.ptr(np.zeros(5)), _lib.ptr(np.zeros(5))) == -1


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_struct_sizes_and_exports(L, H):
    sizes = np.zeros(4, np.int32)
    H.optsim3_host_sizes(_lib.ptr(sizes))
    assert list(sizes) == [OPTSIM3_PAIR_DTYPE.itemsize, OPTSIM3_RESULT_DTYPE.itemsize, OPTSIM3_RESULT_DTYPE.fields["n_pairs"][1],
                           OPTSIM3_RESULT_DTYPE.fields["iterations"][1]]
    assert OPTSIM3_PAIR_DTYPE.itemsize == 48 and OPTSIM3_RESULT_DTYPE.itemsize == 80 and OPTSIM3_RESULT_DTYPE.itemsize % 16 == 0
    for name in ("orbfe_optimize_sim3", "orbfe_optimize_sim3_batch_device"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert hasattr(optimizer, "optimize_sim3") and hasattr(optimizer, "optimize_sim3_batch")


def test_host_form_validation_boundaries(L):
    """every limit at its largest accepted and its first refused value; what passes validation then needs a device"""
    past = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    v = np.zeros(1, SIM3_VIEW_DTYPE)
    v["Rcw"][0, [0, 4, 8]] = 1
    v["fx"] = v["fy"] = 500
    pairs = np.zeros(_lib.OPTSIM3_MAX_PAIRS + 1, OPTSIM3_PAIR_DTYPE)
    pairs["Xw1"][:, 2] = pairs["Xw2"][:, 2] = 5
    pairs["inv_sigma2_1"] = pairs["inv_sigma2_2"] = 1
    bad = np.zeros(len(pairs), np.uint8)
    sRt = np.array([1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    res = np.zeros(1, OPTSIM3_RESULT_DTYPE)
    f = lambda n=24, th2=10.0, v1=v, v2=v, p=pairs, x=sRt, r=res, b=bad: L.orbfe_optimize_sim3(
        _lib.ptr(v1), _lib.ptr(v2), _lib.ptr(p), n, _lib.ptr(x), C.c_float(th2), 0, _lib.ptr(r), _lib.ptr(b))
    assert f() == past
    assert f(n=_lib.OPTSIM3_MAX_PAIRS) == past and f(n=_lib.OPTSIM3_MAX_PAIRS + 1) == _lib.ERR_INVALID
    assert b"9500" in L.orbfe_last_error()
    assert f(n=0) == past and f(n=0, p=None, b=None) == past and f(n=-1) == _lib.ERR_INVALID
    assert f(n=1, p=None) == _lib.ERR_INVALID and f(n=1, b=None) == _lib.ERR_INVALID
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    assert f(th2=tiny) == past and f(th2=0.0) == _lib.ERR_INVALID and f(th2=-1.0) == _lib.ERR_INVALID
    assert f(th2=float("nan")) == _lib.ERR_INVALID and f(th2=float("inf")) == past
    for kw in (dict(v1=None), dict(v2=None), dict(x=None), dict(r=None)):
        assert f(**kw) == _lib.ERR_INVALID, kw
    if not _gpu_present(L):
        assert b"no CPU fallback" in L.orbfe_last_error() or f() == _lib.ERR_NO_DEVICE
        with pytest.raises(_lib.OrbfeError):
            optimizer.optimize_sim3(v, v, pairs[:24], sRt, 10.0, True)


def test_batch_form_validation_boundaries(L):
    past = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    buf = np.zeros(4096, np.uint8)   # never dereferenced: P == 0 launches nothing, and without a device nothing is launched at all
    a = buf.ctypes.data
    assert a % 4 == 0
    args = dict(P=0, v1=a, v2=a + 64, pairs=a + 128, n=a + 256, cap=24, x=a + 512, th2=a + 1024, fix=a + 1028, res=a + 2048, bad=a + 3000)
    order = ("P", "v1", "v2", "pairs", "n", "cap", "x", "th2", "fix", "res", "bad")

    def f(**kw):
        d = dict(args, **kw)
        vals = [d[k] if k in ("P", "cap") else C.c_void_p(d[k]) for k in order]
        return L.orbfe_optimize_sim3_batch_device(*vals, None)

    assert f() == past
    assert f(P=-1) == _lib.ERR_INVALID and f(P=_lib.OPTSIM3_MAX_PROBLEMS + 1) == _lib.ERR_INVALID
    assert f(cap=_lib.OPTSIM3_MAX_PAIRS) == past and f(cap=_lib.OPTSIM3_MAX_PAIRS + 1) == _lib.ERR_INVALID and f(cap=-1) == _lib.ERR_INVALID
    assert f(cap=0) == past and f(cap=0, pairs=None, bad=None) == past
    for k in ("v1", "v2", "pairs", "n", "x", "th2", "fix", "res", "bad"):
        assert f(**{k: None}) == _lib.ERR_INVALID, k
    for k in ("v1", "v2", "pairs", "n", "x", "th2", "fix", "res"):   # 4-byte alignment of every record; d_bad is bytes
        assert f(**{k: args[k] + 2}) == _lib.ERR_INVALID, k
    assert f(bad=args["bad"] + 1) == past
    if not _gpu_present(L):   # P at its largest accepted value passes validation and then needs a device
        assert f(P=_lib.OPTSIM3_MAX_PROBLEMS) == _lib.ERR_NO_DEVICE and b"no CPU fallback" in L.orbfe_last_error()
