"""CPU suite of the pose optimisation: the numpy reading of tests/np_pose.py against closed-form answers, the three conditions that
make a case a parity case (margin, stability, coverage) ASSERTED on the whole case list, and the C ABI without a device: struct
sizes, exports, every validation boundary, ORBFE_ERR_NO_DEVICE from both entry points."""
import ctypes as C
import math

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from tests import np_pose as P


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def runs():
    return {name: (P.case_scene(name), P.run_case(P.case_scene(name))) for name in P.CASES}


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


# ---- the reading against closed forms -------------------------------------------------------------------------------------------
def test_exp_closed_forms():
    q, t = P.se3_exp([0, 0, 0, 0, 0, 0])
    assert q == [0.0, 0.0, 0.0, 1.0] and t == [0.0, 0.0, 0.0]
    q, t = P.se3_exp([0, 0, 0, 0.25, -2.0, 3.5])                      # a pure translation: V = I
    assert q == [0.0, 0.0, 0.0, 1.0] and t == [0.25, -2.0, 3.5]
    th = 0.3
    q, t = P.se3_exp([0, 0, th, 1.0, 0, 0])                            # rotation about z: q = (0, 0, sin th/2, cos th/2)
    assert np.allclose(q, [0, 0, math.sin(th / 2), math.cos(th / 2)], rtol=0, atol=2e-16)
    # V e_x = (sin th / th, (1 - cos th) / th, 0)
    assert np.allclose(t, [math.sin(th) / th, (1 - math.cos(th)) / th, 0.0], rtol=0, atol=2e-16)
    R = np.array(P.quat_to_matrix(q))
    assert np.allclose(R, P.rodrigues([0, 0, th]), rtol=0, atol=4e-16)
    # across the theta = 1e-5 branch: the second-order form and the closed form agree to theta^3 / 6 ~ 2e-16
    for axis in range(3):
        for th in (0.99999e-5, 1.00001e-5):
            u = [0.0] * 6
            u[axis], u[3 + (axis + 1) % 3] = th, 1.0
            q, t = P.se3_exp(u)
            want = [0.0] * 4
            want[axis], want[3] = math.sin(th / 2), math.cos(th / 2)
            assert np.allclose(q, want, rtol=0, atol=1e-15)
            V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * _skew(u[:3]) + (th - math.sin(th)) / th ** 3 * _skew(u[:3]) @ _skew(u[:3])
            assert np.allclose(t, V @ np.array(u[3:]), rtol=0, atol=1e-10)   # (1 - cos th) / th^2 itself is only good to ~1e-6 here
    # exp(u) * T moves a point as R (T p) + t
    T = P.se3_from_Tcw(np.array([1, 0, 0, 0.5, 0, 1, 0, -1, 0, 0, 1, 2], np.float32))
    E = P.se3_exp([0.02, -0.01, 0.03, 0.1, 0.2, -0.3])
    p = (1.0, 2.0, 3.0)
    a = P.quat_rotate(P.se3_mul(E, T)[0], p)
    a = [a[i] + P.se3_mul(E, T)[1][i] for i in range(3)]
    b = P.quat_rotate(E[0], [p[0] + 0.5, p[1] - 1, p[2] + 2])
    b = [b[i] + E[1][i] for i in range(3)]
    assert np.allclose(a, b, rtol=0, atol=1e-15)


def _skew(o):
    return np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], np.float64)


def test_huber_closed_forms():
    d = P.DELTA_MONO
    assert P.huber(d * d, d) == (d * d, 1.0, 0.0)                      # at delta^2: still the quadratic branch
    assert P.huber(1.5, d) == (1.5, 1.0, 0.0)
    e = 4 * d * d                                                       # sqrt(e) = 2 delta: rho = 3 delta^2, rho' = 1/2
    r0, r1, r2 = P.huber(e, d)
    assert math.isclose(r0, 3 * d * d, rel_tol=1e-15) and math.isclose(r1, 0.5, rel_tol=1e-15) and math.isclose(r2, -0.25 / e, rel_tol=1e-15)
    r0, r1, _ = P.huber(np.nextafter(d * d, 9.0), d)                   # continuous across the branch
    assert math.isclose(r0, d * d, rel_tol=1e-14) and math.isclose(r1, 1.0, rel_tol=1e-14)
    # delta^2 and the chi2 bound are the same number up to float rounding: a final inlier is never on the Huber branch
    assert abs(P.DELTA_MONO ** 2 / float(P.CHI2_MONO) - 1) < 2e-7 and abs(P.DELTA_STEREO ** 2 / float(P.CHI2_STEREO) - 1) < 2e-7


def test_ldlt_against_numpy():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(9, 6))
    H = A.T @ A + 1e-3 * np.eye(6)
    b = rng.normal(size=6)
    ok, x = P.ldlt_solve(H.tolist(), b.tolist())
    assert ok and np.allclose(x, np.linalg.solve(H, b), rtol=1e-9, atol=0)
    H[2, 2] = -1.0
    assert P.ldlt_solve(H.tolist(), b.tolist())[0] is False            # not positive: the trial is a bad step


def test_noise_free_scene_returns_the_true_pose():
    """Inputs are exact up to their rounding to float (observations: 2^-24 x 1241 px = 7e-5 px; points: 2^-24 x 60 m, 4e-5 px at 4 m),
    so every residual at the true pose is below 2e-4 px against sigma >= 1: the minimum lies within 2e-4 px / fx = 3e-7 rad of the
    truth in rotation and within that angle x the far depth (60 m) = 2e-5 m in translation, before averaging over 1 000 edges."""
    s = P.make_scene(31, outliers=0.0, noise=False)
    r = P.run_case(s)
    d = np.abs(r["Tcw"].astype(np.float64) - s["Tcw_true"]).reshape(3, 4)
    print("noise-free: rotation error", d[:, :3].max(), "translation error", d[:, 3].max())
    assert r["n_bad"] == 0 and not r["outlier"].any() and r["n_inliers"] == 1000 and r["rounds"] == 4
    assert d[:, :3].max() <= 3e-7 and d[:, 3].max() <= 2e-5


def test_scene_with_outliers_is_pulled_to_the_truth_and_flags_them(runs):
    """A planted offset of >= 4 px x scale on both axes is chi2 >= 32 against a bound of 7.8: the reading should flag all of them;
    the floor asserted is 90 %."""
    for name in ("standard", "outliers_40", "large_error", "all_mono", "all_stereo"):
        s, r = runs[name]
        e_in = np.abs(s["Tcw_in"].astype(np.float64) - s["Tcw_true"]).max()
        e_out = np.abs(r["Tcw"].astype(np.float64) - s["Tcw_true"]).max()
        planted = s["planted"]
        hit = int((r["outlier"].astype(bool) & planted).sum())
        print(f"{name}: error {e_in:.3g} -> {e_out:.3g}, planted outliers flagged {hit}/{int(planted.sum())}")
        assert e_out < 0.2 * e_in
        assert hit >= 0.9 * planted.sum() and planted.sum() > 50


# ---- the conditions a parity case must meet --------------------------------------------------------------------------------------
def _margin(r):
    return min((float(np.abs(t["chi2"].astype(np.float64) / t["bound"].astype(np.float64) - 1).min()) for t in r["trace"]), default=1.0)


def test_condition_margin(runs):
    """over all rounds and edges |chi2 / bound - 1| >= 1e-4: the classification compares floats (granularity 6e-8) and two double
    implementations differ near 1e-15 (1e-10 for the edges the kernel evaluates at the final pose); 1e-4 is far from both"""
    for name, (s, r) in runs.items():
        m = _margin(r)
        print(f"margin {name}: {m:.3g}")
        assert m >= 1e-4, name


def test_condition_stability(runs):
    """8 random summation orders, half of them with relative noise 1e-13 on every reduction: same flags, same counts, poses within
    the tolerance of the GPU test"""
    for name, (s, r) in runs.items():
        worst, not_equal = 0.0, 0
        for k in range(8):
            q = P.run_case(s, order_seed=1000 + k, noise=1e-13 if k % 2 else 0.0)
            assert np.array_equal(q["outlier"], r["outlier"]), (name, k)
            assert (q["n_initial"], q["n_bad"], q["n_inliers"], q["rounds"]) == (r["n_initial"], r["n_bad"], r["n_inliers"], r["rounds"])
            d = np.abs(q["Tcw"].astype(np.float64) - r["Tcw"].astype(np.float64)) / P.pose_tolerance(r["Tcw"])
            worst = max(worst, float(d.max()))
            not_equal += int((q["Tcw"].view(np.uint32) != r["Tcw"].view(np.uint32)).sum())
            assert P.poses_agree(q["Tcw"], r["Tcw"]), (name, k, d)
        print(f"stability {name}: worst diff / tolerance {worst:.3f}, entries not bit-equal over 8 runs {not_equal}/96")


def test_condition_coverage(runs):
    """the case list exercises what the kernel has to get right: rejected trials, both Terminate exits that occur in practice, an
    edge that is an outlier after round 0 and an inlier at the end, active edges on the Huber branch"""
    rejected = sum(t["rejected"] for _, r in runs.values() for t in r["trace"])
    exits = [t["exit"] for _, r in runs.values() for t in r["trace"]]
    readmitted = sum(int((r["trace"][0]["outlier"] & ~r["trace"][-1]["outlier"]).sum()) for _, r in runs.values() if len(r["trace"]) == 4)
    huber_active = 0
    for s, r in runs.values():
        if r["trace"]:
            t0 = r["trace"][0]      # round 0: every edge is active; chi2 above delta^2 = on the Huber branch
            huber_active += int((t0["chi2"].astype(np.float64) > np.where(t0["bound"] > 7, P.DELTA_STEREO, P.DELTA_MONO) ** 2).sum())
    print(f"coverage: {rejected} rejected trials, exits {dict((e, exits.count(e)) for e in set(exits))}, {readmitted} edges re-admitted, "
          f"{huber_active} round-0 edges on the Huber branch")
    assert rejected >= 100 and exits.count("trials") >= 3 and exits.count("rho0") >= 3 and exits.count("iterations") >= 3
    assert readmitted >= 1 and huber_active >= 500
    # one round below 10 edges, none below 3
    assert runs["edges_9"][1]["rounds"] == 1 and runs["edges_3"][1]["rounds"] == 1 and runs["edges_12"][1]["rounds"] == 4
    r2 = runs["edges_2"][1]
    assert r2["rounds"] == 0 and r2["n_inliers"] == 0 and np.array_equal(r2["Tcw"], runs["edges_2"][0]["Tcw_in"])
    # every case has unmatched rows interleaved with the matched ones
    for name, (s, r) in runs.items():
        a = s["assigned"]
        assert (a < 0).sum() >= 1 and r["n_initial"] == (a >= 0).sum(), name
        if r["n_initial"] > 20:
            first, last = np.flatnonzero(a >= 0)[[0, -1]]
            assert (a[first:last] < 0).sum() > 5, name


# ---- the C ABI without a device --------------------------------------------------------------------------------------------------
def test_struct_sizes_and_exports(L):
    assert _lib.POSE_CAMERA_DTYPE.itemsize == 88 and _lib.POSE_RESULT_DTYPE.itemsize == 68
    assert _lib.POSE_CAMERA_DTYPE.fields["n_levels"][1] == 20 and _lib.POSE_CAMERA_DTYPE.fields["inv_level_sigma2"][1] == 24
    assert _lib.POSE_RESULT_DTYPE.fields["n_initial"][1] == 48 and _lib.POSE_RESULT_DTYPE.fields["iterations"][1] == 64
    for name in ("orbfe_pose_optimization", "orbfe_pose_optimization_batch_device"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.POSE_DISCARD == 1


def _host_args(n=4, n_points=3, levels=8, stride=60):
    keys = np.zeros(max(n, 1), _lib.KP_DTYPE)
    fv = _lib.FrameView(n, keys.ctypes.data, None, None, 0, 0, 0, 0)
    assigned = np.full(max(n, 1), -1, np.int32)
    pts = np.zeros(max(n_points, 1) * stride, np.uint8)
    cam = optimizer.pose_camera(700, 700, 600, 180, 380, np.ones(8, np.float32))
    cam["n_levels"] = levels
    T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    res = np.zeros(1, _lib.POSE_RESULT_DTYPE)
    out = np.zeros(max(n, 1), np.uint8)
    keep = (keys, assigned, pts, cam, T, res, out)
    return keep, [C.byref(fv), _lib.ptr(assigned), _lib.ptr(pts), stride, n_points, _lib.ptr(cam), _lib.ptr(T), _lib.ptr(res), _lib.ptr(out)]


def test_host_form_validation_boundaries(L):
    """every limit at its largest accepted and first refused value; an accepted call needs a device next (no CPU fallback)"""
    accepted = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    good = (dict(), dict(levels=1), dict(levels=16), dict(stride=12), dict(stride=72), dict(n=0), dict(n=_lib.POSE_MAX_ROWS), dict(n_points=0))
    bad = (dict(levels=0), dict(levels=17), dict(stride=8), dict(stride=11), dict(stride=14), dict(stride=0), dict(n=-1),
           dict(n=_lib.POSE_MAX_ROWS + 1), dict(n_points=-1))
    for kw in good:
        keep, a = _host_args(**kw)
        assert L.orbfe_pose_optimization(*a) == accepted, kw
    for kw in bad:
        keep, a = _host_args(**kw)
        assert L.orbfe_pose_optimization(*a) == _lib.ERR_INVALID, kw
        assert b"pose optimisation" in L.orbfe_last_error()
    for null in (0, 1, 2, 5, 6, 7, 8):     # frame, assigned, points, camera, Tcw_in, result, outlier
        keep, a = _host_args()
        a[null] = None
        assert L.orbfe_pose_optimization(*a) == _lib.ERR_INVALID, null
    if not _gpu_present(L):
        keep, a = _host_args()
        assert L.orbfe_pose_optimization(*a) == _lib.ERR_NO_DEVICE and b"no CPU fallback" in L.orbfe_last_error()
        with pytest.raises(_lib.OrbfeError):
            optimizer.pose_optimization(np.zeros(4, _lib.KP_DTYPE), None, np.full(4, -1, np.int32), np.zeros((3, 3), np.float32),
                                        optimizer.pose_camera(700, 700, 600, 180, 380, np.ones(8, np.float32)), np.eye(4, dtype=np.float32))


def _batch_args(**kw):
    """n_frames = 0: validation runs in full and nothing is launched, so made-up (aligned, non-null) device pointers are never read"""
    p = 0x1000
    a = dict(n_frames=0, keys=p, ur=p, n=p, cap=2000, assigned=p, points=p, stride=60, n_points=p, p_cap=2000, shift=1, cam=p, T=p, res=p,
             out=p, flags=0, stream=None)
    a.update(kw)
    return [a[k] for k in ("n_frames", "keys", "ur", "n", "cap", "assigned", "points", "stride", "n_points", "p_cap", "shift", "cam", "T",
                           "res", "out", "flags", "stream")]


def test_batch_form_validation_boundaries(L):
    accepted = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    f = L.orbfe_pose_optimization_batch_device
    good = (dict(), dict(ur=None), dict(cap=1), dict(cap=_lib.POSE_MAX_ROWS), dict(p_cap=1), dict(shift=0), dict(shift=2 ** 30), dict(stride=12),
            dict(stride=72), dict(flags=_lib.POSE_DISCARD))
    bad = (dict(n_frames=-1), dict(cap=0), dict(cap=_lib.POSE_MAX_ROWS + 1), dict(p_cap=0), dict(shift=-1), dict(stride=8), dict(stride=13),
           dict(flags=2), dict(flags=-1), dict(keys=0x1002), dict(points=0x1001), dict(res=0x1002))
    bad += tuple({k: None} for k in ("keys", "n", "assigned", "points", "n_points", "cam", "T", "res", "out"))
    for kw in good:
        assert f(*_batch_args(**kw)) == accepted, kw
    for kw in bad:
        assert f(*_batch_args(**kw)) == _lib.ERR_INVALID, kw
        assert b"pose optimisation" in L.orbfe_last_error()
    if not _gpu_present(L):
        assert f(*_batch_args(n_frames=3)) == _lib.ERR_NO_DEVICE and b"no CPU fallback" in L.orbfe_last_error()
