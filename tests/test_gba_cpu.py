"""CPU: the global bundle adjustment across the device (orbfe_global_bundle_adjustment, orbfe_gba_workspace_bytes,
orbfe_global_bundle_adjustment_device) as far as it can be checked without one.

(1) Every scene of tests/np_gba.py is a parity case under the reading (tests/np_ba.optimize), by the conditions of
    tests/test_ba_cpu.py: the Schur solve, the full solve and three runs with permuted edges and 4 ulp of noise take every accept
    alike, and agree within half the parity tolerance.  tests/test_gba_gpu.py compares the device against the same reading.
(2) The three exports, the constants of the header and their mirror in _lib.
(3) Every limit refused one step past its boundary and accepted at it, before a device is looked for."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from refactored_orb_slam2_amd._lib import BA_RESULT_DTYPE, LBA_EDGE_DTYPE
from tests import np_ba as B
from tests import np_gba as G

NOISE = 4 * 2.0 ** -52
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbfe.h")


# ---- (1) the cases -----------------------------------------------------------------------------------------------------------------
def _five_runs(s):
    return [B.run_scene(s), B.run_scene(s, solve="full")] + [B.run_scene(s, order_seed=seed, noise=NOISE) for seed in (1, 2, 3)]


@pytest.mark.parametrize("name", list(G.CASES))
def test_the_case_is_a_parity_case(name):
    s = G.case_scene(name)
    seed, n_free, n_fixed, long, n_it, robust = G.CASES[name]
    runs = [G.reference(name)] + _five_runs(s)[1:]
    a = runs[0]
    worst = max(B.worst_ratio(r["poses"], r["points"], a["poses"], a["points"]) for r in runs[1:])
    print(f"{name}: {len(s['poses'])} keyframes, {len(s['points'])} points, {len(s['edges'])} edges, long tracks {s.get('n_long', 0)}, "
          f"iterations {a['iterations']} of {n_it}, trials {a['trials']}, rejected {a['accepts'].count(False)}, chi2 {a['chi2_first']:.6g} -> "
          f"{a['chi2_final']:.6g}, runs against run A {worst:.4f} of the tolerance")
    assert int((s["fixed"] == 0).sum()) == n_free > _lib.LBA_MAX_FREE and len(s["points"]) == 5 * n_free
    assert a["rounds"] == 1 and a["iterations"] == n_it
    e = s["edges"]
    assert np.all((e["point"][1:] > e["point"][:-1]) | ((e["point"][1:] == e["point"][:-1]) & (e["kf"][1:] > e["kf"][:-1])))
    if long:                                   # blocks far off the band: a point whose observers lie at least 10 rows apart
        assert s["n_long"] >= 10
        span = np.zeros(len(s["points"]), int)
        np.maximum.at(span, e["point"], e["kf"])
        lo = np.full(len(s["points"]), 1 << 30)
        np.minimum.at(lo, e["point"], e["kf"])
        assert int(((span - lo) >= 10).sum()) >= s["n_long"]
    else:
        assert all(a["accepts"])               # no rejected trial
    if name == "past_256":
        assert len(s["poses"]) > _lib.LBA_MAX_KEYFRAMES
    for r in runs[1:]:
        assert r["accepts"] == a["accepts"] and r["rounds"] == a["rounds"] and r["iterations"] == a["iterations"]
    assert worst <= 0.5


def test_the_nan_scene_rejects_every_trial_in_every_run():
    s = G.nan_scene()
    runs = _five_runs(s)
    for r in runs:
        assert (r["iterations"], r["trials"]) == (4, 4) and not any(r["accepts"]) and np.isnan(r["chi2_final"])
        assert B.worst_ratio(r["poses"], r["points"], runs[0]["poses"], runs[0]["points"]) <= 0.5


def test_the_tile_cases_stand_on_the_edges_of_the_tile():
    T = _lib.GBA_TILE_KEYFRAMES
    m = next(m for m in range(1, 1000) if m * T - 1 > _lib.LBA_MAX_FREE)
    assert [G.CASES[f"tile_{n}"][1] for n in (m * T - 1, m * T, m * T + 1)] == [m * T - 1, m * T, m * T + 1]


# ---- (2) exports and constants -----------------------------------------------------------------------------------------------------
def test_exports_and_constants():
    text = open(HEADER).read()
    for name, value in (("ORBFE_GBA_MAX_KEYFRAMES", _lib.GBA_MAX_KEYFRAMES), ("ORBFE_GBA_MAX_POINTS", _lib.GBA_MAX_POINTS),
                        ("ORBFE_GBA_MAX_EDGES", _lib.GBA_MAX_EDGES), ("ORBFE_GBA_TILE_KEYFRAMES", _lib.GBA_TILE_KEYFRAMES)):
        m = re.search(rf"^#define {name} (\d+)$", text, re.M)
        assert m and int(m.group(1)) == value, name
        assert re.search(rf"^ \*   {name} ", text, re.M), f"{name}: no row in the limits table"
    assert (_lib.GBA_MAX_KEYFRAMES, _lib.GBA_MAX_POINTS, _lib.GBA_MAX_EDGES) == (2048, 1048575, 8388600)
    L = _lib.lib()
    for f in ("orbfe_global_bundle_adjustment", "orbfe_gba_workspace_bytes", "orbfe_global_bundle_adjustment_device"):
        assert f in _lib.EXPORTS and getattr(L, f).argtypes and re.search(rf"^int {f}\(", text, re.M), f
    assert "SYNCHRONOUS" in text[text.index("ORBFE_GBA_MAX_KEYFRAMES"):]
    for f in ("global_bundle_adjustment", "global_bundle_adjustment_device", "gba_workspace_bytes"):
        assert callable(getattr(optimizer, f))


# ---- (3) limits --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _accepted(L):
    n = C.c_int(0)
    gpu = L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    return _lib.OK if gpu else _lib.ERR_NO_DEVICE


def _call(L, n_kf, n_free, n_points, n_edges, n_iterations=2, flags=1, edit=None, null=None):
    """orbfe_global_bundle_adjustment on a well-formed problem of these counts (edges: point i % n_points, keyframe spread)"""
    cam = optimizer.pose_camera(700.0, 700.0, 600.0, 180.0, 380.0, [1.0])
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (max(n_kf, 1), 1))
    fixed = np.ones(max(n_kf, 1), np.uint8)
    fixed[:n_free] = 0
    points = np.ones((max(n_points, 1), 3), np.float32)
    edges = np.zeros(max(n_edges, 1), LBA_EDGE_DTYPE)
    i = np.arange(max(n_edges, 1))
    edges["point"], edges["kf"] = i % max(n_points, 1), (i // max(n_points, 1)) % max(n_kf, 1)
    edges["u"], edges["v"], edges["u_right"], edges["inv_sigma2"] = 600, 180, -1, 1
    if edit:
        edit(edges)
    args = dict(cam=cam, poses=poses, fixed=fixed, points=points, edges=edges, poses_out=np.zeros_like(poses), points_out=np.zeros_like(points),
                res=np.zeros(1, BA_RESULT_DTYPE))
    p = {k: (None if k == null else _lib.ptr(v)) for k, v in args.items()}
    return L.orbfe_global_bundle_adjustment(p["cam"], p["poses"], p["fixed"], n_kf, p["points"], n_points, p["edges"], n_edges, n_iterations,
                                            flags, p["poses_out"], p["points_out"], p["res"])


def test_limits_of_the_host_form(L):
    ok = _accepted(L)
    K, NP, NE, IT = _lib.GBA_MAX_KEYFRAMES, _lib.GBA_MAX_POINTS, _lib.GBA_MAX_EDGES, _lib.BA_MAX_ITERATIONS
    assert _call(L, _lib.LBA_MAX_FREE + 2, _lib.LBA_MAX_FREE + 1, 40, 400) == ok      # what orbfe_bundle_adjustment refuses
    assert _call(L, K, 4, 40, 400) == ok and _call(L, K + 1, 4, 40, 400) == _lib.ERR_INVALID
    assert b"global bundle adjustment" in L.orbfe_last_error() and b"n_kf" in L.orbfe_last_error()
    assert _call(L, 8, 4, NP, 400) == ok and _call(L, 8, 4, NP + 1, 400) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, NE + 1) == _lib.ERR_INVALID
    for n in ((-1, 0, 4, 4), (4, 2, -1, 4), (4, 2, 4, -1)):
        assert _call(L, *n) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, n_iterations=1) == ok and _call(L, 8, 4, 40, 160, n_iterations=0) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, n_iterations=IT) == ok and _call(L, 8, 4, 40, 160, n_iterations=IT + 1) == _lib.ERR_INVALID
    assert b"n_iterations" in L.orbfe_last_error()
    assert _call(L, 8, 4, 40, 160, flags=0) == ok and _call(L, 8, 4, 40, 160, flags=2) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, edit=lambda e: e["kf"].__setitem__(7, 8)) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, edit=lambda e: e["inv_sigma2"].__setitem__(3, np.nan)) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, edit=lambda e: e["kf"].__setitem__(40, 0)) == _lib.ERR_INVALID            # (keyframe 0, point 0) twice
    assert b"same keyframe" in L.orbfe_last_error()
    for null in ("cam", "res", "poses", "fixed", "points", "edges", "poses_out", "points_out"):
        assert _call(L, 8, 4, 40, 160, null=null) == _lib.ERR_INVALID, null


def test_limits_of_the_device_form(L):
    ok = _accepted(L)
    K, NP, NE, IT = _lib.GBA_MAX_KEYFRAMES, _lib.GBA_MAX_POINTS, _lib.GBA_MAX_EDGES, _lib.BA_MAX_ITERATIONS
    need = optimizer.gba_workspace_bytes(8, 40, 160)
    buf = np.zeros(need + 512, np.uint8)
    base = (buf.ctypes.data + 255) & ~255                                  # host memory stands in: nothing is launched without a device

    def dev(counts=(8, 40, 160), stride=12, n_it=20, flags=1, ws=base, ws_bytes=need, null=None, off=None):
        a = [0x1000 + 0x100 * k for k in range(8)]                         # aligned stand-ins; refused calls never read them
        if null is not None:
            a[null] = None
        if off is not None:
            a[off] += 2
        return L.orbfe_global_bundle_adjustment_device(a[0], a[1], a[2], counts[0], a[3], stride, counts[1], a[4], counts[2], n_it, flags,
                                                       a[5], a[6], a[7], ws, ws_bytes, None)
    big = 1 << 40                                                          # a size nobody allocates: the caps are checked on the counts
    if ok == _lib.ERR_NO_DEVICE:
        assert dev() == ok                                                 # valid arguments: refused only for want of a device
        assert b"no CPU fallback" in L.orbfe_last_error()
        assert dev(stride=44) == ok and dev(n_it=1) == ok and dev(flags=0) == ok
        assert dev(counts=(K, NP, NE), ws_bytes=big) == ok                 # every count AT its cap
    for counts in ((K + 1, 40, 160), (8, NP + 1, 160), (8, 40, NE + 1), (-1, 40, 160), (8, -1, 160), (8, 40, -1)):
        assert dev(counts=counts, ws_bytes=big) == _lib.ERR_INVALID, counts
    assert dev(n_it=0) == _lib.ERR_INVALID and dev(n_it=IT + 1) == _lib.ERR_INVALID
    assert dev(flags=2) == _lib.ERR_INVALID
    assert dev(stride=8) == _lib.ERR_INVALID and dev(stride=14) == _lib.ERR_INVALID
    assert dev(ws_bytes=need - 1) == _lib.ERR_INVALID and dev(ws=base + 8) == _lib.ERR_INVALID and dev(ws=None) == _lib.ERR_INVALID
    for null in range(8):
        assert dev(null=null) == _lib.ERR_INVALID, null
    for off in (0, 1, 3, 4, 5, 6, 7):
        assert dev(off=off) == _lib.ERR_INVALID, off


def test_workspace_bytes_at_the_caps():
    K, NP, NE = _lib.GBA_MAX_KEYFRAMES, _lib.GBA_MAX_POINTS, _lib.GBA_MAX_EDGES
    top = optimizer.gba_workspace_bytes(K, NP, NE)
    # by hand, in Python's integers: the reduced system, the per-point and the per-edge doubles alone
    floor = 8 * (36 * K * K + 33 * NP + 64 * NE)
    print(f"workspace at the caps: {top} bytes ({top / 2 ** 30:.2f} GiB), at least {floor}")
    assert floor <= top < floor + (1 << 28) and top > 1 << 32 and top % 256 == 0
    for a, b in (((K - 1, NP, NE), (K, NP, NE)), ((K, NP - 1, NE), (K, NP, NE)), ((K, NP, NE - 4096), (K, NP, NE)), ((0, 0, 0), (1, 0, 0)),
                 ((1, 0, 0), (1, 1, 0)), ((1, 1, 0), (1, 1, 1)), ((64, 1000, 5000), (65, 1000, 5000)), ((64, 1000, 5000), (64, 1001, 5000)),
                 ((64, 1000, 5000), (64, 1000, 5001))):
        assert optimizer.gba_workspace_bytes(*a) <= optimizer.gba_workspace_bytes(*b), (a, b)
    assert optimizer.gba_workspace_bytes(K - 1, NP, NE) < top and optimizer.gba_workspace_bytes(K, NP // 2, NE) < top
    assert optimizer.gba_workspace_bytes(K, NP, NE // 2) < top
    for bad in ((K + 1, 0, 0), (0, NP + 1, 0), (0, 0, NE + 1), (-1, 0, 0)):
        with pytest.raises(_lib.OrbfeError) as ei:
            optimizer.gba_workspace_bytes(*bad)
        assert ei.value.code == _lib.ERR_INVALID
    assert _lib.lib().orbfe_gba_workspace_bytes(1, 1, 1, None) == _lib.ERR_INVALID


def test_the_one_workgroup_form_still_refuses_65_free_keyframes(L):
    s = B.make_scene(6500, n_free=_lib.LBA_MAX_FREE + 1, n_points=20)
    with pytest.raises(_lib.OrbfeError) as ei:
        optimizer.bundle_adjustment(optimizer.pose_camera(700.0, 700.0, 600.0, 180.0, 380.0, [1.0]), s["poses"], s["fixed"], s["points"],
                                    s["edges"], 2, True)
    assert ei.value.code == _lib.ERR_INVALID and b"free keyframes" in L.orbfe_last_error()
