"""CPU: (1) the cases of tests/np_lba.py are parity cases -- on the reading alone; (2) csrc/lba_internal.h compiled for the host
(tests/cpp_lba/host_arith.cpp) against the reading by the parity criterion of tests/test_lba_gpu.py; (3) every limit of
orbfe_local_bundle_adjustment* is refused one step past its boundary, before any device is looked for."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from refactored_orb_slam2_amd._lib import LBA_EDGE_DTYPE, LBA_RESULT_DTYPE
from tests import np_lba as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_lba", "_build", "liblba_host.so")
NOISE = 4.0 * 2.0 ** -52     # a few ulp of double on every summand


@functools.lru_cache(maxsize=None)
def _runs(name):
    s = Q.case_scene(name)
    return [Q.reference(name), Q.run_scene(s, solve="full")] + [Q.run_scene(s, order_seed=seed, noise=NOISE) for seed in (1, 2, 3)]


@pytest.mark.parametrize("name", list(Q.CASES))
def test_the_case_is_a_parity_case(name):
    s = Q.case_scene(name)
    runs = _runs(name)
    a = runs[0]
    free = np.asarray(s["fixed"]) == 0
    seen = np.zeros(len(s["points"]), bool)
    seen[s["edges"]["point"]] = True
    worst = max(Q.worst_ratio(r["poses"], r["points"], a["poses"], a["points"]) for r in runs[1:])
    print(f"{name}: {len(s['edges'])} edges, rounds {a['rounds']}, iterations {a['iterations']}, trials {a['trials']}, dropped {a['n_dropped']}, "
          f"erase {a['n_erase']}, margin {a['margin']:.3e}, runs against run A {worst:.4f} of the tolerance")
    # what the name promises
    want_rounds = 0 if name in ("edges_0", "no_free") else (1 if name == "first_round_only" else 2)
    assert a["rounds"] == want_rounds
    if name == "clean":
        assert a["n_dropped"] == 0 and a["n_erase"] == 0
    if name == "outliers_30":
        assert (free & ~a["active_kf"]).any() and (seen & ~a["active_pt"]).any()
    if name == "rejected_step":
        assert not all(a["accepts"][0] + a["accepts"][1])
    if name == "behind":
        P = Q._Problem(a["poses"], s["fixed"], a["points"], s["edges"], s["cam"])
        z = P.camera_points()[2]
        chi2 = P.errors()[1]
        assert ((z <= 0) & (chi2 <= P.th) & (a["erase"] != 0)).any()
    if name == "all_mono":
        assert (s["edges"]["u_right"] < 0).all() and int((s["fixed"] != 0).sum()) >= 2
    if name == "all_stereo":
        assert not (s["edges"]["u_right"] < 0).any()
    if name == "kf0_local":
        assert s["fixed"][int(np.flatnonzero(s["fixed"] == 0)[0]) - 1] != 0 and int((s["fixed"] != 0).sum()) == 4
    if name == "free_11":
        assert int(free.sum()) == 11
    if name == "points_1100":
        assert len(s["points"]) == 1100 and len(s["edges"]) > 2048
    if name == "standard":
        assert a["n_dropped"] > 0 and (s["edges"]["u_right"] < 0).any() and not (s["edges"]["u_right"] < 0).all()
    # every run decides alike, and agrees with run A within half the parity tolerance
    for r in runs[1:]:
        assert np.array_equal(r["dropped"], a["dropped"]) and np.array_equal(r["erase"], a["erase"]) and r["rounds"] == a["rounds"]
        assert r["accepts"] == a["accepts"]
    assert a["margin"] >= 1e-6
    assert worst <= 0.5


# ---- lba_internal.h on the host --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_lba"), "_build/liblba_host.so"], check=True, capture_output=True)
    return C.CDLL(HOST_LIB)


def _camera(s):
    c = s["cam"]
    return optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], [1.0])


def _host(H, s, edges=None):
    edges = np.ascontiguousarray(s["edges"] if edges is None else edges, LBA_EDGE_DTYPE)
    cam = _camera(s)
    poses, points = np.ascontiguousarray(s["poses"]), np.ascontiguousarray(s["points"])
    fixed = np.ascontiguousarray(s["fixed"])
    po, xo = np.zeros_like(poses), np.zeros_like(points)
    er, res = np.zeros(len(edges), np.uint8), np.zeros(1, LBA_RESULT_DTYPE)
    rc = H.lba_host(_lib.ptr(cam), _lib.ptr(poses), _lib.ptr(fixed), len(poses), _lib.ptr(points), len(points), _lib.ptr(edges), len(edges),
                    int(s["flags"]), _lib.ptr(po), _lib.ptr(xo), _lib.ptr(er), _lib.ptr(res))
    return rc, po, xo, er, res[0]


def test_record_layouts(H):
    out = np.zeros(5, np.int32)
    H.lba_host_sizes(_lib.ptr(out))
    assert out.tolist() == [LBA_EDGE_DTYPE.itemsize, _lib.LBA_PROBLEM_DTYPE.itemsize, LBA_RESULT_DTYPE.itemsize,
                            LBA_RESULT_DTYPE.fields["chi2_first"][1], LBA_RESULT_DTYPE.fields["n_dropped"][1]]


@pytest.mark.parametrize("name", list(Q.CASES))
def test_host_arithmetic_against_the_reading(H, name):
    s, ref = Q.case_scene(name), Q.reference(name)
    rc, poses, points, erase, res = _host(H, s)
    ratio = Q.worst_ratio(poses, points, ref["poses"], ref["points"])
    not_equal = int((poses.view(np.uint32) != ref["poses"].view(np.uint32)).sum() + (points.view(np.uint32) != ref["points"].view(np.uint32)).sum())
    print(f"lba host arithmetic {name}: max diff / tolerance {ratio:.4f}, floats not bit-equal {not_equal}/{poses.size + points.size}, rounds "
          f"{int(res['rounds'])}/{ref['rounds']}, n_dropped {int(res['n_dropped'])}/{ref['n_dropped']}, n_erase {int(res['n_erase'])}/"
          f"{ref['n_erase']}, iterations {res['iterations'].tolist()} (reading {ref['iterations']}), trials {res['trials'].tolist()} (reading "
          f"{ref['trials']})")
    assert rc == 0
    assert np.array_equal(erase & _lib.LBA_ERASE, ref["erase"]) and np.array_equal((erase & _lib.LBA_DROPPED) >> 1, ref["dropped"])
    assert (int(res["rounds"]), int(res["n_dropped"]), int(res["n_erase"])) == (ref["rounds"], ref["n_dropped"], ref["n_erase"])
    fixed = np.asarray(s["fixed"]) != 0
    assert poses[fixed].tobytes() == s["poses"][fixed].tobytes()
    seen = np.zeros(len(s["points"]), bool)
    seen[s["edges"]["point"]] = True
    assert points[~seen].tobytes() == s["points"][~seen].tobytes()
    assert ratio <= 1.0


def test_host_arithmetic_refuses_what_the_device_form_refuses(H):
    s = Q.case_scene("one_free")
    for kind in range(3):
        e = s["edges"].copy()
        if kind == 0:
            e[[2, 3]] = e[[3, 2]]                    # out of (point, keyframe) order
        elif kind == 1:
            e[3] = e[2]                              # the same pair twice
        else:
            e["inv_sigma2"][1] = np.inf
        rc, poses, points, erase, res = _host(H, s, e)
        assert rc == -1 and int(res["rounds"]) == -1 and poses.tobytes() == s["poses"].tobytes() and not erase.any()


# ---- the limits: refused before a device is looked for -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _call(L, n_kf, n_free, n_points, n_edges, flags=0, edit=None, null=None):
    """orbfe_local_bundle_adjustment on a well-formed problem of these counts (edges: point i % n_points, keyframe spread)"""
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
                erase=np.zeros(len(edges), np.uint8), res=np.zeros(1, LBA_RESULT_DTYPE))
    p = {k: (None if k == null else _lib.ptr(v)) for k, v in args.items()}
    return L.orbfe_local_bundle_adjustment(p["cam"], p["poses"], p["fixed"], n_kf, p["points"], n_points, p["edges"], n_edges, flags,
                                           p["poses_out"], p["points_out"], p["erase"], p["res"])


def _accepted(L):
    n = C.c_int(0)
    gpu = L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    return _lib.OK if gpu else _lib.ERR_NO_DEVICE


def test_limits_of_the_host_form(L):
    ok = _accepted(L)
    F, K, NP, NE = _lib.LBA_MAX_FREE, _lib.LBA_MAX_KEYFRAMES, _lib.LBA_MAX_POINTS, _lib.LBA_MAX_EDGES
    assert _call(L, F + 2, F, 40, 400) == ok                          # the largest number of free keyframes
    assert _call(L, F + 2, F + 1, 40, 400) == _lib.ERR_INVALID
    assert b"free keyframes" in L.orbfe_last_error()
    assert _call(L, K, 4, 40, 400) == ok                              # keyframes in all
    assert _call(L, K + 1, 4, 40, 400) == _lib.ERR_INVALID
    assert _call(L, 8, 4, NP, 400) == ok                              # points
    assert _call(L, 8, 4, NP + 1, 400) == _lib.ERR_INVALID
    assert _call(L, 8, 4, NP, NE) == ok                               # edges: 65 535 x 4
    assert _call(L, 8, 4, NP, NE + 1) == _lib.ERR_INVALID
    for n in ((-1, 0, 4, 4), (4, 2, -1, 4), (4, 2, 4, -1)):
        assert _call(L, *n) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, flags=_lib.LBA_FIRST_ROUND_ONLY) == ok
    assert _call(L, 8, 4, 40, 160, flags=2) == _lib.ERR_INVALID


def test_edge_rules_of_the_host_form(L):
    ok = _accepted(L)

    def field(name, row, value):
        def edit(e):
            e[name][row] = value
        return edit
    assert _call(L, 8, 4, 40, 160, edit=field("kf", 7, 7)) == ok
    assert _call(L, 8, 4, 40, 160, edit=field("kf", 7, 8)) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, edit=field("kf", 7, -1)) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 41, 160, edit=field("point", 150, 40)) == ok
    assert _call(L, 8, 4, 40, 160, edit=field("point", 150, 40)) == _lib.ERR_INVALID
    assert _call(L, 8, 4, 40, 160, edit=field("point", 150, -1)) == _lib.ERR_INVALID
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    assert _call(L, 8, 4, 40, 160, edit=field("inv_sigma2", 3, tiny)) == ok
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert _call(L, 8, 4, 40, 160, edit=field("inv_sigma2", 3, bad)) == _lib.ERR_INVALID, bad
    assert _call(L, 8, 4, 40, 160, edit=field("kf", 40, 0)) == _lib.ERR_INVALID             # (keyframe 0, point 0) twice
    assert b"same keyframe" in L.orbfe_last_error()
    for null in ("cam", "res", "poses", "fixed", "points", "edges", "poses_out", "points_out", "erase"):
        assert _call(L, 8, 4, 40, 160, null=null) == _lib.ERR_INVALID, null


def test_limits_of_the_workspace_query_and_the_batch_form(L):
    ok = _accepted(L)
    F, K, NP, NE, PR = _lib.LBA_MAX_FREE, _lib.LBA_MAX_KEYFRAMES, _lib.LBA_MAX_POINTS, _lib.LBA_MAX_EDGES, _lib.LBA_MAX_PROBLEMS
    n = C.c_size_t(0)
    assert L.orbfe_lba_workspace_bytes(PR, K, NP, NE, C.byref(n)) == _lib.OK and n.value > 0
    for bad in ((PR + 1, K, NP, NE), (1, K + 1, NP, NE), (1, K, NP + 1, NE), (1, K, NP, NE + 1), (-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1),
                (1, 1, 1, -1)):
        assert L.orbfe_lba_workspace_bytes(*bad, C.byref(n)) == _lib.ERR_INVALID, bad
    assert L.orbfe_lba_workspace_bytes(1, 1, 1, 1, None) == _lib.ERR_INVALID
    # the reduced system grows with the free keyframes up to the cap, not beyond it
    assert optimizer.lba_workspace_bytes(1, F + 1, 10, 10) == optimizer.lba_workspace_bytes(1, F, 10, 10) > optimizer.lba_workspace_bytes(1, F - 1, 10, 10)
    assert optimizer.lba_workspace_bytes(3, 9, 300, 1300) == 3 * optimizer.lba_workspace_bytes(1, 9, 300, 1300)
    need = optimizer.lba_workspace_bytes(2, 8, 40, 160)
    buf = np.zeros(need + 512, np.uint8)
    base = (buf.ctypes.data + 255) & ~255                                  # host memory stands in: nothing is launched without a device

    def batch(P=2, caps=(8, 40, 160), stride=12, flags=0, ws=base, ws_bytes=need, null=None, off=None):
        a = [0x1000 + 0x100 * k for k in range(10)]                        # aligned stand-ins; refused calls never read them
        if null is not None:
            a[null] = None
        if off is not None:
            a[off] += 2
        return L.orbfe_local_bundle_adjustment_batch_device(P, a[0], a[1], a[2], a[3], a[4], stride, a[5], *caps, flags, a[6], a[7], a[8], a[9],
                                                            ws, ws_bytes, None)
    if ok == _lib.ERR_NO_DEVICE:
        assert batch() == ok                                               # valid arguments: refused only for want of a device
    assert batch(P=0) == ok
    assert batch(P=PR + 1) == _lib.ERR_INVALID and batch(P=-1) == _lib.ERR_INVALID
    assert batch(caps=(K + 1, 40, 160)) == _lib.ERR_INVALID and batch(caps=(8, NP + 1, 160)) == _lib.ERR_INVALID
    assert batch(caps=(8, 40, NE + 1)) == _lib.ERR_INVALID
    assert batch(stride=8) == _lib.ERR_INVALID and batch(stride=14) == _lib.ERR_INVALID
    assert batch(flags=4) == _lib.ERR_INVALID
    assert batch(ws_bytes=need - 1) == _lib.ERR_INVALID and batch(ws=base + 8) == _lib.ERR_INVALID and batch(ws=None) == _lib.ERR_INVALID
    for k in range(10):
        assert batch(null=k) == _lib.ERR_INVALID, k
    for k in (0, 1, 2, 4, 5, 6, 7, 9):
        assert batch(off=k) == _lib.ERR_INVALID, k
