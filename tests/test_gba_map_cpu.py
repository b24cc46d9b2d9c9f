"""The map update behind the global bundle adjustment (orbfe_gba_update_map / _device, LoopClosing::RunGlobalBundleAdjustment's block
L/src/LoopClosing.cc:648-703) without a GPU: the two readings of tests/np_gba_map.py agree to the byte on every scene, csrc/gba_map_internal.h
compiled for the host (tests/cpp_gba_map/host_arith.cpp) reproduces those bytes, every limit is refused one step past it and every
null / misaligned / aliased argument is refused before a device is looked for, a valid call without a device is an error, and the
struct sizes are what include/orbfe.h states."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from tests import np_gba_map as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp_gba_map", "_build", "libgba_map_host.so")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_gba_map")], check=True, capture_output=True)
    return C.CDLL(HOST)


def _gpu(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def _same(a, b):
    (ka, xa, ra), (kb, xb, rb) = a, b
    return ka.tobytes() == kb.tobytes() and xa.tobytes() == xb.tobytes() and ra == rb


@pytest.mark.parametrize("name", sorted(M.SCENES))
def test_the_two_readings_agree_to_the_byte(name):
    s = M.scene(name)
    lit, rul = M.literal(s), M.reading(name)
    assert lit[0].tobytes() == rul[0].tobytes() and lit[1].tobytes() == rul[1].tobytes() and lit[2] == rul[2]


def test_the_scenes_hold_what_they_are_for():
    """every kind of keyframe and of point is there, and the counts are the ones the scenes were built for"""
    r = {name: M.reading(name)[2] for name in M.SCENES}
    assert r["single"] == dict(n_optimised=1, n_propagated=0, n_unreached=0, n_taken=0, n_moved=0, n_left=0, rounds=0)
    for n in (1, 2, 63, 64, 65, 1025):
        assert (r[f"chain_{n}"]["n_propagated"], r[f"chain_{n}"]["rounds"]) == (n, n)
    assert (r["fan_1025"]["n_propagated"], r["fan_1025"]["rounds"]) == (1025, 1)
    assert (r["two_origins"]["n_optimised"], r["two_origins"]["n_propagated"], r["two_origins"]["rounds"]) == (2, 5, 2)
    m = r["mixed"]
    assert m["n_optimised"] == 10 and m["n_unreached"] == 6 and m["n_propagated"] == 21 and m["rounds"] == 5
    assert min(m["n_taken"], m["n_moved"], m["n_left"]) > 0
    kf, _, _ = M.reading("mixed")
    s = M.scene("mixed")
    carried = (s["point_gba_row"] < 0) & (s["ref"] >= 0)
    assert (kf["status"][s["ref"][carried]] == M.UNREACHED).any()          # points whose reference keyframe is unreached
    assert r["unoptimised_origin"]["n_unreached"] == 3 and r["cycle"]["n_unreached"] == 2
    assert (s["parent"][s["parent"] >= 0] > np.flatnonzero(s["parent"] >= 0)).any()   # a parent's row behind its child's


def _host_update(host, s):
    n, m = len(s["poses"]), len(s["points"])
    kf = np.zeros(n, M.KEYFRAME_DTYPE)
    out = np.zeros((m, 3), np.float32)
    res = np.zeros(1, _lib.GBA_MAP_RESULT_DTYPE)
    p = _lib.ptr
    host.gba_map_host_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    host.gba_map_host_update(p(s["poses"]), p(s["parent"]), p(s["kf_gba_row"]), n, p(s["gba_poses"]), len(s["gba_poses"]),
                             float(s["half_baseline"]), p(s["points"]), p(s["point_gba_row"]), p(s["ref"]), m, p(s["gba_points"]),
                             len(s["gba_points"]), p(kf), p(out), p(res))
    return kf, out, {f: int(res[0][f]) for f in M.RESULT_FIELDS}


@pytest.mark.parametrize("name", sorted(M.SCENES))
def test_the_header_compiled_for_the_host_gives_the_readings_bytes(host, name):
    assert _same(_host_update(host, M.scene(name)), M.reading(name))


def test_the_header_on_rows_out_of_range(host):
    s = M.out_of_range_scene()
    assert _same(_host_update(host, s), M.rule(s))


def test_set_pose_and_the_product_alone(host):
    """the two primitives on poses with signed zeros and a NaN: a term times zero is added, not dropped"""
    rng = np.random.default_rng(5)
    A, B = M._poses(rng, 64), M._poses(rng, 64)
    A[0, 3], B[0, :] = np.float32(-0.0), np.float32(-0.0)
    A[1, 7] = np.nan
    A[2, :3], A[2, 3] = np.float32(-0.0), np.float32(0.0)
    Cm, Twc, Cw = np.zeros_like(A), np.zeros_like(A), np.zeros((64, 3), np.float32)
    host.gba_map_host_mul(_lib.ptr(A), _lib.ptr(B), 64, _lib.ptr(Cm))
    host.gba_map_host_set_pose.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    host.gba_map_host_set_pose(_lib.ptr(A), 64, 0.2685, _lib.ptr(Twc), _lib.ptr(Cw))
    with np.errstate(invalid="ignore"):
        want = M.mul(A, B)
        wT, wC = M.set_pose(A, 0.2685)
    nan = np.isnan(want)
    assert nan[1, 4:8].all() and (np.isnan(Cm) == nan).all() and Cm[~nan].tobytes() == want[~nan].tobytes()
    nan = np.isnan(wT)
    assert (np.isnan(Twc) == nan).all() and Twc[~nan].tobytes() == wT[~nan].tobytes()
    assert (np.isnan(Cw) == np.isnan(wC)).all() and Cw[~np.isnan(wC)].tobytes() == wC[~np.isnan(wC)].tobytes()


def test_struct_sizes():
    assert _lib.GBA_MAP_KEYFRAME_DTYPE.itemsize == 112 and _lib.GBA_MAP_RESULT_DTYPE.itemsize == 32
    assert _lib.GBA_MAP_KEYFRAME_DTYPE == M.KEYFRAME_DTYPE
    assert tuple(_lib.GBA_MAP_RESULT_DTYPE.names[:7]) == M.RESULT_FIELDS
    txt = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    assert int(re.search(r"#define ORBFE_GBA_MAP_MAX_KEYFRAMES (\d+)", txt).group(1)) == _lib.GBA_MAP_MAX_KEYFRAMES == 65536
    assert int(re.search(r"#define ORBFE_GBA_MAP_MAX_POINTS (\d+)", txt).group(1)) == _lib.GBA_MAP_MAX_POINTS == 16777216
    assert _lib.GBA_MAP_MAX_KEYFRAMES >= 2 * _lib.GBA_MAX_KEYFRAMES
    for k, name in enumerate(("OPTIMISED", "PROPAGATED", "UNREACHED")):
        assert int(re.search(rf"#define ORBFE_GBA_MAP_KF_{name} (\d+)", txt).group(1)) == getattr(_lib, "GBA_MAP_KF_" + name) == k


# ---- validation: everything below returns before a device is looked for
ARGS = ("poses", "parent", "kf_gba_row", "n_kf", "gba_poses", "n_gba_kf", "hb", "points", "point_gba_row", "ref", "n_points", "gba_points",
        "n_gba_points", "kf_out", "points_out", "result")
DEV_ARGS = ARGS[:8] + ("stride",) + ARGS[8:] + ("stream",)


def _args(s):
    """the arguments of the host form as a dict of name -> value, with outputs of the right size"""
    a = dict(poses=s["poses"], parent=s["parent"], kf_gba_row=s["kf_gba_row"], n_kf=len(s["poses"]), gba_poses=s["gba_poses"],
             n_gba_kf=len(s["gba_poses"]), hb=float(s["half_baseline"]), points=s["points"], point_gba_row=s["point_gba_row"], ref=s["ref"],
             n_points=len(s["points"]), gba_points=s["gba_points"], n_gba_points=len(s["gba_points"]),
             kf_out=np.zeros(len(s["poses"]), M.KEYFRAME_DTYPE), points_out=np.zeros((len(s["points"]), 3), np.float32),
             result=np.zeros(1, _lib.GBA_MAP_RESULT_DTYPE), stride=12, stream=None)
    return a


def _v(x):
    return _lib.ptr(x) if isinstance(x, np.ndarray) else x


def _call(L, a, device=False):
    if device:
        return L.orbfe_gba_update_map_device(*[_v(a[k]) for k in DEV_ARGS])
    return L.orbfe_gba_update_map(*[_v(a[k]) for k in ARGS])


def _off(x, nbytes):
    """a pointer nbytes into x"""
    return C.c_void_p(x.ctypes.data + nbytes)


@pytest.mark.parametrize("device", [False, True])
def test_limits_nulls_alignment_and_aliasing_are_refused_before_a_device_is_looked_for(L, device):
    inv = _lib.ERR_INVALID
    ok = _lib.OK if _gpu(L) else _lib.ERR_NO_DEVICE
    s = M.scene("chain_2")
    one = C.c_void_p(1 << 20)           # never read: every call below is refused
    base = _args(s)
    # the limits, one step past each
    for key, over in (("n_kf", _lib.GBA_MAP_MAX_KEYFRAMES + 1), ("n_gba_kf", _lib.GBA_MAP_MAX_KEYFRAMES + 1),
                      ("n_points", _lib.GBA_MAP_MAX_POINTS + 1), ("n_gba_points", _lib.GBA_MAP_MAX_POINTS + 1), ("n_kf", -1),
                      ("n_gba_kf", -1), ("n_points", -1), ("n_gba_points", -1)):
        a = {k: (one if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        a["kf_out"], a["points_out"], a["result"] = C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
        a[key] = over
        assert _call(L, a, device) == inv, (key, over)
    # null arrays with a count > 0, and a null result
    for key in ("poses", "parent", "kf_gba_row", "gba_poses", "points", "point_gba_row", "ref", "gba_points", "kf_out", "points_out",
                "result"):
        a = dict(base)
        a[key] = None
        assert _call(L, a, device) == inv, key
    # misaligned arrays: two bytes into a 4-byte array, four bytes into the 8-byte one
    big = {k: np.zeros(v.nbytes + 16, np.uint8) for k, v in base.items() if isinstance(v, np.ndarray)}
    for key in big:
        a = dict(base)
        a[key] = _off(big[key], 4 if key == "kf_out" else 2)
        assert _call(L, a, device) == inv, key
    # an output that is an input, and two outputs that are one array
    for out in ("kf_out", "points_out", "result"):
        for other in ("poses", "parent", "kf_gba_row", "gba_poses", "points", "point_gba_row", "ref", "gba_points", "kf_out", "points_out",
                      "result"):
            if other == out:
                continue
            a = dict(base)
            a[out] = a[other] = _lib.ptr(big["kf_out"])
            assert _call(L, a, device) == inv, (out, other)
    if device:
        for stride in (0, 8, 11, 13, 14, 30, -12):
            a = dict(base)
            a["stride"] = stride
            assert _call(L, a, True) == inv, stride
    else:
        # rows out of range, which only the host form can see
        for key, rows in (("parent", base["n_kf"]), ("kf_gba_row", base["n_gba_kf"]), ("point_gba_row", base["n_gba_points"]),
                          ("ref", base["n_kf"])):
            for bad in (rows, -2):
                a = dict(base)
                a[key] = base[key].copy()
                a[key][-1] = bad
                assert _call(L, a) == inv, (key, bad)
                assert key.encode() in L.orbfe_last_error()
        assert _call(L, base) == ok     # and the scene itself is a valid call
    assert not base["kf_out"]["Tcw"].any() or _gpu(L)


def test_a_valid_call_without_a_device_is_an_error_not_a_fallback(L):
    if _gpu(L):
        pytest.skip("a GPU is present")
    s = M.scene("mixed")
    a = _args(s)
    assert _call(L, a) == _lib.ERR_NO_DEVICE and b"no CPU fallback" in L.orbfe_last_error()
    assert not a["kf_out"]["Tcw"].any() and not a["points_out"].any()
    assert _call(L, a, device=True) == _lib.ERR_NO_DEVICE
    # the limits themselves pass validation
    one = C.c_void_p(1 << 20)
    a = {k: (one if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    a["kf_out"], a["points_out"], a["result"] = C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    a["n_kf"] = a["n_gba_kf"] = _lib.GBA_MAP_MAX_KEYFRAMES
    a["n_points"] = a["n_gba_points"] = _lib.GBA_MAP_MAX_POINTS
    assert _call(L, a, device=True) == _lib.ERR_NO_DEVICE
    with pytest.raises(_lib.OrbfeError):
        optimizer.gba_update_map(s["poses"], s["parent"], s["kf_gba_row"], s["gba_poses"], s["half_baseline"], s["points"],
                                 s["point_gba_row"], s["ref"], s["gba_points"])
