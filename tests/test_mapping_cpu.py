"""CPU suite of CreateNewMapPoints: the numpy reading of tests/np_mapping.py against a noise-free scene, the conditions that make
the GPU comparison meaningful (margin, R32 == R64 on parity pairs, coverage) ASSERTED on the whole case list, the arithmetic of
csrc/mapping_internal.h compiled for the host against the reading, and the C ABI without a device: struct sizes, exports, every
validation boundary on both sides, ORBFE_ERR_NO_DEVICE from all three entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, mapping
from tests import np_mapping as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_mapping", "_build", "libmapping_host.so")
NON_PARITY_CAP = M.NON_PARITY_CAP


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in M.CASES:
        s = M.case_scene(name)
        out[name] = (s, M.run(s, "R64"), M.run(s, "R32"))
    return out


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_struct_sizes_and_exports(L):
    assert _lib.TRI_VIEW_DTYPE.itemsize == 224 and _lib.NEW_POINT_DTYPE.itemsize == 44 and _lib.TRI_NEIGHBOR_DTYPE.itemsize == 464
    assert M.VIEW_DTYPE == _lib.TRI_VIEW_DTYPE and M.POINT_DTYPE == _lib.NEW_POINT_DTYPE and M.EPIPOLAR_DTYPE == _lib.EPIPOLAR_DTYPE
    assert _lib.TRI_NEIGHBOR_DTYPE.fields["view"][1] == 64 and _lib.TRI_NEIGHBOR_DTYPE.fields["ep"][1] == 288
    for sym in ("orbfe_triangulate_matches", "orbfe_triangulate_matches_batch_device", "orbfe_create_new_map_points"):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for text in ("} orbfe_tri_view;", "/* 224 bytes */", "} orbfe_new_point;", "/* 44 bytes */", "/* 464 bytes (LP64) */"):
        assert text in hdr
    assert (M.OK, M.NO_MATCH, M.W_ZERO, M.LOW_PARALLAX, M.BEHIND1, M.BEHIND2, M.REPROJ1, M.REPROJ2, M.DIST_ZERO, M.SCALE) == (
        _lib.TRI_OK, _lib.TRI_NO_MATCH, _lib.TRI_W_ZERO, _lib.TRI_LOW_PARALLAX, _lib.TRI_BEHIND1, _lib.TRI_BEHIND2, _lib.TRI_REPROJ1,
        _lib.TRI_REPROJ2, _lib.TRI_DIST_ZERO, _lib.TRI_SCALE)


# ---- the reading -------------------------------------------------------------------------------------------------------------------
def test_noise_free_scene_returns_the_true_points():
    """Without noise the only errors are the roundings to float of what the ABI carries: four pixel coordinates (half an ulp of
    1 241 = 6.1e-5 px each, 1.2e-7 rad of ray direction at fx = 719), nine rotation entries per pose (6e-8 each, 1.8e-7 rad) and the
    translations (1.2e-7 m).  That is 3e-7 rad per ray, 6e-7 rad on the angle between the two, and a point triangulated from rays
    that meet at the angle theta moves by dist x 6e-7 / theta; an unprojected point inherits the relative rounding of its depth
    and pixel (1e-6 x dist covers both).  The bound asserted is 1e-6 x dist x (1 + 1 / theta) + 1e-6 m."""
    for stereo in (0.0, 0.6):
        s = M.make_scene(31, base=2.9, stereo=stereo, noise=False, outliers=0.0)
        r = M.run(s, "R64")
        ok = r["code"] == M.OK
        assert ok.sum() > 500 and set(np.unique(r["code"])) <= {M.OK, M.NO_MATCH, M.LOW_PARALLAX, M.SCALE, M.REPROJ1, M.REPROJ2}
        truth = s["Pw"][ok]
        Ow1, Ow2 = s["view1"]["Ow"][0].astype(np.float64), s["view2"]["Ow"][0].astype(np.float64)
        d1, d2 = truth - Ow1, truth - Ow2
        dist = np.linalg.norm(d1, axis=1)
        theta = np.arccos(np.clip((d1 * d2).sum(1) / dist / np.linalg.norm(d2, axis=1), -1, 1))
        err = np.linalg.norm(r["pos"][ok] - truth, axis=1)
        lin = r["path"][ok] == M.PATH_LINEAR
        bound = 1e-6 * dist * (1 + np.where(lin, 1 / theta, 0.0)) + 1e-6
        print(f"noise-free stereo={stereo}: {ok.sum()} points ({lin.sum()} linear), worst error / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()
        # the normal is the mean of the two unit viewing rays, the distances follow the octave of pKF1
        want = (d1 / dist[:, None] + d2 / np.linalg.norm(d2, axis=1)[:, None]) / 2
        assert np.abs(r["normal"][ok] - want).max() <= 1e-6 / theta.min() + 1e-6
        sf = s["view1"]["scale_factors"][0].astype(np.float64)
        assert np.allclose(r["max_distance"][ok], dist * sf[s["keys1"]["octave"][ok]], rtol=1e-5 / theta.min())
        assert np.allclose(r["min_distance"][ok] * sf[7], r["max_distance"][ok], rtol=1e-12)


def test_case_list_margins_stability_and_coverage(runs):
    """What makes the GPU comparison meaningful, on the yardstick alone: few pairs are too close to a threshold to be compared, the
    float reading takes the decisions of the double one on all the others, and every reachable code and path is exercised."""
    codes, paths = np.zeros(10, np.int64), np.zeros(4, np.int64)
    for name, (s, r64, r32) in runs.items():
        par = r64["parity"]
        loose = (~par).sum() / len(par)
        lin = par & (r64["code"] == M.OK) & (r64["path"] == M.PATH_LINEAR)
        e = M.rel_error(r32["pos"][lin], r64["pos"][lin]) if lin.any() else np.zeros(1)
        print(f"{name}: non-parity {100 * loose:.2f} %, codes {np.bincount(r64['code'][par], minlength=10)}, "
              f"paths {np.bincount(r64['path'][par], minlength=4)}, R32 vs R64 on {lin.sum()} linear points: median {np.median(e):.3g} "
              f"max {e.max():.3g}")
        assert loose <= NON_PARITY_CAP
        assert np.array_equal(r32["code"][par], r64["code"][par]) and np.array_equal(r32["path"][par], r64["path"][par])
        assert np.array_equal(r32["idx2"], r64["idx2"])
        codes += np.bincount(r64["code"][par], minlength=10)
        paths += np.bincount(r64["path"][par], minlength=4)
    assert all(codes[c] >= 5 for c in M.REACHABLE), codes
    assert all(paths[p] >= 5 for p in range(4)), paths
    assert codes[M.W_ZERO] == 0 and codes[M.DIST_ZERO] == 0           # need exact zeros: untested


def test_baseline_gate_reading():
    v1 = M.make_view(np.eye(3), np.zeros(3))
    near, far = M.make_view(np.eye(3), [-0.5, 0, 0]), M.make_view(np.eye(3), [-0.6, 0, 0])
    assert M.baseline_too_short(v1, near, False, 0.0) and not M.baseline_too_short(v1, far, False, 0.0)       # mb = 0.537
    assert M.baseline_too_short(v1, far, True, 61.0) and not M.baseline_too_short(v1, far, True, 59.0)      # 0.6 / 60 = 0.01


# ---- csrc/mapping_internal.h on the host -------------------------------------------------------------------------------------------
def _host_lib():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_mapping")], check=True, capture_output=True)
    H = C.CDLL(HOST_LIB)
    vp, ci = C.c_void_p, C.c_int
    H.mapping_host_triangulate.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp]
    H.mapping_host_triangulate.restype = None
    return H


@pytest.mark.parametrize("name", list(M.CASES))
def test_host_arithmetic_against_the_reading(runs, name):
    """csrc/mapping_internal.h is host- and device-callable; compiled for the host with the library's flags it must already meet
    the criteria the kernel is held to on the GPU."""
    H = _host_lib()
    s, r64, r32 = runs[name]
    v1, k1, ur1, z1, v2, k2, ur2, z2, mA = M.scene_args(s)
    got = np.zeros(len(k1), _lib.NEW_POINT_DTYPE)
    H.mapping_host_triangulate(_lib.ptr(v1), _lib.ptr(k1), _lib.ptr(ur1), _lib.ptr(z1), len(k1), _lib.ptr(v2), _lib.ptr(k2), _lib.ptr(ur2),
                               _lib.ptr(z2), len(k2), _lib.ptr(mA), _lib.ptr(got))
    M.check_against_yardstick(name, s, r64, r32, got)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
def _tri(L, nA=4, nB=4, lv1=8, lv2=8, view1=True, view2=True, n_new=True, keys1=True, keys2=True, match=True, out=True, ur1=False,
         z1=False, ur2=False, z2=False):
    v1, v2 = M.make_view(np.eye(3), np.zeros(3), lv1), M.make_view(np.eye(3), [0, 0, -1.0], lv2)
    a, b = max(nA, 1), max(nB, 1)
    k1, k2 = np.zeros(a, _lib.KP_DTYPE), np.zeros(b, _lib.KP_DTYPE)
    mA, pts = np.full(a, -1, np.int32), np.zeros(a, _lib.NEW_POINT_DTYPE)
    fa, fb = np.full(a, -1, np.float32), np.full(b, -1, np.float32)
    nn = C.c_int(-7)
    p = lambda flag, arr: _lib.ptr(arr) if flag else None
    return L.orbfe_triangulate_matches(p(view1, v1), p(keys1, k1), p(ur1, fa), p(z1, fa), nA, p(view2, v2), p(keys2, k2), p(ur2, fb),
                                       p(z2, fb), nB, p(match, mA), p(out, pts), C.byref(nn) if n_new else None)


def test_triangulate_matches_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    assert _tri(L) == good
    assert _tri(L, nA=-1) == _lib.ERR_INVALID and _tri(L, nA=0) == good
    assert _tri(L, nB=-1) == _lib.ERR_INVALID and _tri(L, nB=0) == good
    assert _tri(L, nA=_lib.TRI_MAX_ROWS) == good and _tri(L, nA=_lib.TRI_MAX_ROWS + 1) == _lib.ERR_INVALID
    assert _tri(L, nB=_lib.TRI_MAX_ROWS) == good and _tri(L, nB=_lib.TRI_MAX_ROWS + 1) == _lib.ERR_INVALID
    for lv, want in ((0, _lib.ERR_INVALID), (1, good), (_lib.MAX_LEVELS, good), (_lib.MAX_LEVELS + 1, _lib.ERR_INVALID)):
        assert _tri(L, lv1=lv) == want and _tri(L, lv2=lv) == want
    for null in ("view1", "view2", "n_new", "keys1", "keys2", "match", "out"):
        assert _tri(L, **{null: False}) == _lib.ERR_INVALID, null
    assert _tri(L, nA=0, keys1=False, match=False, out=False) == good and _tri(L, nB=0, keys2=False) == good
    assert _tri(L, ur1=True) == _lib.ERR_INVALID and _tri(L, ur2=True) == _lib.ERR_INVALID      # u_right without depth
    assert _tri(L, ur1=True, z1=True, ur2=True, z2=True) == good


def _batch(L, K=0, capA=8, capB=8, null=None, misalign=None, ur_without_depth=False):
    """Nothing is launched for K == 0, so the pointers only have to look like device pointers."""
    names = ["view1", "keys1", "ur1", "z1", "nA", "view2", "keys2", "ur2", "z2", "nB", "matchA", "out", "n_new"]
    ptrs = {n: 0x10000 + 0x1000 * i for i, n in enumerate(names)}
    for n in ("ur1", "z1", "ur2", "z2"):
        ptrs[n] = 0
    if ur_without_depth:
        ptrs["ur2"] = 0x90000
    if null:
        ptrs[null] = 0
    if misalign:
        ptrs[misalign] += 2
    a = [C.c_void_p(ptrs[n] or None) for n in names]
    return L.orbfe_triangulate_matches_batch_device(K, a[0], a[1], a[2], a[3], a[4], capA, a[5], a[6], a[7], a[8], a[9], capB, a[10], a[11],
                                                    a[12], None)


def test_triangulate_batch_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    assert _batch(L) == good
    assert _batch(L, K=-1) == _lib.ERR_INVALID and _batch(L, K=_lib.TRI_MAX_ROWS + 1) == _lib.ERR_INVALID
    for cap in ("capA", "capB"):
        assert _batch(L, **{cap: 0}) == _lib.ERR_INVALID and _batch(L, **{cap: 1}) == good
        assert _batch(L, **{cap: _lib.TRI_MAX_ROWS}) == good and _batch(L, **{cap: _lib.TRI_MAX_ROWS + 1}) == _lib.ERR_INVALID
    for n in ("view1", "keys1", "nA", "view2", "keys2", "nB", "matchA", "out", "n_new"):
        assert _batch(L, null=n) == _lib.ERR_INVALID, n
        assert _batch(L, misalign=n) == _lib.ERR_INVALID, n
    assert _batch(L, ur_without_depth=True) == _lib.ERR_INVALID


def _chain(L, nA=4, K=1, nb_n=4, lvA=8, lv_nb=8, n_nodesA=0, nb_nodes=0, null=None, nb_null=None, ur_without_depth=False):
    a = max(nA, 1)
    kA, dA, has = np.zeros(a, _lib.KP_DTYPE), np.zeros((a, 32), np.uint8), np.zeros(a, np.uint8)
    vA = M.make_view(np.eye(3), np.zeros(3), lvA)
    b = max(nb_n, 1)
    kB, dB, hB = np.zeros(b, _lib.KP_DTYPE), np.zeros((b, 32), np.uint8), np.zeros(b, np.uint8)
    fB = np.full(b, -1, np.float32)
    rec = np.zeros(max(K, 1), _lib.TRI_NEIGHBOR_DTYPE)
    for r in rec:
        r["keys"], r["desc"], r["has_mp"] = kB.ctypes.data, dB.ctypes.data, hB.ctypes.data
        r["n"], r["n_nodes"] = nb_n, nb_nodes
        r["view"] = M.make_view(np.eye(3), [0, 0, -1.0], lv_nb)[0]
        if ur_without_depth:
            r["u_right"] = fB.ctypes.data
        if nb_null:
            r[nb_null] = 0
    pts = np.zeros((max(K, 1), a), _lib.NEW_POINT_DTYPE)
    nm, nn = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32)
    args = dict(keysA=kA, descA=dA, has=has, viewA=vA, rec=rec, pts=pts, nm=nm, nn=nn)
    if null:
        args[null] = None
    g = lambda k: _lib.ptr(args[k])
    return L.orbfe_create_new_map_points(g("keysA"), g("descA"), None, None, g("has"), nA, None, n_nodesA, None, g("viewA"), g("rec"), K, 0, 0,
                                         1, g("pts"), g("nm"), g("nn"))


def test_create_new_map_points_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    assert _chain(L) == good
    assert _chain(L, K=-1) == _lib.ERR_INVALID and _chain(L, K=0) == good
    assert _chain(L, nA=-1) == _lib.ERR_INVALID and _chain(L, nA=0) == good
    assert _chain(L, nA=_lib.TRI_MAX_ROWS, K=0) == good and _chain(L, nA=_lib.TRI_MAX_ROWS + 1, K=0) == _lib.ERR_INVALID
    assert _chain(L, nb_n=-1) == _lib.ERR_INVALID and _chain(L, nb_n=0) == good
    assert _chain(L, nb_n=_lib.TRI_MAX_ROWS) == good and _chain(L, nb_n=_lib.TRI_MAX_ROWS + 1) == _lib.ERR_INVALID
    for lv, want in ((0, _lib.ERR_INVALID), (1, good), (_lib.MAX_LEVELS, good), (_lib.MAX_LEVELS + 1, _lib.ERR_INVALID)):
        assert _chain(L, lvA=lv) == want and _chain(L, lv_nb=lv) == want
    assert _chain(L, n_nodesA=-1) == _lib.ERR_INVALID and _chain(L, nb_nodes=-1) == _lib.ERR_INVALID
    assert _chain(L, n_nodesA=1) == _lib.ERR_INVALID and _chain(L, nb_nodes=1) == _lib.ERR_INVALID      # node counts without arrays
    for null in ("keysA", "descA", "has", "viewA", "rec", "pts", "nm", "nn"):
        assert _chain(L, null=null) == _lib.ERR_INVALID, null
    for null in ("keys", "desc", "has_mp"):
        assert _chain(L, nb_null=null) == _lib.ERR_INVALID, null
    assert _chain(L, ur_without_depth=True) == _lib.ERR_INVALID


def test_no_device_is_an_error_not_a_fallback(L):
    """Through the Python mirror: without a device both host forms raise ORBFE_ERR_NO_DEVICE (with one they simply run)."""
    s = M.case_scene("mixed", n=16)
    c = M.make_chain_scene(n=40)
    A = c["A"]
    chain = (A["keys"], A["desc"], A["u_right"], A["depth"], A["has_mp"], A["groups"], A["view"], c["neighbors"])
    if _gpu_present(L):
        assert len(mapping.triangulate_matches(*M.scene_args(s))[0]) == 16
        assert mapping.create_new_map_points(*chain)[0].shape == (3, 40)
        return
    with pytest.raises(_lib.OrbfeError) as e:
        mapping.triangulate_matches(*M.scene_args(s))
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(_lib.OrbfeError) as e:
        mapping.create_new_map_points(*chain)
    assert e.value.code == _lib.ERR_NO_DEVICE
