"""CPU: (1) the cases of tests/np_ba.py are parity cases -- on the reading alone: the Schur solve, the full solve and the stability
runs (permuted summation order, 4 ulp of noise on every summand) take every accept / reject alike, reach the same reset decision and
agree within half the parity tolerance; (2) five robust iterations of the reading are round 1 of np_lba's; (3) csrc/lba_internal.h
under BundleAdjustment's schedule and csrc/initial_map_internal.h, compiled for the host (tests/cpp_ba/host_arith.cpp), against the
reading -- the adjustment by the parity criterion of tests/test_ba_gpu.py, the build and finish stages bit for bit; (4) every limit of
orbfe_bundle_adjustment* and orbfe_create_initial_map* is refused one step past its boundary, before any device is looked for, and
without a device a valid call is an error."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, initializer, optimizer
from refactored_orb_slam2_amd._lib import BA_RESULT_DTYPE, INITIAL_MAP_RESULT_DTYPE, LBA_EDGE_DTYPE
from tests import np_ba as B
from tests import np_lba as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_ba", "_build", "libba_host.so")
NOISE = 4.0 * 2.0 ** -52     # a few ulp of double on every summand


# ---- (1) the cases ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _runs(name):
    s = B.case_scene(name)
    return [B.reference(name), B.run_scene(s, solve="full")] + [B.run_scene(s, order_seed=seed, noise=NOISE) for seed in (1, 2, 3)]


@pytest.mark.parametrize("name", list(B.CASES))
def test_the_case_is_a_parity_case(name):
    s, runs = B.case_scene(name), _runs(name)
    a = runs[0]
    worst = max(B.worst_ratio(r["poses"], r["points"], a["poses"], a["points"]) for r in runs[1:])
    print(f"{name}: {len(s['poses'])} keyframes, {len(s['points'])} points, {len(s['edges'])} edges, iterations {a['iterations']} of "
          f"{s['n_iterations']}, trials {a['trials']}, rejected {a['accepts'].count(False)}, chi2 {a['chi2_first']:.6g} -> {a['chi2_final']:.6g}, "
          f"runs against run A {worst:.4f} of the tolerance")
    mono = s["edges"]["u_right"] < 0
    seen = np.zeros(len(s["points"]), bool)
    seen[s["edges"]["point"]] = True
    # what the name promises
    assert a["rounds"] == (0 if name in ("edges_0", "no_free") else 1)
    if a["rounds"]:
        assert 2 <= len(s["poses"]) <= 9 and (len(s["points"]) <= 300)
    if name in ("robust_1", "robust_5", "plain_10", "robust_20"):
        assert a["iterations"] == s["n_iterations"] and mono.any() and not mono.all()
    if name == "rejected_step":
        assert not all(a["accepts"]) and a["iterations"] == s["n_iterations"]
    if name == "at_optimum":       # terminates early: rho == 0 after the first trial
        assert a["iterations"] == 1 < s["n_iterations"] and a["accepts"] == [False] and a["chi2_first"] == 0.0
    if name == "plain_5_mono":
        assert mono.all()
    if name == "robust_10_stereo":
        assert not mono.any()
    if name == "nothing_fixed":
        assert not s["fixed"].any()
    else:
        assert s["fixed"][0] == 1 and int(s["fixed"].sum()) == 1
    if name == "lonely_point":
        assert not seen[-1] and a["points"][-1].tobytes() == s["points"][-1].tobytes()
    if name == "lonely_keyframe":
        assert len(s["poses"]) - 1 not in s["edges"]["kf"] and s["fixed"][-1] == 0
        assert Q.worst_ratio(a["poses"][-1], [], s["poses"][-1], []) <= 1.0     # through the quaternion and back
    if name.startswith("points_"):
        assert len(s["points"]) == int(name[7:]) and seen.all()
    if name == "nine_keyframes":
        assert len(s["poses"]) == 9
    if name == "two_keyframes":
        assert len(s["poses"]) == 2
    assert a["points"][~seen].tobytes() == s["points"][~seen].tobytes()
    # every run decides alike, and agrees with run A within half the parity tolerance
    for r in runs[1:]:
        assert r["accepts"] == a["accepts"] and r["rounds"] == a["rounds"] and r["iterations"] == a["iterations"]
    assert worst <= 0.5


@functools.lru_cache(maxsize=None)
def _map_runs(name):
    s = B.map_scene(name)
    return [B.map_reference(name), B.run_map_case(s, solve="full")] + [B.run_map_case(s, order_seed=seed, noise=NOISE) for seed in (1, 2, 3)]


@pytest.mark.parametrize("name", list(B.MAP_CASES))
def test_the_map_case_is_a_parity_case(name):
    s, runs = B.map_scene(name), _map_runs(name)
    a = runs[0]
    worst = max(B.worst_ratio(r["poses"], r["points"], a["poses"], a["points"]) for r in runs[1:])
    z = a["depths"][~np.isnan(a["depths"])]
    spread = float(np.abs(z - a["median_depth"]).min(initial=np.inf, where=z != a["median_depth"])) if len(z) else 0.0
    print(f"{name}: n1 {len(s['keys1'])}, n2 {len(s['keys2'])}, points {a['n_points']}, tracked {a['tracked']}, median depth "
          f"{float(a['median_depth']):.6g} (nearest other depth {spread:.3g} away), reason {a['reason']}, iterations {a['ba']['iterations']}, "
          f"trials {a['ba']['trials']}, runs against run A {worst:.4f} of the tolerance")
    if name.startswith("tri_"):
        n = int(name[4:])
        assert a["n_points"] == a["tracked"] == n and bool(a["reason"] & B.MAP_FEW_POINTS) == (n < 100)
    if name.startswith("n1_"):
        assert len(s["keys1"]) == int(name[3:]) and a["n_points"] >= 20
    if name == "typical":
        assert a["success"] and a["n_points"] >= 250
    if name == "even":
        assert a["n_points"] == 6 and float(a["median_depth"]) == 8.0           # sorted 2 4 8 16 32 64: element (6 - 1) / 2 = 2
    if name == "odd":
        assert a["n_points"] == 7 and float(a["median_depth"]) == 8.0           # sorted 1 2 4 8 16 32 64: element 3
    if name == "ties":
        assert float(a["median_depth"]) == 8.0 and int((a["depths"] == 8.0).sum()) == 5
    if name == "duplicate_keypoint":
        assert a["tracked"] == a["n_points"] - 1 and a["reason"] == B.MAP_FEW_POINTS
    if name in ("exact_negative", "negative_median"):
        assert a["reason"] == B.MAP_MEDIAN_NEGATIVE and not a["success"]
        # the margin on the sign: the median lies far below zero on the scale of what the runs differ by
        assert float(a["median_depth"]) < -1.0 if name == "negative_median" else float(a["median_depth"]) == -2.0
        assert a["points"].tobytes() == a["unscaled_points"].tobytes()          # a reset rescales nothing
    if name == "nan_depth":
        assert int(np.isnan(a["depths"]).sum()) == 1 and float(a["median_depth"]) == 8.0 and a["success"]   # sorted 2 4 8 16 NaN
        # every trial of the NaN system is rejected (rho is NaN) and none terminates the call: all 20 iterations, one trial each
        assert (a["ba"]["iterations"], a["ba"]["trials"]) == (20, 20) and not any(a["ba"]["accepts"])
    if name == "zero_points":
        assert a["n_points"] == 0 and a["reason"] == B.MAP_NO_POINTS | B.MAP_FEW_POINTS and a["ba"]["rounds"] == 0
    if name == "general_pose":
        assert a["success"] and not np.array_equal(s["pose1"], B.IDENTITY)
    if a["success"]:
        with np.errstate(all="ignore"):
            inv = np.float32(1.0) / a["median_depth"]
        assert np.array_equal(a["points"], a["unscaled_points"] * inv, equal_nan=True)
        assert a["poses"][0].tobytes() == a["unscaled_poses"][0].tobytes()
    for r in runs[1:]:
        assert r["reason"] == a["reason"] and r["tracked"] == a["tracked"] and np.array_equal(r["index"], a["index"])
        assert r["ba"]["accepts"] == a["ba"]["accepts"] and r["ba"]["iterations"] == a["ba"]["iterations"]
    assert worst <= 0.5


# ---- (2) against the local bundle adjustment's reading -------------------------------------------------------------------------------
@pytest.mark.parametrize("name, delta", [("all_stereo", None), ("standard", Q.DELTA_MONO), ("kf0_local", Q.DELTA_MONO)])
def test_five_robust_iterations_are_round_one_of_the_local_bundle_adjustment(name, delta):
    """bit for bit.  The monocular Huber delta of BundleAdjustment is (float)sqrt(5.99), LocalBundleAdjustment's (float)sqrt(5.991)
    (Optimizer.cc:82, :499): with the deltas as the source has them the two are equal on a scene without monocular edges, and on
    any scene once the reading is given the other delta"""
    s = Q.case_scene(name)
    lba = Q.optimize(s["poses"], s["fixed"], s["points"], s["edges"], s["cam"], flags=Q.FIRST_ROUND_ONLY)
    kw = {} if delta is None else dict(delta_mono=delta)
    ba = B.optimize(s["poses"], s["fixed"], s["points"], s["edges"], s["cam"], n_iterations=5, robust=True, **kw)
    assert ba["accepts"] == lba["accepts"][0] and ba["chi2_final"] == lba["chi2_final"][0]
    assert ba["poses"].tobytes() == np.asarray(lba["round1_poses"], np.float32).tobytes()
    assert ba["points"].tobytes() == np.asarray(lba["round1_points"], np.float32).tobytes()
    if delta is not None:          # and with its own delta it is another optimisation: the difference is real
        own = B.optimize(s["poses"], s["fixed"], s["points"], s["edges"], s["cam"], n_iterations=5, robust=True)
        assert own["chi2_first"] != lba["chi2_first"][0]


# ---- (3) the internal headers on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_ba"), "_build/libba_host.so"], check=True, capture_output=True)
    return C.CDLL(HOST_LIB)


def _camera(cam, sig=(1.0,)):
    return optimizer.pose_camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], list(sig))


def test_record_layouts(H):
    out = np.zeros(5, np.int32)
    H.ba_host_sizes(_lib.ptr(out))
    assert out.tolist() == [BA_RESULT_DTYPE.itemsize, BA_RESULT_DTYPE.fields["chi2_first"][1], INITIAL_MAP_RESULT_DTYPE.itemsize,
                            INITIAL_MAP_RESULT_DTYPE.fields["ba"][1], INITIAL_MAP_RESULT_DTYPE.fields["median_depth"][1]]
    assert (_lib.BA_MAX_ITERATIONS, _lib.BA_ROBUST) == (20, 1)


def _ba_host(H, s, n_iterations=None, robust=None):
    edges = np.ascontiguousarray(s["edges"], LBA_EDGE_DTYPE)
    poses, points, fixed = np.ascontiguousarray(s["poses"]), np.ascontiguousarray(s["points"]), np.ascontiguousarray(s["fixed"])
    po, xo, res = np.zeros_like(poses), np.zeros_like(points), np.zeros(1, BA_RESULT_DTYPE)
    n_it = s["n_iterations"] if n_iterations is None else n_iterations
    rb = s["robust"] if robust is None else robust
    rc = H.ba_host(_lib.ptr(_camera(s["cam"])), _lib.ptr(poses), _lib.ptr(fixed), len(poses), _lib.ptr(points), len(points), _lib.ptr(edges),
                   len(edges), int(n_it), _lib.BA_ROBUST if rb else 0, _lib.ptr(po), _lib.ptr(xo), _lib.ptr(res))
    return rc, po, xo, res[0]


@pytest.mark.parametrize("name", list(B.CASES))
def test_host_arithmetic_against_the_reading(H, name):
    s, ref = B.case_scene(name), B.reference(name)
    rc, poses, points, res = _ba_host(H, s)
    ratio = B.worst_ratio(poses, points, ref["poses"], ref["points"])
    not_equal = int((poses.view(np.uint32) != ref["poses"].view(np.uint32)).sum() + (points.view(np.uint32) != ref["points"].view(np.uint32)).sum())
    print(f"ba host arithmetic {name}: max diff / tolerance {ratio:.4f}, floats not bit-equal {not_equal}/{poses.size + points.size}, rounds "
          f"{int(res['rounds'])}/{ref['rounds']}, iterations {int(res['iterations'])}/{ref['iterations']}, trials {int(res['trials'])}/{ref['trials']}, "
          f"chi2 {float(res['chi2_first']):.6g} -> {float(res['chi2_final']):.6g} (reading {ref['chi2_first']:.6g} -> {ref['chi2_final']:.6g})")
    assert rc == 0
    assert (int(res["rounds"]), int(res["iterations"]), int(res["trials"])) == (ref["rounds"], ref["iterations"], ref["trials"])
    assert int(res["n_free"]) == int((s["fixed"] == 0).sum()) and int(res["n_edges"]) == len(s["edges"])
    seen = np.zeros(len(s["points"]), bool)
    seen[s["edges"]["point"]] = True
    assert points[~seen].tobytes() == s["points"][~seen].tobytes()
    assert ratio <= 1.0
    if ref["rounds"]:
        assert abs(float(res["chi2_final"]) - ref["chi2_final"]) <= 1e-9 * max(1.0, ref["chi2_final"])


def test_host_arithmetic_of_five_robust_iterations_is_round_one_of_the_local_bundle_adjustment(H):
    """byte for byte, poses and points, on an all-stereo scene whose one fixed keyframe is the identity (see
    test_five_robust_iterations_are_round_one_of_the_local_bundle_adjustment; BundleAdjustment writes the fixed keyframe back through
    the quaternion, which returns the identity exactly)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_lba"), "_build/liblba_host.so"], check=True, capture_output=True)
    HL = C.CDLL(os.path.join(ROOT, "tests", "cpp_lba", "_build", "liblba_host.so"))
    s = B.stereo_scene()
    assert s["fixed"].tolist() == [1, 0, 0, 0, 0] and s["poses"][0].tobytes() == B.IDENTITY.tobytes() and not (s["edges"]["u_right"] < 0).any()
    edges, poses, points, fixed = (np.ascontiguousarray(s[k]) for k in ("edges", "poses", "points", "fixed"))
    po, xo = np.zeros_like(poses), np.zeros_like(points)
    er, res = np.zeros(len(edges), np.uint8), np.zeros(1, _lib.LBA_RESULT_DTYPE)
    assert HL.lba_host(_lib.ptr(_camera(s["cam"])), _lib.ptr(poses), _lib.ptr(fixed), len(poses), _lib.ptr(points), len(points), _lib.ptr(edges),
                       len(edges), _lib.LBA_FIRST_ROUND_ONLY, _lib.ptr(po), _lib.ptr(xo), _lib.ptr(er), _lib.ptr(res)) == 0
    rc, poses_ba, points_ba, res_ba = _ba_host(H, s, 5, True)
    assert rc == 0 and poses_ba.tobytes() == po.tobytes() and points_ba.tobytes() == xo.tobytes()
    assert float(res_ba["chi2_final"]) == float(res[0]["chi2_final"][0]) and int(res_ba["trials"]) == int(res[0]["trials"][0])
    assert int(res[0]["n_erase"]) > 0                                      # outliers are there: the Huber branch was taken


def _words(tri):
    b = np.zeros(((len(tri) + 63) // 64) * 64, np.uint8)
    b[:len(tri)] = tri
    return np.ascontiguousarray(np.packbits(b.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64)) if len(tri) else np.zeros(1, np.uint64)


@pytest.mark.parametrize("name", list(B.MAP_CASES))
def test_host_arithmetic_of_the_build_and_finish_stages_is_the_reading_bit_for_bit(H, name):
    s, ref = B.map_scene(name), B.map_reference(name)
    n1, n2 = len(s["keys1"]), len(s["keys2"])
    cam = _camera(s["cam"], s["inv_level_sigma2"])
    index, points = np.zeros(n1, np.int32), np.zeros((n1, 3), np.float32)
    edges, poses = np.zeros(2 * n1, LBA_EDGE_DTYPE), np.zeros((2, 12), np.float32)
    pose1 = np.ascontiguousarray(s["pose1"]) if "pose1" in s else None
    m12, p3d = np.ascontiguousarray(s["matches12"], np.int32), np.ascontiguousarray(s["P3D"], np.float32)
    n = H.imap_build_host(_lib.ptr(cam), _lib.ptr(np.ascontiguousarray(s["keys1"])), n1, _lib.ptr(np.ascontiguousarray(s["keys2"])), n2,
                          _lib.ptr(m12), _lib.ptr(p3d), _lib.ptr(_words(s["triangulated"])), _lib.ptr(np.ascontiguousarray(s["R21"])),
                          _lib.ptr(np.ascontiguousarray(s["t21"])), _lib.ptr(s["octaves1"]), _lib.ptr(s["octaves2"]), _lib.ptr(pose1),
                          _lib.ptr(index), _lib.ptr(points), _lib.ptr(edges), _lib.ptr(poses))
    r_index, r_poses, _, r_points, r_edges = B.build_map(s["keys1"], s["keys2"], s["matches12"], s["P3D"], s["triangulated"], s["R21"], s["t21"],
                                                          s["octaves1"], s["octaves2"], s["inv_level_sigma2"], s.get("pose1"))
    assert n == len(r_index) == ref["n_points"] and np.array_equal(index[:n], r_index) and (index[n:] == -1).all()
    assert points[:n].tobytes() == r_points.tobytes() and edges[:2 * n].tobytes() == r_edges.tobytes() and poses.tobytes() == r_poses.tobytes()
    # the finish stage on the READING's adjustment
    kw = s["kw"]
    depths, out_poses, out_points = np.zeros(max(n, 1), np.float32), np.zeros((2, 12), np.float32), np.zeros((max(n, 1), 3), np.float32)
    res = np.zeros(1, INITIAL_MAP_RESULT_DTYPE)
    mop = np.ascontiguousarray(m12[r_index], np.int32) if n else np.zeros(1, np.int32)
    H.imap_finish_host(_lib.ptr(np.ascontiguousarray(ref["unscaled_poses"])), _lib.ptr(np.ascontiguousarray(ref["unscaled_points"]) if n else out_points),
                       _lib.ptr(mop), n, n2, int(kw.get("q", 2)), int(kw.get("min_points", 100)), int(ref["ba"]["rounds"]), _lib.ptr(depths),
                       _lib.ptr(out_poses), _lib.ptr(out_points), _lib.ptr(res))
    r = res[0]
    print(f"{name}: {n} points, tracked {int(r['tracked'])}, median depth {float(r['median_depth'])!r} (reading {float(ref['median_depth'])!r}), reason "
          f"{int(r['reason'])} (reading {ref['reason']})")
    assert depths[:n].tobytes() == ref["depths"].tobytes()
    assert (int(r["n_points"]), int(r["tracked"]), int(r["reason"]), int(r["success"])) == (n, ref["tracked"], ref["reason"], int(ref["success"]))
    assert np.float32(r["median_depth"]).tobytes() == np.float32(ref["median_depth"]).tobytes()
    assert out_poses.tobytes() == ref["poses"].tobytes() and out_points[:n].tobytes() == ref["points"].tobytes()


def test_the_depth_of_a_general_pose_is_this_projects_reading_of_mat_dot(H):
    """cv::Mat::dot in double in element order, + zcw in double, one rounding: a case in which summing in float, or in another order,
    gives another float"""
    T = np.zeros((2, 12), np.float32)
    T[0, 8:12] = [0.581118106842041, 0.3645724058151245, 0.2941325008869171, 0.028422242030501366]
    X = np.array([[5.467129707336426, -7.364541053771973, -1.6290994882583618]], np.float32)
    d = B.scene_depths(T[0], X)
    f32 = np.float32
    in_float = f32(f32(f32(T[0, 8] * X[0, 0]) + f32(T[0, 9] * X[0, 1])) + f32(T[0, 10] * X[0, 2])) + T[0, 11]
    assert d[0] != in_float
    out = np.zeros(1, np.float32)
    res = np.zeros(1, INITIAL_MAP_RESULT_DTYPE)
    H.imap_finish_host(_lib.ptr(T), _lib.ptr(X), _lib.ptr(np.zeros(1, np.int32)), 1, 1, 2, 0, 1, _lib.ptr(out), _lib.ptr(np.zeros((2, 12), np.float32)),
                       _lib.ptr(np.zeros((1, 3), np.float32)), _lib.ptr(res))
    assert out.tobytes() == d.tobytes() and np.float32(res[0]["median_depth"]).tobytes() == d.tobytes()


# ---- (4) the limits: refused before a device is looked for ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _accepted(L):
    n = C.c_int(0)
    gpu = L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    return _lib.OK if gpu else _lib.ERR_NO_DEVICE


def _call(L, n_kf, n_free, n_points, n_edges, n_iterations=5, flags=1, edit=None, null=None):
    """orbfe_bundle_adjustment on a well-formed problem of these counts (edges: point i % n_points, keyframe spread)"""
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
    return L.orbfe_bundle_adjustment(p["cam"], p["poses"], p["fixed"], n_kf, p["points"], n_points, p["edges"], n_edges, n_iterations, flags,
                                     p["poses_out"], p["points_out"], p["res"])


def test_limits_of_the_host_form(L):
    ok = _accepted(L)
    F, K, NP, NE, IT = _lib.LBA_MAX_FREE, _lib.LBA_MAX_KEYFRAMES, _lib.LBA_MAX_POINTS, _lib.LBA_MAX_EDGES, _lib.BA_MAX_ITERATIONS
    assert _call(L, F + 2, F, 40, 400) == ok                          # the largest number of free keyframes
    assert _call(L, F + 2, F + 1, 40, 400) == _lib.ERR_INVALID
    assert b"free keyframes" in L.orbfe_last_error() and b"bundle adjustment" in L.orbfe_last_error()
    assert _call(L, K, 4, 40, 400) == ok and _call(L, K + 1, 4, 40, 400) == _lib.ERR_INVALID
    assert _call(L, 8, 4, NP, 400) == ok and _call(L, 8, 4, NP + 1, 400) == _lib.ERR_INVALID
    assert _call(L, 8, 4, NP, NE) == ok and _call(L, 8, 4, NP, NE + 1) == _lib.ERR_INVALID
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


def test_limits_of_the_batch_form(L):
    ok = _accepted(L)
    K, NP, NE, PR, IT = _lib.LBA_MAX_KEYFRAMES, _lib.LBA_MAX_POINTS, _lib.LBA_MAX_EDGES, _lib.LBA_MAX_PROBLEMS, _lib.BA_MAX_ITERATIONS
    need = optimizer.lba_workspace_bytes(2, 8, 40, 160)
    buf = np.zeros(need + 512, np.uint8)
    base = (buf.ctypes.data + 255) & ~255                                  # host memory stands in: nothing is launched without a device

    def batch(P=2, caps=(8, 40, 160), stride=12, n_it=20, flags=1, ws=base, ws_bytes=need, null=None, off=None):
        a = [0x1000 + 0x100 * k for k in range(9)]                         # aligned stand-ins; refused calls never read them
        if null is not None:
            a[null] = None
        if off is not None:
            a[off] += 2
        return L.orbfe_bundle_adjustment_batch_device(P, a[0], a[1], a[2], a[3], a[4], stride, a[5], *caps, n_it, flags, a[6], a[7], a[8], ws,
                                                      ws_bytes, None)
    if ok == _lib.ERR_NO_DEVICE:
        assert batch() == ok                                               # valid arguments: refused only for want of a device
        assert b"no CPU fallback" in L.orbfe_last_error()
    assert batch(P=0) == ok
    assert batch(P=PR + 1) == _lib.ERR_INVALID and batch(P=-1) == _lib.ERR_INVALID
    assert batch(caps=(K + 1, 40, 160)) == _lib.ERR_INVALID and batch(caps=(8, NP + 1, 160)) == _lib.ERR_INVALID
    assert batch(caps=(8, 40, NE + 1)) == _lib.ERR_INVALID
    assert batch(stride=8) == _lib.ERR_INVALID and batch(stride=14) == _lib.ERR_INVALID
    assert batch(flags=2) == _lib.ERR_INVALID and batch(n_it=0) == _lib.ERR_INVALID and batch(n_it=IT + 1) == _lib.ERR_INVALID
    assert batch(ws_bytes=need - 1) == _lib.ERR_INVALID and batch(ws=base + 8) == _lib.ERR_INVALID and batch(ws=None) == _lib.ERR_INVALID
    for k in range(9):
        assert batch(null=k) == _lib.ERR_INVALID, k
    for k in (0, 1, 2, 4, 5, 6, 7, 8):
        assert batch(off=k) == _lib.ERR_INVALID, k


def _map_call(L, n1=40, n2=50, n_it=20, q=2, min_points=100, null=None, edit=None, levels=2):
    cam = optimizer.pose_camera(520.0, 520.0, 320.0, 240.0, 0.0, [1.0] * levels)
    a = dict(cam=cam, keys1=np.ones((max(n1, 1), 2), np.float32), keys2=np.ones((max(n2, 1), 2), np.float32),
             m12=(np.arange(max(n1, 1)) % max(min(n2, n1), 1)).astype(np.int32), p3d=np.ones((max(n1, 1), 3), np.float32),
             tri=np.full((max(n1, 1) + 63) // 64, np.uint64(0xFFFFFFFFFFFFFFFF)), init=np.zeros(1, _lib.INIT_RESULT_DTYPE),
             o1=np.zeros(max(n1, 1), np.int32), o2=np.zeros(max(n2, 1), np.int32), poses=np.zeros((2, 12), np.float32),
             points=np.zeros((max(n1, 1), 3), np.float32), index=np.zeros(max(n1, 1), np.int32), res=np.zeros(1, INITIAL_MAP_RESULT_DTYPE))
    if edit:
        edit(a)
    p = {k: (None if k == null else _lib.ptr(v)) for k, v in a.items()}
    return L.orbfe_create_initial_map(p["cam"], p["keys1"], n1, p["keys2"], n2, p["m12"], p["p3d"], p["tri"], p["init"], p["o1"], p["o2"], None,
                                      n_it, q, min_points, p["poses"], p["points"], p["index"], None, None, p["res"])


def test_limits_of_the_initial_map(L):
    ok = _accepted(L)
    M, IT, PR = _lib.INIT_MAX_MATCHES, _lib.BA_MAX_ITERATIONS, _lib.LBA_MAX_PROBLEMS
    assert _map_call(L) == ok
    assert _map_call(L, n1=M, n2=M) == ok
    assert _map_call(L, n1=M + 1, n2=M) == _lib.ERR_INVALID and _map_call(L, n1=M, n2=M + 1) == _lib.ERR_INVALID
    assert _map_call(L, n1=-1) == _lib.ERR_INVALID and _map_call(L, n2=-1) == _lib.ERR_INVALID
    assert _map_call(L, n_it=0) == _lib.ERR_INVALID and _map_call(L, n_it=IT) == ok and _map_call(L, n_it=IT + 1) == _lib.ERR_INVALID
    assert _map_call(L, q=0) == _lib.ERR_INVALID and _map_call(L, q=1) == ok and _map_call(L, min_points=-1) == _lib.ERR_INVALID
    assert _map_call(L, min_points=0) == ok
    assert _map_call(L, edit=lambda a: a["m12"].__setitem__(3, 50)) == _lib.ERR_INVALID       # a match outside frame 2
    assert _map_call(L, edit=lambda a: a["m12"].__setitem__(3, -1)) == ok
    assert _map_call(L, edit=lambda a: a["o1"].__setitem__(5, 2)) == _lib.ERR_INVALID         # an octave the camera has no level for
    assert _map_call(L, edit=lambda a: a["o1"].__setitem__(5, 1)) == ok
    assert _map_call(L, edit=lambda a: a["o2"].__setitem__(5, -1)) == _lib.ERR_INVALID
    for null in ("cam", "keys1", "keys2", "m12", "p3d", "tri", "init", "o1", "o2", "poses", "points", "index", "res"):
        assert _map_call(L, null=null) == _lib.ERR_INVALID, null
    n = C.c_size_t(0)
    assert L.orbfe_initial_map_workspace_bytes(PR, M, C.byref(n)) == _lib.OK and n.value > 0
    for bad in ((PR + 1, M), (1, M + 1), (-1, 8), (1, 0)):
        assert L.orbfe_initial_map_workspace_bytes(*bad, C.byref(n)) == _lib.ERR_INVALID, bad
    assert L.orbfe_initial_map_workspace_bytes(1, 8, None) == _lib.ERR_INVALID
    assert initializer.initial_map_workspace_bytes(3, 300) >= 3 * optimizer.lba_workspace_bytes(1, 2, 300, 600)
    need = initializer.initial_map_workspace_bytes(2, 64)
    buf = np.zeros(need + 512, np.uint8)
    base = (buf.ctypes.data + 255) & ~255

    def batch(P=2, cap=64, n_it=20, q=2, min_points=100, ws=base, ws_bytes=need, null=None, off=None, opt=(None, None, None)):
        a = [0x1000 + 0x100 * k for k in range(15)]
        if null is not None:
            a[null] = None
        if off is not None:
            a[off] += 2
        return L.orbfe_create_initial_map_batch_device(P, a[0], a[1], a[2], a[3], a[4], cap, a[5], a[6], a[7], a[8], a[9], a[10], opt[0], n_it, q,
                                                       min_points, a[11], a[12], a[13], opt[1], opt[2], a[14], ws, ws_bytes, None)
    if ok == _lib.ERR_NO_DEVICE:
        assert batch() == ok and batch(opt=(0x4000, 0x4100, 0x4200)) == ok
    assert batch(P=0) == ok
    assert batch(P=PR + 1) == _lib.ERR_INVALID and batch(cap=0) == _lib.ERR_INVALID and batch(cap=M + 1) == _lib.ERR_INVALID
    assert batch(n_it=0) == _lib.ERR_INVALID and batch(n_it=IT + 1) == _lib.ERR_INVALID and batch(q=0) == _lib.ERR_INVALID
    assert batch(ws_bytes=need - 1) == _lib.ERR_INVALID and batch(ws=base + 8) == _lib.ERR_INVALID and batch(ws=None) == _lib.ERR_INVALID
    for k in range(15):
        assert batch(null=k) == _lib.ERR_INVALID, k
        assert batch(off=k) == _lib.ERR_INVALID, k
    assert batch(opt=(0x4002, None, None)) == _lib.ERR_INVALID


def test_no_device_is_an_error_not_a_fallback(L):
    if _accepted(L) == _lib.OK:
        pytest.skip("a GPU is present")
    s = B.case_scene("robust_1")
    with pytest.raises(_lib.OrbfeError) as ei:
        optimizer.bundle_adjustment(_camera(s["cam"]), s["poses"], s["fixed"], s["points"], s["edges"], 1, True)
    assert ei.value.code == _lib.ERR_NO_DEVICE and b"no CPU fallback" in L.orbfe_last_error()
    m = B.map_scene("even")
    init = np.zeros(1, _lib.INIT_RESULT_DTYPE)
    with pytest.raises(_lib.OrbfeError) as ei:
        initializer.create_initial_map(_camera(m["cam"], m["inv_level_sigma2"]), m["keys1"], m["keys2"], m["matches12"], m["P3D"], m["triangulated"],
                                       init, m["octaves1"], m["octaves2"])
    assert ei.value.code == _lib.ERR_NO_DEVICE
