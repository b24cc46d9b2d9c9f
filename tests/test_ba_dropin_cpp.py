"""csrc/host/Optimizer_hip.h -- orbfe_host::BundleAdjustment / GlobalBundleAdjustemnt, the functions with the signatures of
ORB_SLAM2::Optimizer's, and AdjustAndScaleInitialMap (Tracking.cc:618-642) -- on the mock KeyFrame / MapPoint / Map of tests/cpp_ba.
Without a GPU: which vertices and edges the adapter collects, what it marshals, what it writes for nLoopKF == 0 and for nLoopKF != 0,
and that a stop flag set on entry, or no device, leaves the map alone.  With a GPU: the map afterwards against the numpy reading of
tests/np_ba.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from refactored_orb_slam2_amd._lib import INITIAL_MAP_RESULT_DTYPE, LBA_EDGE_DTYPE, POSE_CAMERA_DTYPE
from tests import np_ba as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_ba", "_build", "test_ba_dropin")
N_LEVELS = 8
SIG = np.array([1.0 / (1.2 ** l) ** 2 for l in range(N_LEVELS)], np.float32)


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_ba")], check=True, capture_output=True)


def _pack(cam, sig, kfs, mps, in_map, n_iterations, robust, n_loop, stop, deltas=None):
    """kfs: (mnId, bad, pose[12], [(x, y, octave, u_right)]); mps: (mnId, bad, X[3], [(keyframe index, keypoint)])"""
    out = [struct.pack("<5f", cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"]), struct.pack("<i", len(sig)), np.asarray(sig, np.float32).tobytes()]
    out.append(struct.pack("<i", len(kfs)))
    for mnid, bad, pose, kps in kfs:
        out.append(struct.pack("<ii", mnid, bad) + np.asarray(pose, np.float32).tobytes() + struct.pack("<i", len(kps)))
        out += [struct.pack("<ffif", x, y, o, ur) for x, y, o, ur in kps]
    out.append(struct.pack("<i", len(mps)))
    for mnid, bad, X, obs in mps:
        out.append(struct.pack("<ii", mnid, bad) + np.asarray(X, np.float32).tobytes() + struct.pack("<i", len(obs)))
        out += [struct.pack("<ii", k, i) for k, i in obs]
    out.append(np.asarray(in_map, np.int32).tobytes())
    out.append(struct.pack("<4i", n_iterations, int(robust), n_loop, stop))
    if deltas:
        out.append(struct.pack("<2f", *deltas))
    return b"".join(out)


def _scene(name, n_loop=0, stop=0, deltas=None):
    """A case of np_ba as a map.  Keyframe 0 of the case has mnId 0 where the case fixes it, the others 10 + k; the keypoints of a
    keyframe are its observations in a shuffled order plus three without a point.  Added: a bad keyframe of the map that observes
    some points (no vertex, no edges), a keyframe with the largest mnId that is NOT among the map's keyframes and observes a point
    (above maxKFid: skipped), a bad map point, and a point that only the bad keyframe observes (no edge: left out, left alone)."""
    s = B.case_scene(name)
    rng = np.random.default_rng(78)
    n_kf, n_pt = len(s["poses"]), len(s["points"])
    ids = [0 if (k == 0 and s["fixed"][0]) else 10 + k for k in range(n_kf)] + [50, 99]
    bad_kf, far_kf = n_kf, n_kf + 1
    kps = [[] for _ in range(n_kf + 2)]
    for e in s["edges"]:
        kps[e["kf"]].append((float(e["u"]), float(e["v"]), int(np.argmin(np.abs(SIG - e["inv_sigma2"]))), float(e["u_right"]), int(e["point"])))
    for p in range(0, n_pt, 7):
        kps[bad_kf].append((100.0 + p, 50.0, 0, -1.0, p))
    kps[bad_kf].append((11.0, 12.0, 0, -1.0, n_pt + 1))                          # the point nobody else sees
    kps[far_kf].append((300.0, 80.0, 1, 250.0, 0))
    kps[n_kf - 1].append((10.0, 10.0, 0, -1.0, n_pt))                            # the bad map point
    obs = [[] for _ in range(n_pt + 2)]
    for k in range(n_kf + 2):
        kps[k] += [(5.0, 6.0, 0, -1.0, -1)] * 3
        kps[k] = [kps[k][i] for i in rng.permutation(len(kps[k]))]
        for i, kp in enumerate(kps[k]):
            if kp[4] >= 0:
                obs[kp[4]].append((k, i))
    poses = list(s["poses"]) + [s["poses"][-1], s["poses"][-1]]
    kfs = [(ids[k], int(k == bad_kf), poses[k], [kp[:4] for kp in kps[k]]) for k in range(n_kf + 2)]
    pts = list(s["points"]) + [np.array([1, 2, 3], np.float32), np.array([4, 5, 6], np.float32)]
    mps = [(100 + p, int(p == n_pt), pts[p], obs[p]) for p in range(n_pt + 2)]
    in_map = [1] * (n_kf + 1) + [0]
    raw = _pack(s["cam"], SIG, kfs, mps, in_map, s["n_iterations"], s["robust"], n_loop, stop, deltas)
    return s, raw, dict(ids=ids, n_kf=n_kf, n_pt=n_pt, bad_kf=bad_kf, far_kf=far_kf, poses=np.array(poses, np.float32), points=np.array(pts, np.float32))


def _exe(tmp_path, raw, mode):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(raw)
    r = subprocess.run([EXE, str(fin), str(fout), mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return fout.read_bytes(), r.stderr


KF_OUT = np.dtype([("set_pose", "<i4"), ("pose", "<f4", (12,)), ("gba_for", "<i4"), ("gba_rows", "<i4"), ("gba", "<f4", (12,))])
MP_OUT = np.dtype([("set_pos", "<i4"), ("update", "<i4"), ("pos", "<f4", (3,)), ("gba_for", "<i4"), ("gba_rows", "<i4"), ("gba", "<f4", (3,))])


def _read_map(out, n_kfs, n_mps):
    ret = struct.unpack_from("<i", out, 0)[0]
    kf = np.frombuffer(out, KF_OUT, n_kfs, 4)
    mp = np.frombuffer(out, MP_OUT, n_mps, 4 + n_kfs * KF_OUT.itemsize)
    return ret, kf, mp, out[4 + n_kfs * KF_OUT.itemsize + n_mps * MP_OUT.itemsize:]


def _gpu():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.mark.parametrize("name", ["robust_5", "nothing_fixed"])
def test_what_the_adapter_collects_and_marshals(tmp_path, name):
    _build()
    s, raw, info = _scene(name)
    out, _ = _exe(tmp_path, raw, "marshal")
    off = 0
    n_kf = struct.unpack_from("<i", out, off)[0]; off += 4
    ids = np.frombuffer(out, "<i4", n_kf, off); off += 4 * n_kf
    fixed = np.frombuffer(out, np.uint8, n_kf, off); off += n_kf
    poses = np.frombuffer(out, "<f4", 12 * n_kf, off).reshape(n_kf, 12); off += 48 * n_kf
    max_id, n_pt = struct.unpack_from("<ii", out, off); off += 8
    mp_ids = np.frombuffer(out, "<i4", n_pt, off); off += 4 * n_pt
    included = np.frombuffer(out, np.uint8, n_pt, off); off += n_pt
    points = np.frombuffer(out, "<f4", 3 * n_pt, off).reshape(n_pt, 3); off += 12 * n_pt
    n_e = struct.unpack_from("<i", out, off)[0]; off += 4
    edges = np.frombuffer(out, LBA_EDGE_DTYPE, n_e, off); off += 24 * n_e
    cam = np.frombuffer(out, POSE_CAMERA_DTYPE, 1, off)[0]
    # the vertices: the map's keyframes that are not bad, in its order (the bad one and the one outside the map are no vertex); the
    # points that are not bad; the one without an edge is not included
    assert ids.tolist() == info["ids"][:info["n_kf"]] and max_id == max(info["ids"][:info["n_kf"]])
    assert fixed.tolist() == [int(i == 0) for i in ids] == s["fixed"].tolist()
    assert poses.tobytes() == s["poses"].tobytes()
    assert mp_ids.tolist() == [100 + p for p in range(info["n_pt"])] + [100 + info["n_pt"] + 1]
    assert included.tolist() == [1] * info["n_pt"] + [0] and points[:info["n_pt"]].tobytes() == s["points"].tobytes()
    # the edges: the case's, point by point (inside a point in the order of its std::map, i.e. of the keyframes' addresses)
    assert n_e == len(s["edges"]) and (np.diff(edges["point"]) >= 0).all()
    order = np.lexsort((edges["kf"], edges["point"]))
    assert edges[order].tobytes() == s["edges"].tobytes()
    assert (float(cam["fx"]), float(cam["mbf"])) == (np.float32(s["cam"]["fx"]), np.float32(s["cam"]["mbf"]))


@pytest.mark.parametrize("n_loop", [0, 7])
def test_what_the_adapter_writes(tmp_path, n_loop):
    _build()
    s, raw, info = _scene("robust_5", n_loop=n_loop, deltas=(0.5, 0.25))
    out, _ = _exe(tmp_path, raw, "apply")
    _, kf, mp, _ = _read_map(out, info["n_kf"] + 2, info["n_pt"] + 2)
    good = np.arange(info["n_kf"])
    pts = np.arange(info["n_pt"])
    for rows, n_good, before, delta, width in ((kf, good, info["poses"], 0.5, 12), (mp, pts, info["points"], 0.25, 3)):
        cur = rows["pose"] if width == 12 else rows["pos"]
        calls = rows["set_pose"] if width == 12 else rows["set_pos"]
        rest = np.setdiff1d(np.arange(len(rows)), n_good)
        # the bad keyframe, the keyframe outside the map, the bad point and the point without an edge: nothing at all
        assert not calls[rest].any() and cur[rest].tobytes() == before[rest].tobytes() and not rows["gba_for"][rest].any() and not rows["gba_rows"][rest].any()
        if n_loop == 0:        # into the map: SetPose of EVERY keyframe of the graph, the fixed one too; SetWorldPos + UpdateNormalAndDepth
            assert (calls[n_good] == 1).all() and np.array_equal(cur[n_good], before[n_good] + np.float32(delta))
            assert not rows["gba_for"].any() and not rows["gba_rows"].any()
        else:                  # beside the map: mTcwGBA / mPosGBA / mnBAGlobalForKF
            assert not calls.any() and cur.tobytes() == before.tobytes()
            assert (rows["gba_for"][n_good] == n_loop).all() and (rows["gba_rows"][n_good] == (4 if width == 12 else 3)).all()
            assert np.array_equal(rows["gba"][n_good], before[n_good] + np.float32(delta))
    assert (mp["update"][pts] == (1 if n_loop == 0 else 0)).all() and not mp["update"][info["n_pt"]:].any()


def _untouched(kf, mp, info):
    return (not kf["set_pose"].any() and not mp["set_pos"].any() and not mp["update"].any() and not kf["gba_rows"].any() and
            not mp["gba_rows"].any() and kf["pose"].tobytes() == info["poses"].tobytes() and mp["pos"].tobytes() == info["points"].tobytes())


def test_a_stop_flag_on_entry_leaves_the_map_alone(tmp_path):
    _build()
    s, raw, info = _scene("robust_5", stop=1)
    out, err = _exe(tmp_path, raw, "run")
    _, kf, mp, _ = _read_map(out, info["n_kf"] + 2, info["n_pt"] + 2)
    assert _untouched(kf, mp, info) and "orbfe" not in err


def test_without_a_device_the_map_is_left_alone_and_the_error_is_reported(tmp_path):
    _build()
    if _gpu():
        pytest.skip("a GPU is present")
    s, raw, info = _scene("robust_5")
    out, err = _exe(tmp_path, raw, "run")
    _, kf, mp, _ = _read_map(out, info["n_kf"] + 2, info["n_pt"] + 2)
    assert _untouched(kf, mp, info) and "orbfe BundleAdjustment" in err and "no CPU fallback" in err


def test_a_map_beyond_the_limits_is_left_alone_and_the_error_is_reported(tmp_path):
    """65 free keyframes: refused by the library before a device is looked for"""
    _build()
    n = _lib.LBA_MAX_FREE + 2
    cam = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, mbf=40.0)
    kfs = [(k, 0, B.IDENTITY, [(320.0, 240.0, 0, -1.0)]) for k in range(n)]
    mps = [(100, 0, np.array([0, 0, 5], np.float32), [(k, 0) for k in range(n)])]
    out, err = _exe(tmp_path, _pack(cam, SIG, kfs, mps, [1] * n, 5, 1, 0, 0), "run")
    _, kf, mp, _ = _read_map(out, n, 1)
    assert not kf["set_pose"].any() and not mp["set_pos"].any() and "free keyframes" in err


@pytest.mark.gpu
@pytest.mark.parametrize("name, n_loop", [("robust_5", 0), ("plain_10", 3), ("nothing_fixed", 0)])
def test_the_map_afterwards_against_the_reading(tmp_path, name, n_loop):
    _build()
    s, raw, info = _scene(name, n_loop=n_loop)
    ref = B.reference(name)
    out, err = _exe(tmp_path, raw, "run")
    _, kf, mp, _ = _read_map(out, info["n_kf"] + 2, info["n_pt"] + 2)
    good, pts = np.arange(info["n_kf"]), np.arange(info["n_pt"])
    poses, points = (kf["pose"], mp["pos"]) if n_loop == 0 else (kf["gba"], mp["gba"])
    ratio = B.worst_ratio(poses[good], points[pts], ref["poses"], ref["points"])
    print(f"drop-in {name} (nLoopKF {n_loop}): max diff / tolerance {ratio:.4f}")
    assert err == "" and ratio <= 1.0
    if n_loop == 0:
        assert (kf["set_pose"][good] == 1).all() and (mp["set_pos"][pts] == 1).all() and (mp["update"][pts] == 1).all() and not kf["gba_rows"].any()
    else:
        assert not kf["set_pose"].any() and kf["pose"].tobytes() == info["poses"].tobytes() and (kf["gba_for"][good] == n_loop).all()
        assert not mp["set_pos"].any() and (mp["gba_for"][pts] == n_loop).all()
    rest_k, rest_p = [info["bad_kf"], info["far_kf"]], [info["n_pt"], info["n_pt"] + 1]
    assert not kf["set_pose"][rest_k].any() and kf["pose"][rest_k].tobytes() == info["poses"][rest_k].tobytes()
    assert not mp["set_pos"][rest_p].any() and mp["pos"][rest_p].tobytes() == info["points"][rest_p].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["typical", "tri_99"])
def test_the_initial_map_afterwards_against_the_reading(tmp_path, name):
    """AdjustAndScaleInitialMap on the two keyframes of a two-view scene whose map points stand where the initialiser put them"""
    _build()
    s, ref = B.map_scene(name), B.map_reference(name)
    n1, n2 = len(s["keys1"]), len(s["keys2"])
    idx = ref["index"]
    kfs = [(0, 0, B.IDENTITY, [(float(x), float(y), int(o), -1.0) for (x, y), o in zip(s["keys1"], s["octaves1"])]),
           (1, 0, np.concatenate([s["R21"].reshape(3, 3), s["t21"].reshape(3, 1)], 1).reshape(12),
            [(float(x), float(y), int(o), -1.0) for (x, y), o in zip(s["keys2"], s["octaves2"])])]
    mps = [(100 + k, 0, s["P3D"][i], [(0, int(i)), (1, int(s["matches12"][i]))]) for k, i in enumerate(idx)]
    sig = list(s["inv_level_sigma2"])
    out, err = _exe(tmp_path, _pack(s["cam"], sig, kfs, mps, [1, 1], 20, 1, 0, 0), "initmap")
    ret, kf, mp, tail = _read_map(out, 2, len(idx))
    res = np.frombuffer(tail, INITIAL_MAP_RESULT_DTYPE, 1)[0]
    print(f"drop-in initial map {name}: returned {ret}, {int(res['n_points'])} points, median depth {float(res['median_depth'])!r} (reading "
          f"{float(ref['median_depth'])!r}), reason {int(res['reason'])}/{ref['reason']}")
    assert err == "" and bool(ret) == ref["success"] and (int(res["n_points"]), int(res["reason"])) == (ref["n_points"], ref["reason"])
    assert (mp["update"] == 1).all() and (mp["set_pos"] == (2 if ret else 1)).all()
    assert kf["set_pose"].tolist() == ([1, 2] if ret else [1, 1])
    # What stands in the map is what the library's finish stage made of the library's adjustment.  Against the reading, derived from
    # the number formats: before the rescale a coordinate is within the parity tolerance u = 2^-23 max(1, |X|_inf) of the reading's;
    # the median is the depth of one point, so within that point's u; 1.0f / median adds half a unit in the last place, the product
    # another half.  Hence |d (X / m)| <= u / |m| + |X / m| (u_m / |m| + 2^-24 + 2^-24).  A reset rescales nothing: the parity criterion.
    if ret:
        U, m = ref["unscaled_points"].astype(np.float64), float(ref["median_depth"])
        k = int(np.flatnonzero(ref["depths"] == ref["median_depth"])[0])
        m_rel = 2.0 ** -23 * max(1.0, np.abs(U[k]).max()) / abs(m) + 2.0 ** -23
        tol = lambda before, after: 2.0 ** -23 * np.maximum(1.0, np.abs(before).max(axis=-1, keepdims=True)) / abs(m) + np.abs(after).max(axis=-1, keepdims=True) * m_rel
        t_u, t_s = ref["unscaled_poses"][1, [3, 7, 11]].astype(np.float64), ref["poses"][1, [3, 7, 11]].astype(np.float64)
        r_points = float((np.abs(mp["pos"].astype(np.float64) - ref["points"]) / tol(U, ref["points"].astype(np.float64))).max())
        r_t = float((np.abs(kf["pose"][1, [3, 7, 11]].astype(np.float64) - t_s) / tol(t_u, t_s)).max())
    else:
        r_points = B.worst_ratio([], mp["pos"], [], ref["points"])
        r_t = B.worst_ratio(kf["pose"][1:], [], ref["poses"][1:], [])
    print(f"  in the map against the reading, difference / bound: points {r_points:.4f}, translation {r_t:.4f}")
    assert r_points <= 1.0 and r_t <= 1.0
    assert B.worst_ratio(kf["pose"][:1], [], ref["poses"][:1], []) <= 1.0
    assert np.abs(kf["pose"][1].reshape(3, 4)[:, :3].astype(np.float64) - ref["poses"][1].reshape(3, 4)[:, :3]).max() <= 2.0 ** -23
