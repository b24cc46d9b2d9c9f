"""csrc/host/Optimizer_hip.h -- orbfe_host::GlobalBundleAdjustemnt on a mock map of MORE than 64 keyframes (tests/cpp_gba): the
adapter, compiled with ORBFE_HOST_GLOBAL_BA_ACROSS_DEVICE as tests/cpp_gba does, hands a map within the ORBFE_LBA_MAX_* limits to
orbfe_bundle_adjustment and any other to orbfe_global_bundle_adjustment (without the definition it refuses such a map as before:
tests/test_ba_dropin_cpp.py).  Without a GPU: such a map is no longer refused for its size -- the call gets as far as looking for
a device -- and is left alone.  With a GPU: the map afterwards against the numpy reading, once written into the map (nLoopKF == 0)
and once beside it (nLoopKF != 0: mTcwGBA / mPosGBA / mnBAGlobalForKF, poses and positions untouched)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_ba as B
from tests import np_gba as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_gba", "_build", "test_gba_dropin")
SIG = np.array([1.0 / (1.2 ** l) ** 2 for l in range(8)], np.float32)
KF_OUT = np.dtype([("set_pose", "<i4"), ("pose", "<f4", (12,)), ("gba_for", "<i4"), ("gba_rows", "<i4"), ("gba", "<f4", (12,))])
MP_OUT = np.dtype([("set_pos", "<i4"), ("update", "<i4"), ("pos", "<f4", (3,)), ("gba_for", "<i4"), ("gba_rows", "<i4"), ("gba", "<f4", (3,))])
CASE = "long_72_robust_5"                      # five robust iterations: GlobalBundleAdjustemnt(pMap, 5)


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_gba")], check=True, capture_output=True)


def _map(n_iterations, robust, n_loop, stop=0):
    """the case as a map: keyframe k has mnId k (keyframe 0 is the fixed one), its keypoints are its observations in edge order"""
    s = G.case_scene(CASE)
    cam = s["cam"]
    n_kf, n_pt = len(s["poses"]), len(s["points"])
    assert n_kf > _lib.LBA_MAX_FREE + 1 and s["fixed"].tolist() == [1] + [0] * (n_kf - 1)
    kps, obs = [[] for _ in range(n_kf)], [[] for _ in range(n_pt)]
    for e in s["edges"]:
        obs[e["point"]].append((int(e["kf"]), len(kps[e["kf"]])))
        kps[e["kf"]].append((float(e["u"]), float(e["v"]), int(np.argmin(np.abs(SIG - e["inv_sigma2"]))), float(e["u_right"])))
    out = [struct.pack("<5f", cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"]), struct.pack("<i", len(SIG)), SIG.tobytes(),
           struct.pack("<i", n_kf)]
    for k in range(n_kf):
        out.append(struct.pack("<ii", k, 0) + s["poses"][k].tobytes() + struct.pack("<i", len(kps[k])))
        out += [struct.pack("<ffif", *kp) for kp in kps[k]]
    out.append(struct.pack("<i", n_pt))
    for p in range(n_pt):
        out.append(struct.pack("<ii", 100 + p, 0) + s["points"][p].tobytes() + struct.pack("<i", len(obs[p])))
        out += [struct.pack("<ii", k, i) for k, i in obs[p]]
    out.append(np.ones(n_kf, np.int32).tobytes())
    out.append(struct.pack("<4i", n_iterations, int(robust), n_loop, stop))
    return s, b"".join(out)


def _exe(tmp_path, raw, n_kf, n_pt):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(raw)
    r = subprocess.run([EXE, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = fout.read_bytes()
    return np.frombuffer(out, KF_OUT, n_kf, 4), np.frombuffer(out, MP_OUT, n_pt, 4 + n_kf * KF_OUT.itemsize), r.stderr


def _gpu():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_a_map_of_more_than_64_keyframes_is_no_longer_refused_for_its_size(tmp_path):
    _build()
    if _gpu():
        pytest.skip("a GPU is present")
    s, raw = _map(5, True, 0)
    kf, mp, err = _exe(tmp_path, raw, len(s["poses"]), len(s["points"]))
    assert "orbfe BundleAdjustment" in err and "no CPU fallback" in err and "free keyframes" not in err
    assert not kf["set_pose"].any() and not mp["set_pos"].any() and not mp["update"].any() and not kf["gba_rows"].any()
    assert kf["pose"].tobytes() == s["poses"].tobytes() and mp["pos"].tobytes() == s["points"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_loop", [0, 7])
def test_the_map_afterwards_against_the_reading(tmp_path, n_loop):
    """GlobalBundleAdjustemnt(pMap, 5) as LoopClosing calls it (nLoopKF != 0) and as Tracking does (nLoopKF == 0)"""
    _build()
    s, raw = _map(5, True, n_loop)
    assert (s["n_iterations"], s["robust"]) == (5, True)
    ref = G.reference(CASE)
    kf, mp, err = _exe(tmp_path, raw, len(s["poses"]), len(s["points"]))
    poses, points = (kf["pose"], mp["pos"]) if n_loop == 0 else (kf["gba"], mp["gba"])
    ratio = B.worst_ratio(poses, points, ref["poses"], ref["points"])
    print(f"drop-in {CASE} (nLoopKF {n_loop}): {len(s['poses'])} keyframes, max diff / tolerance {ratio:.4f}")
    assert err == "" and ratio <= 1.0
    if n_loop == 0:
        assert (kf["set_pose"] == 1).all() and (mp["set_pos"] == 1).all() and (mp["update"] == 1).all()
        assert not kf["gba_rows"].any() and not mp["gba_rows"].any()
    else:
        assert not kf["set_pose"].any() and kf["pose"].tobytes() == s["poses"].tobytes() and (kf["gba_for"] == n_loop).all()
        assert not mp["set_pos"].any() and mp["pos"].tobytes() == s["points"].tobytes() and (mp["gba_for"] == n_loop).all()
        assert (kf["gba_rows"] == 4).all() and (mp["gba_rows"] == 3).all()
