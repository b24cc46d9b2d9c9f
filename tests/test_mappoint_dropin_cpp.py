"""csrc/host/MapPoint_hip.h -- the batched MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth -- on the mock MapPoint /
KeyFrame of tests/cpp_mappoint: builds everywhere and fails loudly without a device (a log line, every point as it was); on the GPU a
scripted map (points with 1 to about 100 observations, bad keyframes, bad points, points without observations, a point whose
observers are all bad) gives, point by point, the results of the Python mirror, which tests/test_mappoint_gpu.py ties to the
reading."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_mappoint as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_mappoint", "_build", "test_mappoint_dropin")
BEFORE = bytes([0xEE]) * 32 + np.array([7, 7, 7, -1, -2], np.float32).tobytes()


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_mappoint")], check=True, capture_output=True)


def _script():
    """the scene (observations in keyframe order: the mock's std::map orders by address and its keyframes lie in one array), the
    keypoint octaves, which points are bad"""
    sizes = [1, 2, 3, 5, 8, 13, 21, 40, 63, 64, 65, 80, 100, 0, 4, 6, 0, 30]
    s = M.make_scene(55, sizes)
    rng = np.random.default_rng(56)
    for kf in s["keyframes"]:
        kf["octave"] = rng.integers(0, 8, len(kf["desc"])).astype(np.int32)
    n_kf = len(s["keyframes"])
    for k in range(3):   # three keyframes, all bad, that only the last point sees
        s["keyframes"].append(dict(desc=rng.integers(0, 256, (2, 32), dtype=np.uint8), bad=True, Ow=rng.uniform(-5, 5, 3).astype(np.float32),
                                   octave=np.array([1, 2], np.int32)))
    s["points"].append(dict(obs=[(n_kf + k, k % 2) for k in range(3)], pos=np.array([3, -2, 25], np.float32), ref=1, ref_octave=0))
    for p in s["points"]:
        ref_kf = p["obs"][p["ref"]][0] if p["obs"] else -1
        p["obs"] = sorted(p["obs"])
        p["ref_kf"] = ref_kf
        if p["obs"]:
            p["ref"] = [kf for kf, _ in p["obs"]].index(ref_kf)
            p["ref_octave"] = int(s["keyframes"][ref_kf]["octave"][p["obs"][p["ref"]][1]])
    bad_points = {3, 11}
    return s, bad_points


def _serialise(s, bad_points):
    sf = s["scale_factors"]
    b = struct.pack("<i", len(sf)) + sf.tobytes() + struct.pack("<ii", len(s["keyframes"]), len(s["points"]))
    for kf in s["keyframes"]:
        b += struct.pack("<i3fi", int(kf["bad"]), *[float(x) for x in kf["Ow"]], len(kf["desc"])) + kf["desc"].tobytes() + kf["octave"].tobytes()
    for i, p in enumerate(s["points"]):
        b += struct.pack("<i3fii", int(i in bad_points), *[float(x) for x in p["pos"]], p["ref_kf"], len(p["obs"]))
        b += np.array(p["obs"], np.int32).reshape(-1, 2).tobytes()
    return b


def _run(tmp_path, s, bad_points, mode):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(_serialise(s, bad_points))
    r = subprocess.run([EXE, pin, pout, str(mode)], capture_output=True, text=True)
    raw = open(pout, "rb").read() if os.path.exists(pout) else b""
    return r, [raw[o:o + 52] for o in range(0, len(raw), 52)]


def _gpu_present():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_dropin_builds_and_fails_loudly_without_a_device(tmp_path):
    _build()
    assert os.path.exists(EXE)
    s, bad_points = _script()
    r, out = _run(tmp_path, s, bad_points, 0)
    assert len(out) == len(s["points"])
    if _gpu_present():
        assert r.returncode == 0, r.stderr[-2000:]
        return
    assert r.returncode == 3 and all(o == BEFORE for o in out)
    assert "orbfe_refresh_map_points failed" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_dropin_equals_the_mirror_point_by_point(tmp_path, mode):
    from refactored_orb_slam2_amd import map_point
    _build()
    s, bad_points = _script()
    r, out = _run(tmp_path, s, bad_points, mode)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    want = map_point.refresh_map_points(s["keyframes"], s["points"], s["scale_factors"])
    assert want.tobytes() == M.run(s).tobytes()
    changed = kept_desc = 0
    for i, (p, o) in enumerate(zip(s["points"], out)):
        if i in bad_points or not p["obs"]:
            assert o == BEFORE, i
            continue
        w = want[i]
        floats = w["normal"].tobytes() + w["min_distance"].tobytes() + w["max_distance"].tobytes()
        assert o[32:] == floats, i
        if w["best"] < 0:
            assert o[:32] == BEFORE[:32], i
            kept_desc += 1
        else:
            assert o[:32] == w["desc"].tobytes(), i
        changed += 1
    assert changed >= 14 and kept_desc == 1
