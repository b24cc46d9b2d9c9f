"""csrc/host/Optimizer_hip.h -- orbfe_host::PoseOptimization, the body that replaces Optimizer::PoseOptimization -- on the mock
Frame / MapPoint of tests/cpp_pose: builds everywhere and fails loudly without a device; on the GPU it leaves in the Frame what the
Python host form returns, byte for byte."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from tests import np_pose as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_pose", "_build", "test_pose_dropin")


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_pose")], check=True, capture_output=True)


def _keys(s):
    k = np.zeros(len(s["keys_xy"]), _lib.KP_DTYPE)
    k["x"], k["y"], k["octave"] = s["keys_xy"][:, 0], s["keys_xy"][:, 1], s["octave"]
    return k


def _run(tmp_path, s, outlier_in):
    c = s["cam"]
    cam = optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["inv_level_sigma2"])
    n = len(s["keys_xy"])
    ur = np.full(n, -1, np.float32) if s["u_right"] is None else s["u_right"]
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(struct.pack("<i", n) + _keys(s).tobytes() + ur.astype(np.float32).tobytes() + s["assigned"].astype(np.int32).tobytes())
        f.write(struct.pack("<i", len(s["points"])) + s["points"].astype(np.float32).tobytes() + cam.tobytes())
        f.write(s["Tcw_in"].astype(np.float32).tobytes() + outlier_in.astype(np.uint8).tobytes())
    r = subprocess.run([EXE, pin, pout], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(pout):
        return r, None
    raw = open(pout, "rb").read()
    ret, calls = struct.unpack("<ii", raw[:8])
    return r, (ret, calls, np.frombuffer(raw[8:56], np.float32), np.frombuffer(raw[56:], np.uint8))


def test_pose_dropin_builds_and_fails_loudly_without_device(tmp_path):
    _build()
    n = C.c_int(0)
    gpu = _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    s = P.case_scene("edges_40")
    r, got = _run(tmp_path, s, np.ones(len(s["keys_xy"]), np.uint8))
    assert r.returncode == 0 and got is not None, r.stderr
    if not gpu:      # logged, never thrown; the Frame is untouched and the function returns 0
        ret, calls, T, out = got
        assert "no CPU fallback" in r.stderr and ret == 0 and calls == 0
        assert np.array_equal(T, s["Tcw_in"]) and out.all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standard", "u_right_null", "edges_9", "edges_2"])
def test_pose_dropin_equals_the_python_host_form(tmp_path, name):
    _build()
    s = P.case_scene(name)
    n = len(s["keys_xy"])
    c = s["cam"]
    cam = optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["inv_level_sigma2"])
    res, outlier = optimizer.pose_optimization(_keys(s), s["u_right"], s["assigned"], s["points"], cam, s["Tcw_in"])
    r, got = _run(tmp_path, s, np.ones(n, np.uint8))
    assert r.returncode == 0 and got is not None, r.stdout + r.stderr
    ret, calls, T, out = got
    has = s["assigned"] >= 0
    assert ret == int(res["n_inliers"])
    assert np.array_equal(out[has], outlier[has]) and out[~has].all()          # entries without a point stay as they were
    if int(res["n_initial"]) < 3:
        assert ret == 0 and calls == 0 and np.array_equal(T, s["Tcw_in"])
    else:
        assert calls == 1 and T.tobytes() == np.asarray(res["Tcw"], np.float32).tobytes()
