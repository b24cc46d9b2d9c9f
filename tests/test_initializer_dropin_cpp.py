"""csrc/host/Initializer_hip.h -- orbfe_host::Initializer, the class with the constructor and the Initialize() signature of
ORB_SLAM2::Initializer -- on the mock Frame of tests/cpp_initializer: builds everywhere and fails loudly without a device; on the GPU
Initialize() hands back what the Python mirror computes on the sets the adapter drew, and the first call's sets are the reference's
draw from rand() seeded with 0.  (Later calls go on in the same process-wide rand() stream, which this test does not own: their sets
are checked to be draws, not replayed.)"""
import ctypes as C
import ctypes.util
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, initializer
from tests import initializer_host as IH
from tests import np_initializer as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_initializer", "_build", "test_initializer_dropin")
ITERATIONS = 48


def _run(tmp_path, name, calls):
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_initializer")], check=True, capture_output=True)
    c = Y.solved(name)
    p = c["params"]
    n1, n2 = len(c["keys1"]), len(c["keys2"])
    blob = struct.pack("<5f4i", p[0], p[1], p[2], p[3], p[4], ITERATIONS, calls, n1, n2)
    blob += c["keys1"].astype("<f4").tobytes() + c["keys2"].astype("<f4").tobytes() + c["matches12"].astype("<i4").tobytes()
    fin, fout = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    fin.write_bytes(blob)
    r = subprocess.run([EXE, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    raw, off, out = fout.read_bytes(), 0, []
    for _ in range(calls):
        ok = struct.unpack_from("<i", raw, off)[0]; off += 4
        res = np.frombuffer(raw, _lib.INIT_RESULT_DTYPE, 1, off)[0]; off += 224
        sets = np.frombuffer(raw, "<i4", ITERATIONS * 8, off).reshape(ITERATIONS, 8); off += ITERATIONS * 32
        Rt = np.frombuffer(raw, "<f4", 12, off); off += 48
        p3d = np.frombuffer(raw, "<f4", n1 * 3, off).reshape(n1, 3); off += n1 * 12
        tri = np.frombuffer(raw, np.uint8, n1, off).astype(bool); off += n1
        out.append({"ok": ok, "result": res, "sets": sets, "R21": Rt[:9], "t21": Rt[9:], "P3D": p3d, "triangulated": tri})
    assert off == len(raw)
    return c, out, r.stderr


def _gpu_present():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_adapter_builds_and_fails_loudly_without_a_device(tmp_path):
    c, out, err = _run(tmp_path, "general", 1)
    if _gpu_present():
        assert out[0]["ok"] == 1
        return
    assert out[0]["ok"] == 0 and "orbfe_initializer_initialize failed" in err and "no HIP device" in err
    assert not out[0]["P3D"].any() and not out[0]["triangulated"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["general", "plane"])
def test_adapter_equals_the_python_mirror_on_its_own_sets(tmp_path, name):
    c, out, _ = _run(tmp_path, name, 2)
    N = int((c["matches12"] >= 0).sum())
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.srand(0)                                            # DUtils::Random::SeedRandOnce(0); RAND_MAX of glibc
    below = lambda k: int(libc.rand() / (2147483647 + 1.0) * k)
    assert np.array_equal(out[0]["sets"], initializer.draw_sets(N, ITERATIONS, below))
    for call in out:
        assert all(len(set(r)) == 8 and min(r) >= 0 and max(r) < N for r in call["sets"].tolist())
        ref = initializer.initialize(IH.params_of(c["params"]), c["keys1"], c["keys2"], c["matches12"], call["sets"])
        assert call["result"].tobytes() == ref["result"].tobytes()
        assert call["ok"] == int(ref["result"]["success"])
        if call["ok"]:
            assert np.array_equal(call["R21"], ref["result"]["R21"]) and np.array_equal(call["t21"], ref["result"]["t21"])
            assert np.array_equal(call["P3D"], ref["P3D"]) and np.array_equal(call["triangulated"], ref["triangulated"])
            assert call["triangulated"].sum() == int(ref["result"]["n_triangulated"]) > 50
    if name == "general":
        assert out[0]["ok"] == 1 and int(out[0]["result"]["model"]) == 2
    else:
        assert int(out[0]["result"]["model"]) == 1
