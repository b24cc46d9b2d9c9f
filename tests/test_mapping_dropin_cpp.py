"""csrc/host/LocalMapping_hip.h -- orbfe_host::CreateNewMapPoints, the loop that replaces the neighbour loop of
LocalMapping::CreateNewMapPoints -- on the mock KeyFrame of tests/cpp_mapping: builds everywhere and fails loudly without a device;
on the GPU it hands back what the replay of oracle search, numpy reading and mask update expects, and the bytes of the Python mirror."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, mapping
from tests import np_mapping as M
from tests import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_mapping", "_build", "test_mapping_dropin")


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_mapping")], check=True, capture_output=True)


def _keyframe_bytes(kf, median_depth=0.0):
    n, stereo = len(kf["keys"]), kf["u_right"] is not None
    b = struct.pack("<ii", n, int(stereo)) + kf["keys"].tobytes() + np.ascontiguousarray(kf["desc"], np.uint8).tobytes()
    if stereo:
        b += kf["u_right"].astype(np.float32).tobytes() + kf["depth"].astype(np.float32).tobytes()
    b += kf["has_mp"].astype(np.uint8).tobytes() + np.ascontiguousarray(kf["view"], _lib.TRI_VIEW_DTYPE).tobytes()
    b += struct.pack("<fi", median_depth, len(kf["groups"]))
    for nid in sorted(kf["groups"]):
        idx = np.asarray(kf["groups"][nid], np.int32)
        b += struct.pack("<ii", nid, len(idx)) + idx.tobytes()
    return b


def _run(tmp_path, sc):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(struct.pack("<ii", len(sc["neighbors"]), int(sc["monocular"])) + _keyframe_bytes(sc["A"]))
        for nb in sc["neighbors"]:
            f.write(_keyframe_bytes(nb, nb["median_depth"]) + np.ascontiguousarray(nb["epipolar"], _lib.EPIPOLAR_DTYPE).tobytes())
    r = subprocess.run([EXE, pin, pout], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(pout):
        return r, None
    raw = open(pout, "rb").read()
    ret, calls = struct.unpack("<ii", raw[:8])
    off, res = 8, []
    rec = np.dtype([("idx1", "<i4"), ("idx2", "<i4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                    ("max_distance", "<f4")])
    while off < len(raw):
        skipped, nm, npts = struct.unpack("<iii", raw[off:off + 12])
        off += 12
        res.append((skipped, nm, np.frombuffer(raw[off:off + npts * rec.itemsize], rec)))
        off += npts * rec.itemsize
    return r, (ret, calls, res)


def test_mapping_dropin_builds_and_fails_loudly_without_device(tmp_path):
    _build()
    n = C.c_int(0)
    gpu = _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    r, got = _run(tmp_path, M.make_chain_scene(seed=45, n=60))
    assert r.returncode == 0 and got is not None, r.stderr
    if not gpu:      # logged, never thrown: -1 and nothing handed back
        assert "no CPU fallback" in r.stderr and got[0] == -1 and got[2] == []
    assert got[1] == 2                                   # ComputeF12 is not asked for the neighbour that stands too close


@pytest.mark.gpu
@pytest.mark.parametrize("monocular", [False, True])
def test_mapping_dropin_agrees_with_the_replay(tmp_path, monocular):
    _build()
    sc = M.make_chain_scene(seed=46, n=120, monocular=monocular)
    A = sc["A"]
    pts = mapping.create_new_map_points(A["keys"], A["desc"], A["u_right"], A["depth"], A["has_mp"], A["groups"], A["view"], sc["neighbors"],
                                        monocular=monocular, check_orientation=True)[0]

    def search(*a):
        a = list(a)
        a[10] = np.ascontiguousarray(a[10]).astype(ol.EPIPOLAR_DTYPE)
        return ol.search_for_triangulation(*a)
    want, w_matches, w_new, _, adopted, _ = M.replay_chain(sc, search, device_points=pts)
    assert adopted <= M.NON_PARITY_CAP * 120 * 3
    r, got = _run(tmp_path, sc)
    assert r.returncode == 0 and got is not None, r.stdout + r.stderr
    ret, calls, res = got
    assert ret == int(w_new.sum()) and ret > 0 and len(res) == 3 and calls == 2
    for k, (skipped, nm, p) in enumerate(res):
        assert skipped == int(w_matches[k] < 0) and nm == max(int(w_matches[k]), 0)
        ok = np.nonzero(want[k]["code"] == M.OK)[0]
        assert np.array_equal(p["idx1"], ok) and np.array_equal(p["idx2"], want[k]["idx2"][ok])      # the reference's order
        for f in ("pos", "normal", "min_distance", "max_distance"):                                     # the bytes of the Python mirror
            assert p[f].tobytes() == pts[k][f][ok].tobytes(), (k, f)
