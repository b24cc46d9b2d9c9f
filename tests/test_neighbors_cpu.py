"""LocalMapping::SearchInNeighbors with all Fuse calls batched, without a device: mapping.search_in_neighbors on the numpy row search
against the sequential reading of tests/np_neighbors.py (operation log and final map state), the census of the scenes, the negative
control with the repair searches switched off, and the argument validation of the orbfe_fuse_batch_* exports."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, mapping
from tests import np_neighbors as N


@pytest.fixture(scope="module")
def scenes():
    return N.scenes()


@pytest.fixture(scope="module")
def sequential(scenes):
    out = []
    for s in scenes:
        c = N.clone(s)
        log, n_fused, notes = N.sequential(c["map"], c["current"], c["targets"])
        out.append(dict(log=log, n_fused=n_fused, notes=notes, state=c["map"].state()))
    return out


def _batched(scene, **kw):
    c = N.clone(scene)
    backends = []

    def make(m, targets, th):
        backends.append(N.NumpySearch(m, targets, th, **kw))
        return backends[-1]
    r = mapping.search_in_neighbors(c["map"], c["current"], c["targets"], search=make)
    return r, c["map"].state(), backends


@pytest.mark.parametrize("i", range(len(N.SCENE_SEEDS)))
def test_batched_protocol_equals_the_sequential_reading(scenes, sequential, i):
    """one full search, the replay in target order, a repair search where a descriptor changed: the reference's operations, one for one"""
    r, state, backends = _batched(scenes[i])
    want = sequential[i]
    assert r["log"] == want["log"]
    assert r["n_fused"] == want["n_fused"]
    assert state == want["state"]
    kinds = {op[0] for op in r["log"]}
    assert kinds == {"target", "add", "replace", "bad"}
    # the forward pass: one full search and at most one repair per target boundary, each over a handful of points and the targets ahead
    fwd = backends[0].calls
    assert fwd[0] == (None, 0) and r["n_full"] == 2 and r["n_repair"] == len(fwd) - 1
    K = len(scenes[i]["targets"])
    assert 2 <= r["n_repair"] <= K - 1
    firsts = [ft for _, ft in fwd[1:]]
    assert firsts == sorted(set(firsts)) and all(0 < ft < K for ft in firsts)
    assert all(idx == sorted(set(idx)) and 0 < len(idx) <= 8 for idx, _ in fwd[1:])
    assert backends[1].calls == [(None, 0)]           # the reverse pass needs no repair
    print(f"scene {scenes[i]['seed']}: {len(r['log'])} log entries, n_fused {r['n_fused']}, repair searches {fwd[1:]}")


def test_census_is_complete(sequential):
    """every event of the issue's table is reached (a condition on the scenes, not a measurement)"""
    union = set()
    for s in sequential:
        got = N.census(s["notes"])
        union |= got
        assert got == set(N.TAGS), sorted(set(N.TAGS) - got)      # the builder places every event in every scene
    assert union == set(N.TAGS)


@pytest.mark.parametrize("i", range(len(N.SCENE_SEEDS)))
def test_without_the_repair_the_scenes_diverge(scenes, sequential, i):
    """negative control: the scenes do reach the stale path -- with the repair searches off the log and the state differ"""
    assert {"a", "b"} <= N.census(sequential[i]["notes"])
    r, state, backends = _batched(scenes[i], no_repair=True)
    assert r["n_repair"] == 0 and len(backends[0].calls) == 1
    assert r["log"] != sequential[i]["log"]
    assert state != sequential[i]["state"]


def test_a_point_held_twice_is_refused(scenes):
    c = N.clone(scenes[0])
    mp = c["map"].kfs[c["current"]].mp
    mp[1] = mp[0]
    with pytest.raises(ValueError):
        mapping.search_in_neighbors(c["map"], c["current"], c["targets"], search=lambda m, t, th: N.NumpySearch(m, t, th))


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def _target(n, bounds=(0, 640, 0, 480)):
    k = np.zeros(max(n, 1), _lib.KP_DTYPE)
    i = np.arange(len(k))
    k["x"], k["y"] = i % 640, (i // 640) * 4 % 480        # spread over the grid: no cell holds more than a few
    d = np.zeros((max(n, 1), 32), np.uint8)
    return _lib.FrameView(n, k.ctypes.data, d.ctypes.data, None, *bounds), (k, d)


def _create(L, views, cams, inv, mode=_lib.KF_FUSE, K=None, out=True):
    h = C.c_void_p(None)
    arr = (_lib.FrameView * max(len(views), 1))(*views) if views is not None else None
    rc = L.orbfe_fuse_batch_create(len(views) if K is None else K, None if arr is None else C.cast(arr, C.c_void_p), _lib.ptr(cams),
                                   _lib.ptr(inv), mode, C.byref(h) if out else None)
    return rc, h


def test_create_validates_before_a_device_is_looked_for(L):
    """each limit of orbfe_fuse_batch_create at its last accepted and its first refused value.  A refusal is ORBFE_ERR_INVALID with a
    text, made before a device is looked for and before anything is allocated or read; an accepted call goes on to the device (and
    without one is ORBFE_ERR_NO_DEVICE)."""
    accepted = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    cam = np.zeros(1, _lib.KF_CAMERA_DTYPE); cam["n_levels"] = 8
    inv = np.ones((1, 16), np.float32)

    def ok(rc, h):
        assert rc == accepted, L.orbfe_last_error()
        assert bool(h.value) == (accepted == _lib.OK)
        assert L.orbfe_fuse_batch_destroy(h) == _lib.OK

    def refused(rc, h, text=b"fuse batch"):
        assert rc == _lib.ERR_INVALID and not h.value
        assert text in L.orbfe_last_error()

    v1, keep1 = _target(1)
    ok(*_create(L, [v1], cam, inv))
    ok(*_create(L, [], None, None))                                       # K = 0: a batch that launches nothing
    refused(*_create(L, [], None, None, K=-1))
    v, keep = _target(65535); ok(*_create(L, [v], cam, inv))              # the keypoint limit of the projection searches
    big = _lib.FrameView(65536, keep[0].ctypes.data, keep[1].ctypes.data, None, 0, 640, 0, 480)   # refused before the arrays are read
    refused(*_create(L, [big], cam, inv))
    refused(*_create(L, [_lib.FrameView(-1, None, None, None, 0, 640, 0, 480)], cam, inv))
    v0 = _lib.FrameView(0, None, None, None, 0, 640, 0, 480); ok(*_create(L, [v0], cam, inv))   # an empty target needs no arrays
    for n_levels, good in ((1, True), (16, True), (0, False), (17, False)):
        c = cam.copy(); c["n_levels"] = n_levels
        (ok if good else refused)(*_create(L, [v1], c, inv))
    for mode, good in ((_lib.KF_FUSE, True), (_lib.KF_FUSE_SIM3, True), (0, False), (_lib.KF_SIM3, False)):
        (ok if good else refused)(*_create(L, [v1], cam, inv, mode=mode))
    ok(*_create(L, [v1], cam, None, mode=_lib.KF_FUSE_SIM3))              # no chi-square gate: no table
    refused(*_create(L, [v1], cam, None))
    refused(*_create(L, None, cam, inv, K=1))
    refused(*_create(L, [v1], None, inv))
    assert _create(L, [v1], cam, inv, out=False)[0] == _lib.ERR_INVALID
    refused(*_create(L, [_lib.FrameView(1, None, keep1[1].ctypes.data, None, 0, 640, 0, 480)], cam, inv))
    refused(*_create(L, [_lib.FrameView(1, keep1[0].ctypes.data, keep1[1].ctypes.data, None, 0, 0, 0, 480)], cam, inv))
    cams2 = np.concatenate([cam, cam]); inv2 = np.ones((2, 16), np.float32)
    other, keep2 = _target(1, (0, 641, 0, 480))
    ok(*_create(L, [v1, v1], cams2, inv2))
    ok(*_create(L, [v1, other], cams2, inv2))                             # targets may have image bounds of their own


def test_create_device_and_search_validate(L):
    h = C.c_void_p(None)
    one = C.c_void_p(16)     # never dereferenced: every call below is refused, or ends at the missing device

    def create_device(K=1, keys=one, desc=one, n=one, cap=1, bounds=(0.0, 640.0, 0.0, 480.0), cams=one, inv=one, mode=_lib.KF_FUSE, out=True):
        return L.orbfe_fuse_batch_create_device(K, keys, desc, None, n, cap, *bounds, cams, inv, mode, None, C.byref(h) if out else None)

    for kw in (dict(K=-1), dict(cap=0), dict(cap=65536), dict(keys=None), dict(desc=None), dict(n=None), dict(cams=None), dict(inv=None),
               dict(mode=_lib.KF_LOOP), dict(bounds=(0.0, 0.0, 0.0, 480.0)), dict(bounds=(0.0, 640.0, 5.0, 5.0)), dict(out=False),
               dict(desc=C.c_void_p(8))):
        assert create_device(**kw) == _lib.ERR_INVALID and not h.value, kw
    if not _gpu_present(L):   # accepted arguments go on to the device; with one these fake addresses must not
        for kw in (dict(), dict(cap=65535), dict(K=0, keys=None, desc=None, n=None, cams=None, inv=None), dict(inv=None, mode=_lib.KF_FUSE_SIM3)):
            assert create_device(**kw) == _lib.ERR_NO_DEVICE and not h.value, kw
            assert b"no CPU fallback" in L.orbfe_last_error()
    # the searches need a handle
    res = np.zeros(1, _lib.KF_RESULT_DTYPE); pts = np.zeros(1, _lib.KF_POINT_DTYPE)
    assert L.orbfe_fuse_batch_search(None, pts.ctypes.data, 1, None, 0, 0, None, res.ctypes.data) == _lib.ERR_INVALID
    assert L.orbfe_fuse_batch_search_device(None, one, 1, None, 0, 0, None, one, None) == _lib.ERR_INVALID
    assert L.orbfe_fuse_batch_destroy(None) == _lib.OK


def test_no_device_is_an_error(L):
    if _gpu_present(L):
        pytest.skip("a GPU is present")
    from refactored_orb_slam2_amd.matcher import FrameView, FuseBatch
    k = np.zeros(4, _lib.KP_DTYPE); d = np.zeros((4, 32), np.uint8)
    cam = np.zeros(1, _lib.KF_CAMERA_DTYPE); cam["n_levels"] = 8
    with pytest.raises(_lib.OrbfeError) as e:
        FuseBatch([FrameView(k, d, 0, 640, 0, 480)], cam, [np.ones(8, np.float32)])
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    s = N.scenes()[0]
    with pytest.raises(_lib.OrbfeError):
        mapping.search_in_neighbors(s["map"], s["current"], s["targets"])    # the default backend is the device: no fallback


def test_host_code_is_clean_under_sanitizers(L):
    """tests/cpp_neighbors/fuse_host_sanitize.cpp: csrc/fuse.cpp compiled with -fsanitize=address,undefined and linked with a main of its
    own (no device, no Python in the process).  It drives every orbfe_fuse_batch_* entry point through its refusals, checks K x n_points
    within int32_t and the index list at their last accepted and first refused values, and runs the staging arithmetic on real buffers."""
    import os
    import shutil
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    if _gpu_present(L):   # the program expects every accepted call to end at the missing device, and sanitizers stay away from GPUs
        pytest.skip("a GPU is present")
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp_neighbors")
    r = subprocess.run(["make", "-C", d, "sanitize", "HIPCC=" + hipcc], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fuse host code: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
