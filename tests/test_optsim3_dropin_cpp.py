"""csrc/host/Optimizer_hip.h -- orbfe_host::OptimizeSim3, the function with the signature of ORB_SLAM2::Optimizer::OptimizeSim3 -- on
the mock KeyFrame / MapPoint / Sim3 of tests/cpp_optsim3.  Without a GPU: what the adapter marshals (the filters of
Optimizer.cc:1436-1468, the i2 lookup, octave -> mvInvLevelSigma2, which vpMatches1 entries a result would null) and the logged
return 0 that leaves everything alone.  With a GPU: vpMatches1 and g2oS12 against the figures the numpy reading wrote to
tests/golden/optsim3_dropin.npz (regenerate: python -c "from tests import test_optsim3_dropin_cpp as t; t.write_fixture()")."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_optsim3 as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_optsim3", "_build", "test_optsim3_dropin")
FIXTURE = os.path.join(ROOT, "tests", "golden", "optsim3_dropin.npz")
NAMES = ("free_scale", "pairs_12_return_0", "survivors_10", "clean")
EXTRA = 20   # match slots the filters drop


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_optsim3")], check=True, capture_output=True)


def _problem(name, seed):
    """A case scene spread over N = n + 20 match slots: 20 slots spread evenly over them are ones the filters drop (no match, no map
    point in keyframe 1, a bad point on either side, a point of keyframe 2 without an index there).  Keypoint i of keyframe 1 belongs
    to slot i (the reference reads mvKeysUn[i]); keyframe 2's keypoints are permuted and found through GetIndexInKeyFrame.
    Returns the scene, the bytes of the problem and the slots that are kept."""
    s = Q.case_scene(name)
    n = len(s["pairs"])
    N = n + EXTRA
    rng = np.random.default_rng(seed)
    drop = {k * N // EXTRA: k % 5 for k in range(EXTRA)}
    kept = [i for i in range(N) if i not in drop]
    assert len(kept) == n
    perm2 = rng.permutation(N)
    kp1 = np.zeros(N, [("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])
    kp2 = kp1.copy()
    kp1["x"], kp1["y"], kp1["octave"] = 3.0, 5.0, 1                            # what a wrong lookup would pick up
    kp2["x"], kp2["y"], kp2["octave"] = 7.0, 11.0, 2
    kp1["x"][kept], kp1["y"][kept], kp1["octave"][kept] = s["pairs"]["obs1"][:, 0], s["pairs"]["obs1"][:, 1], s["oct1"]
    kp2["x"][perm2[kept]], kp2["y"][perm2[kept]], kp2["octave"][perm2[kept]] = s["pairs"]["obs2"][:, 0], s["pairs"]["obs2"][:, 1], s["oct2"]
    sig = s["inv_level_sigma2"]
    b = struct.pack("<if", int(s["fix_scale"]), float(s["th2"])) + s["sRt_in"].tobytes()
    for v, kp in ((s["view1"], kp1), (s["view2"], kp2)):
        rec = np.zeros(1, _lib.SIM3_VIEW_DTYPE)
        for k in ("Rcw", "tcw", "fx", "fy", "cx", "cy"):
            rec[k] = v[k]
        b += rec.tobytes() + struct.pack("<i", N) + kp.tobytes() + struct.pack("<i", len(sig)) + sig.tobytes()
    b += struct.pack("<i", N)
    j = 0
    for i in range(N):
        m = [1, 1, 0, 0, int(perm2[i])]
        X = np.full(6, 7.0, np.float32)
        if i in drop:
            kind = drop[i]
            if kind == 0: m[0] = 0
            elif kind == 1: m[1] = 0
            elif kind == 2: m[2] = 1
            elif kind == 3: m[3] = 1
            else: m[4] = -1
        else:
            X[:3], X[3:] = s["pairs"]["Xw1"][j], s["pairs"]["Xw2"][j]
            j += 1
        b += struct.pack("<5i", *m) + X.tobytes()
    matched = np.array([drop.get(i, -1) != 0 for i in range(N)])               # vpMatches1[i] != NULL on entry
    return s, b, np.array(kept), matched


def _run(tmp_path, problems):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(struct.pack("<i", len(problems)))
        for p in problems:
            f.write(p[1])
    r = subprocess.run([EXE, pin, pout], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(pout):
        return r, None
    raw, off, out = open(pout, "rb").read(), 0, []
    for _ in problems:
        n, = struct.unpack("<i", raw[off:off + 4]); off += 4
        pairs = np.frombuffer(raw[off:off + 48 * n], _lib.OPTSIM3_PAIR_DTYPE); off += 48 * n
        index = np.frombuffer(raw[off:off + 4 * n], np.int32); off += 4 * n
        ret, written = struct.unpack("<ii", raw[off:off + 8]); off += 8
        sRt = np.frombuffer(raw[off:off + 52], np.float32); off += 52
        N, = struct.unpack("<i", raw[off:off + 4]); off += 4
        left = np.frombuffer(raw[off:off + N], np.uint8).astype(bool); off += N
        out.append(dict(pairs=pairs, index=index, ret=ret, written=written, sRt=sRt, left=left))
    assert off == len(raw)
    return r, out


def _expected(problem):
    """what the reference would leave behind, from the reading: return value, g2oS12 written?, its 13 floats, vpMatches1 != NULL"""
    s, _, kept, matched = problem
    ref = Q.run_case(s)
    left = matched.copy()
    left[kept[ref["bad"].astype(bool)]] = False
    written = ref["n_pairs"] - ref["n_bad"] >= 10
    return ref["n_inliers"], int(written), ref["sRt"] if written else s["sRt_in"], left


def write_fixture():
    d = {}
    for k, name in enumerate(NAMES):
        ret, written, sRt, left = _expected(_problem(name, 30 + k))
        d[name + ".ret"], d[name + ".written"], d[name + ".sRt"], d[name + ".left"] = np.int32(ret), np.int32(written), sRt, left
    np.savez(FIXTURE, **d)


def test_optsim3_dropin_marshals_what_the_reference_reads_and_fails_loudly_without_device(tmp_path):
    _build()
    n = C.c_int(0)
    gpu = _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    problems = [_problem(name, 30 + k) for k, name in enumerate(NAMES)]
    r, out = _run(tmp_path, problems)
    assert r.returncode == 0 and out is not None, r.stderr
    gold = np.load(FIXTURE)
    for (s, _, kept, matched), o, name in zip(problems, out, NAMES):
        # the filters, the i2 lookup and octave -> sigma: the adapter hands the library exactly the scene's records, in slot order
        assert np.array_equal(o["index"], kept) and o["pairs"].tobytes() == s["pairs"].tobytes(), name
        # the fixture is what the reading computes now, and the entries it nulls are matched slots that passed the filters
        ret, written, sRt, left = _expected((s, None, kept, matched))
        assert (ret, written) == (int(gold[name + ".ret"]), int(gold[name + ".written"])) and np.array_equal(left, gold[name + ".left"])
        assert sRt.tobytes() == gold[name + ".sRt"].tobytes()
        assert not (matched & ~left)[np.setdiff1d(np.arange(len(left)), kept)].any()
        if not gpu:   # logged, never thrown: return 0, vpMatches1 and g2oS12 as they were
            assert o["ret"] == 0 and o["written"] == 0 and np.array_equal(o["left"], matched), name
            assert o["sRt"].tobytes() == s["sRt_in"].tobytes()
    if not gpu:
        assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_optsim3_dropin_writes_what_the_reference_writes(tmp_path):
    _build()
    problems = [_problem(name, 30 + k) for k, name in enumerate(NAMES)]
    r, out = _run(tmp_path, problems)
    assert r.returncode == 0 and out is not None, r.stdout + r.stderr
    gold = np.load(FIXTURE)
    for (s, _, kept, matched), o, name in zip(problems, out, NAMES):
        want = gold[name + ".sRt"]
        d = np.abs(o["sRt"].astype(np.float64) - want.astype(np.float64)) / Q.tolerance(want)
        print(f"dropin {name}: return {o['ret']}/{int(gold[name + '.ret'])}, written {o['written']}/{int(gold[name + '.written'])}, "
              f"max diff / tolerance {d.max():.3f}, matches left {int(o['left'].sum())}/{int(gold[name + '.left'].sum())}")
        assert o["ret"] == int(gold[name + ".ret"]) and o["written"] == int(gold[name + ".written"]), name
        assert np.array_equal(o["left"], gold[name + ".left"]), name
        if o["written"]:
            assert np.all(d <= 1.0), (name, d)
        else:   # return 0 by the fewer-than-10 rule: g2oS12 untouched, the bad matches nulled all the same
            assert o["sRt"].tobytes() == s["sRt_in"].tobytes() and o["left"].sum() < matched.sum(), name
