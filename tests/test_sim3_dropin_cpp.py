"""csrc/host/Sim3Solver_hip.h -- orbfe_host::Sim3Solver, the class with the public surface of ORB_SLAM2::Sim3Solver -- on the mock
KeyFrame / MapPoint of tests/cpp_sim3: builds everywhere and fails loudly without a device; on the GPU find() and a round-robin of
iterate(5) over three solvers hand back what the Python mirror computes on the triples the adapter drew, vbInliers is indexed by the original match index, and bNoMore arrives on the call that consumes the last iteration."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, sim3
from tests import np_sim3 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_sim3", "_build", "test_sim3_dropin")
MIN_INLIERS, MAX_ITS, SEED = 20, 300, 1234


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_sim3")], check=True, capture_output=True)


def _problem(name, seed):
    """A case scene spread over N1 = n + 24 match slots: every fourth of the first 96 slots is a match the constructor filters out
    (no match, no map point in keyframe 1, a bad point on either side, a point without an index in its keyframe).  Returns the scene,
    the bytes of the solver's input and mvnIndices1."""
    s = S.case_scene(name)
    n = len(s["pairs"])
    N1 = n + 24
    rng = np.random.default_rng(seed)
    drop = {int(i): k % 6 for k, i in enumerate(range(1, 96, 4))}
    sf = np.ones(s["n_levels"], np.float32)
    for i in range(1, len(sf)):
        sf[i] = sf[i - 1] * np.float32(1.2)
    sigma2 = sf * sf
    kept = [i for i in range(N1) if i not in drop]
    assert len(kept) == n
    perm1, perm2 = rng.permutation(N1), rng.permutation(N1)                  # keypoint index of slot i in either keyframe
    oct1, oct2 = np.zeros(N1, np.int32), np.zeros(N1, np.int32)
    oct1[perm1[kept]], oct2[perm2[kept]] = s["oct1"], s["oct2"]
    b = struct.pack("<i", int(s["fix_scale"]))
    for v, octv in ((s["view1"], oct1), (s["view2"], oct2)):
        b += np.ascontiguousarray(v, _lib.SIM3_VIEW_DTYPE).tobytes() + struct.pack("<i", N1) + octv.tobytes()
        b += struct.pack("<i", len(sigma2)) + sigma2.tobytes()
    b += struct.pack("<i", N1)
    j = 0
    for i in range(N1):
        m = [1, 1, 0, 0, int(perm1[i]), int(perm2[i])]
        X = np.zeros(6, np.float32)
        if i in drop:
            X[:] = 7.0
            kind = drop[i]
            if kind == 0: m[0] = 0
            elif kind == 1: m[1] = 0
            elif kind == 2: m[2] = 1
            elif kind == 3: m[3] = 1
            elif kind == 4: m[4] = -1
            else: m[5] = -1
        else:
            X[:3], X[3:] = s["pairs"]["Xw1"][j], s["pairs"]["Xw2"][j]
            j += 1
        b += struct.pack("<6i", *m) + X.tobytes()
    return s, b, np.array(kept)


def _run(tmp_path, problems, mode):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(struct.pack("<iiIii", len(problems), mode, SEED, MIN_INLIERS, MAX_ITS))
        for _, b, _ in problems:
            f.write(b)
    r = subprocess.run([EXE, pin, pout], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(pout):
        return r, None, None
    raw = open(pout, "rb").read()
    off, calls, tails = 0, [], []
    while off < len(raw):
        k, = struct.unpack("<i", raw[off:off + 4])
        if k >= 0:
            got, = struct.unpack("<i", raw[off + 4:off + 8])
            T = np.frombuffer(raw[off + 8:off + 72], np.float32).reshape(4, 4)
            n_inl, no_more, N1 = struct.unpack("<iii", raw[off + 72:off + 84])
            vb = np.frombuffer(raw[off + 84:off + 84 + N1], np.uint8).astype(bool)
            calls.append((k, got, T, n_inl, no_more, vb))
            off += 84 + N1
        else:
            N, its, status = struct.unpack("<iii", raw[off + 4:off + 16])
            v = np.frombuffer(raw[off + 16:off + 68], np.float32)
            nt, = struct.unpack("<i", raw[off + 68:off + 72])
            tr = np.frombuffer(raw[off + 72:off + 72 + nt * 12], np.int32).reshape(nt, 3)
            tails.append((N, its, status, v, tr))
            off += 72 + nt * 12
    return r, calls, tails


def test_sim3_dropin_builds_and_fails_loudly_without_device(tmp_path):
    _build()
    n = C.c_int(0)
    gpu = _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    problems = [_problem("fixed_stereo", 1)]
    r, calls, tails = _run(tmp_path, problems, 1)
    assert r.returncode == 0 and calls is not None, r.stderr
    assert tails[0][0] == 130 and tails[0][1] == sim3.ransac_iterations(130, 0.99, MIN_INLIERS, MAX_ITS)
    if not gpu:      # logged, never thrown: no matrix, bNoMore at once
        assert "no CPU fallback" in r.stderr and tails[0][2] == _lib.ERR_NO_DEVICE
        assert len(calls) == 1 and calls[0][1] == 0 and calls[0][4] == 1 and not calls[0][5].any() and len(calls[0][5]) == 154


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_sim3_dropin_agrees_with_the_python_mirror(tmp_path, mode):
    _build()
    names = ("mostly_outliers", "free_scale", "fixed_stereo") if mode else ("fixed_stereo", "mostly_outliers", "free_scale")
    problems = [_problem(nm, 10 + i) for i, nm in enumerate(names)]
    r, calls, tails = _run(tmp_path, problems, mode)
    assert r.returncode == 0 and calls is not None, r.stdout + r.stderr
    # the mirror runs on the triples the adapter drew and reports: rand() is process-wide state that any library may advance, so its
    # stream is not replayed here; the draws are checked for what the sampling of :159-172 guarantees
    first = []
    for c in calls:
        if c[0] not in first:
            first.append(c[0])
    expect = {}
    for k in first:
        s, _, kept = problems[k]
        its = sim3.ransac_iterations(len(s["pairs"]), 0.99, MIN_INLIERS, MAX_ITS)
        tr = tails[k][4]
        assert tr.shape == (its, 3) and tr.min() >= 0 and tr.max() < 130
        assert (tr[:, 0] != tr[:, 1]).all() and (tr[:, 0] != tr[:, 2]).all() and (tr[:, 1] != tr[:, 2]).all()
        assert len(np.unique(tr, axis=0)) > its // 2                          # draws, not one triple repeated
        res, mask, hyps, words = sim3.sim3_solve(s["view1"], s["view2"], s["pairs"], tr, s["fix_scale"], MIN_INLIERS)
        expect[k] = (tr, hyps, words, sim3.iterate_replay(hyps["n_inliers"], MIN_INLIERS, its if mode == 0 else 5), its)
        assert tails[k][0] == 130 and tails[k][1] == its and tails[k][2] == 0
    seen = {k: 0 for k in first}
    last_best = {}
    for k, got, T, n_inl, no_more, vb in calls:
        s, _, kept = problems[k]
        tr, hyps, words, replay, its = expect[k]
        ret, want_inl, want_no_more, consumed = replay[seen[k]]
        seen[k] += 1
        assert got == int(ret >= 0) and n_inl == want_inl and len(vb) == 154
        if mode == 1:
            assert no_more == int(want_no_more)                               # on the call that consumes iteration mRansacMaxIts
        c = hyps["n_inliers"][:consumed]
        last_best[k] = int(len(c) - 1 - np.argmax(c[::-1]))                   # the last maximum of what has been consumed
        if ret >= 0:
            h = hyps[ret]
            want = np.eye(4, dtype=np.float32)
            want[:3, :3], want[:3, 3] = (h["s"] * h["R"]).reshape(3, 3), h["t"]
            assert T.tobytes() == want.tobytes()
            bits = S.words_to_bits(words[ret], 130)
            want_vb = np.zeros(154, bool)
            want_vb[kept[bits]] = True                                        # vbInliers is indexed through mvnIndices1
            assert np.array_equal(vb, want_vb) and vb.sum() == n_inl
            last_best[k] = int(ret)
        else:
            assert not T.any() and not vb.any()
    if mode == 0:
        assert [c[1] for c in calls] == [1, 0, 1]                             # find: fixed_stereo and free_scale return, the outliers do not
    else:
        # round-robin: solver 0 (mostly outliers) never returns and runs dry only if nobody matches first; the loop ends at the
        # first match, as LoopClosing::ComputeSim3's does
        assert calls[-1][1] == 1 and sum(c[1] for c in calls) == 1 and len(calls) >= 2 and calls[0][:2] == (0, 0)
    for k in first:                                                           # the getters: the best of what the cursor has passed
        v, h = tails[k][3], expect[k][1][last_best[k]]
        assert v[0] == h["s"] and np.array_equal(v[1:10], h["R"]) and np.array_equal(v[10:13], h["t"])


@pytest.mark.gpu
def test_sim3_dropin_reports_no_more_on_the_last_iteration(tmp_path):
    _build()
    problems = [_problem("mostly_outliers", 20)]
    r, calls, tails = _run(tmp_path, problems, 1)
    assert r.returncode == 0 and calls is not None, r.stdout + r.stderr
    its = tails[0][1]
    assert its == 300 and len(calls) == 60 and [c[4] for c in calls] == [0] * 59 + [1] and not any(c[1] for c in calls)
