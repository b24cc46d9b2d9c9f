"""csrc/host/PnPsolver_hip.h -- orbfe_host::PnPsolver, the class with the public surface of ORB_SLAM2::PnPsolver -- on the mock Frame /
MapPoint of tests/cpp_pnp: builds everywhere and fails loudly without a device; on the GPU the loop shape of Tracking::Relocalization
(SolveAll, then iterate(5) round robin over three candidates) hands back what iterate_replay computes over the records of the sets the
adapter drew: returned poses, vbInliers by keypoint index, nInliers and bNoMore."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, pnp
from tests import np_pnp as Y
from tests import pnp_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_pnp", "_build", "test_pnp_dropin")
SEED, TH2 = 4321, np.float32(5.991)
SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2            # the level table of the scenes (np_pnp._scene_points)


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_pnp")], check=True, capture_output=True)


def _candidate(name, seed):
    """A case spread over n + min(12, n) keypoint slots: the first odd slots have no map point or a bad one.  Returns the case, the
    bytes of the candidate and the kept slots (mvKeyPointIndices)."""
    c = pnp_host.case(name)
    p = c["points"]
    n = len(p)
    slots = n + min(12, n)
    drop = {i: k % 2 for k, i in enumerate(range(1, 2 * (slots - n), 2))}
    kept = [i for i in range(slots) if i not in drop]
    assert len(kept) == n
    octave = np.array([int(np.flatnonzero(SIGMA2 * TH2 == e)[0]) for e in p["max_err"]], np.int32)
    b = struct.pack("<f4fi", float(np.float32(c["params"]["epsilon"])), *(c["cam"][k] for k in ("fx", "fy", "cx", "cy")), len(SIGMA2))
    b += SIGMA2.tobytes() + struct.pack("<i", slots)
    rng = np.random.default_rng(seed)
    j = 0
    for i in range(slots):
        if i in drop:
            b += struct.pack("<3i5f", drop[i], 1, int(rng.integers(8)), *rng.normal(0, 5, 5).astype(np.float32).tolist())
        else:
            b += struct.pack("<3i", 1, 0, int(octave[j])) + p["Xw"][j].tobytes() + p["u"][j].tobytes() + p["v"][j].tobytes()
            j += 1
    return c, b, np.array(kept)


def _run(tmp_path, cands):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(struct.pack("<iI", len(cands), SEED))
        for _, b, _ in cands:
            f.write(b)
    r = subprocess.run([EXE, pin, pout], capture_output=True, text=True, timeout=120)
    if r.returncode != 0 or not os.path.exists(pout):
        return r, None, None
    raw = open(pout, "rb").read()
    off, calls, tails = 0, [], []
    while off < len(raw):
        k, = struct.unpack("<i", raw[off:off + 4])
        if k >= 0:
            got, = struct.unpack("<i", raw[off + 4:off + 8])
            T = np.frombuffer(raw[off + 8:off + 72], np.float32).reshape(4, 4)
            n_inl, no_more, slots = struct.unpack("<iii", raw[off + 72:off + 84])
            calls.append((k, got, T, n_inl, no_more, np.frombuffer(raw[off + 84:off + 84 + slots], np.uint8).astype(bool)))
            off += 84 + slots
        else:
            N, mi, its, status, consumed, ns = struct.unpack("<6i", raw[off + 4:off + 28])
            sets = np.frombuffer(raw[off + 28:off + 28 + ns * 16], np.int32).reshape(ns, 4)
            pts = np.frombuffer(raw[off + 28 + ns * 16:off + 28 + ns * 16 + N * 24], _lib.PNP_POINT_DTYPE)
            tails.append(dict(N=N, min_inliers=mi, its=its, status=status, consumed=consumed, sets=sets, points=pts))
            off += 28 + ns * 16 + N * 24
    return r, calls, tails


NAMES = ("second_best_refines", "best_at_exhaustion", "kitti")


def test_pnp_dropin_builds_and_fails_loudly_without_device(tmp_path):
    _build()
    n = C.c_int(0)
    gpu = _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    cands = [_candidate("kitti", 1), _candidate("too_few", 2)]
    r, calls, tails = _run(tmp_path, cands)
    assert r.returncode == 0 and calls is not None, r.stderr
    # the constructor and SetRansacParameters need no device
    for (c, _, _), t in zip(cands, tails):
        assert t["N"] == len(c["points"]) and (t["min_inliers"], t["its"]) == (c["min_inliers"], c["iterations"])
        assert t["points"].tobytes() == np.ascontiguousarray(c["points"]).tobytes()
    too_few = [x for x in calls if x[0] == 1]
    assert len(too_few) == 1 and too_few[0][1] == 0 and too_few[0][4] == 1 and len(tails[1]["sets"]) == 0      # N < nMinInliers: bNoMore at once
    if not gpu:      # logged, never thrown: no matrix, bNoMore at once
        assert "no CPU fallback" in r.stderr and tails[0]["status"] == _lib.ERR_NO_DEVICE
        first = [x for x in calls if x[0] == 0]
        assert len(first) == 1 and first[0][1] == 0 and first[0][4] == 1 and not first[0][5].any()


@pytest.mark.gpu
def test_pnp_dropin_agrees_with_iterate_replay(tmp_path):
    _build()
    cands = [_candidate(nm, 10 + i) for i, nm in enumerate(NAMES)]
    r, calls, tails = _run(tmp_path, cands)
    assert r.returncode == 0 and calls is not None, r.stdout + r.stderr
    seen = [0] * len(cands)
    replays, sols = [], []
    for (c, _, kept), t in zip(cands, tails):
        n, sets = t["N"], t["sets"]
        assert t["status"] == 0 and t["points"].tobytes() == np.ascontiguousarray(c["points"]).tobytes()
        assert (t["min_inliers"], t["its"]) == (c["min_inliers"], c["iterations"]) and len(sets) >= t["its"] + 5
        assert sets.min() >= 0 and sets.max() < n and all(len(set(row)) == 4 for row in sets.tolist())     # draws of :184-197
        assert len(np.unique(sets, axis=0)) > len(sets) // 2
        sol = pnp.pnp_solve(pnp_host.camera(c["cam"]), t["points"], sets, t["min_inliers"], want_diag=False)
        sols.append(sol)
        replays.append(pnp.iterate_replay(sol.hyps, sol.refines, t["min_inliers"], 5, t["its"]))
    for k, got, T, n_inl, no_more, vb in calls:
        c, _, kept = cands[k]
        sol, call = sols[k], replays[k][seen[k]]
        seen[k] += 1
        n, slots = tails[k]["N"], tails[k]["N"] + min(12, tails[k]["N"])
        assert len(vb) == slots and no_more == int(call.no_more) and n_inl == call.n_inliers and got == int(call.returned >= 0)
        if call.returned < 0:
            assert not T.any() and not vb.any()
            continue
        rec = sol.refines[call.refine] if call.refine >= 0 else sol.hyps[call.returned]
        bits = Y.unpack_bits((sol.refine_words[call.refine] if call.refine >= 0 else sol.words[call.returned]), n)
        want = np.eye(4, dtype=np.float32)
        want[:3, :3], want[:3, 3] = rec["R"].reshape(3, 3).astype(np.float32), rec["t"].astype(np.float32)
        assert T.tobytes() == want.tobytes()
        want_vb = np.zeros(slots, bool)
        want_vb[kept[bits]] = True                                            # vbInliers is indexed through mvKeyPointIndices
        assert np.array_equal(vb, want_vb) and vb.sum() == n_inl
    for k, t in enumerate(tails):
        assert seen[k] == len(replays[k]) and t["consumed"] == replays[k][-1].consumed
    # what the cases are for: somebody returns a refined pose before running dry; the ten exact inliers of the second never refine
    assert any(c.refine >= 0 and not c.no_more for rp in replays for c in rp)
    assert all(c.refine < 0 for c in replays[1]) and replays[1][-1].no_more
