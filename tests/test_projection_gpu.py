"""The ordered projection searches on directed input, device side: every scene of tests/np_projection.py byte for byte against the
instrumented walk (which tests/test_projection_cpu.py holds against the C oracle) through the host entry points, the candidate lists
and the independent arg-min on the window scenes, one device batch of eleven frames per mode, and scenes with their queries reversed."""
import functools

import numpy as np
import pytest

from refactored_orb_slam2_amd.matcher import FrameView, Matcher, ORBmatcher
from tests import np_projection as npj
from tests import np_restatement as nr

pytestmark = pytest.mark.gpu
CASES = [(form, geom) for form in npj.FORMS for geom in npj.GEOMETRIES]


def frame_view(sc):
    return FrameView(sc.keys, sc.desc, 0, sc.w, 0, sc.h, sc.u_right if sc.has_u_right else None)


def device_result(sc, queries=None, check_ori=None):
    q = sc.queries if queries is None else queries
    check = sc.check_ori if check_ori is None else check_ori
    fv = frame_view(sc)
    if sc.form == "points":
        return ORBmatcher(sc.nnratio, False).SearchByProjection(fv, q, sc.blocked0)
    if sc.form == "frame":
        return ORBmatcher(0.9, check).SearchByProjectionFrame(fv, q, sc.blocked0)
    return ORBmatcher(0.9, check).SearchByProjectionKeyFrame(fv, q, npj.ORB_DIST, sc.blocked0)


def same(got, want, what):
    nm, assigned, blocked = got
    wnm, wassigned, wblocked = want[:3]
    bad = np.flatnonzero(np.asarray(assigned) != wassigned)
    assert assigned.tobytes() == wassigned.tobytes(), (what, bad[:8], np.asarray(assigned)[bad[:8]], wassigned[bad[:8]])
    assert blocked.tobytes() == wblocked.tobytes(), (what, np.flatnonzero(np.asarray(blocked) != wblocked)[:8])
    assert nm == wnm, (what, nm, wnm)


@pytest.mark.parametrize("form,geom", CASES)
def test_every_scene_equals_the_walk(form, geom):
    for sc in npj.build_scenes(form, *geom):
        same(device_result(sc), sc.result, sc.name)
        if form != "points":     # the rotation check the other way round
            same(device_result(sc, check_ori=not sc.check_ori), sc.walk(check_ori=not sc.check_ori), sc.name + " check_ori flipped")


@pytest.mark.parametrize("form,geom", [c for c in CASES if c[0] != "keyframe"])
def test_candidate_lists_of_the_window_and_list_length_scenes(form, geom):
    """ProjCandidates with max_cand 64: the count is the walk's n_window, the list GetFeaturesInArea's order after the stereo gate"""
    by_name = {s.name: s for s in npj.build_scenes(form, *geom)}
    for sc in (by_name["windows"], by_name["listlen"]):
        F = sc.ref_frame()
        cand, n = ORBmatcher().ProjCandidates(frame_view(sc), sc.queries, max_cand=64)
        np.testing.assert_array_equal(n, sc.result[4]["n_window"], err_msg=sc.name)
        for i, q in enumerate(sc.queries):
            if not q["valid"]:
                continue
            idx = F.GetFeaturesInArea(q["u"], q["v"], q["radius"], int(q["min_level"]), int(q["max_level"]))
            keep = [j for j in idx if not (sc.has_u_right and sc.u_right[j] > 0 and abs(np.float32(q["u_r"]) - sc.u_right[j]) > q["radius"])][:64]
            assert cand[i, :len(keep)]["idx"].tolist() == keep, (sc.name, i)
            assert cand[i, :len(keep)]["dist"].tolist() == [nr.descriptor_distance(q["desc"], sc.desc[j]) for j in keep], (sc.name, i)


@pytest.mark.parametrize("geom", npj.GEOMETRIES)
def test_independent_best_of_the_tie_and_window_scenes(geom):
    """ProjBest without a gate: the first minimum in GetFeaturesInArea's order, whatever is blocked"""
    by_name = {s.name: s for s in npj.build_scenes("frame", *geom)}
    for sc in (by_name["ties"], by_name["windows"]):
        F = sc.ref_frame()
        bi, bd = ORBmatcher().ProjBest(frame_view(sc), sc.queries)
        for i, q in enumerate(sc.queries):
            want = (-1, 256)
            if q["valid"]:
                for j in F.GetFeaturesInArea(q["u"], q["v"], q["radius"], int(q["min_level"]), int(q["max_level"])):
                    d = nr.descriptor_distance(q["desc"], sc.desc[j])
                    if d < want[1]:
                        want = (j, d)
            assert (bi[i], bd[i]) == want, (sc.name, i)
        if sc.name == "ties":
            f = sc.result[4]
            assert [bi[i] for i in sc.tags["tie_cells"] + sc.tags["tie_cell"]] == [f["best_idx"][i] for i in sc.tags["tie_cells"] + sc.tags["tie_cell"]]


@pytest.mark.parametrize("form", npj.FORMS)
def test_reversed_queries(form):
    """the walk's result changes with the order of the queries, and the kernel follows it"""
    by_name = {s.name: s for s in npj.build_scenes(form)}
    for name in ("chain", "staging", "listlen"):
        sc = by_name[name]
        rq = sc.queries[::-1].copy()
        want = sc.walk(rq)
        back = np.where(want[1] >= 0, len(rq) - 1 - want[1], -1)
        assert not np.array_equal(back, sc.result[1]), name
        same(device_result(sc, rq), want, name + " reversed")


# ---- the device entry point ------------------------------------------------------------------------------------------------------------
N_BATCH, CAP, Q_CAP = 11, 300, 2100       # an XCD group of 8 and a tail of 3; capacities above every n and nq


@functools.lru_cache(maxsize=None)
def matcher():
    return Matcher()


def batch_frames(form):
    by_name = {s.name: s for s in npj.build_scenes(form)}
    names = ["chain", "staging", "listlen", "withdrawn" if form == "points" else "rot_11_1", "windows", "ties", "thresholds",
             "counts_1025", "counts_2049"]
    frames = [(by_name[n], True, True) for n in names]
    frames.insert(3, (by_name["counts_1023"], True, False))     # nq == 0
    frames.insert(9, (by_name["counts_1024"], False, True))     # n == 0
    assert len(frames) == N_BATCH
    return frames


@pytest.mark.parametrize("form", ("points", "frame"))
def test_device_batch_of_eleven_frames(form):
    import torch
    frames = batch_frames(form)
    rng = np.random.default_rng(11)
    kps = rng.integers(0, 256, (N_BATCH, CAP, 28), dtype=np.uint8); desc = rng.integers(0, 256, (N_BATCH, CAP, 32), dtype=np.uint8)
    ur = np.full((N_BATCH, CAP), -1, np.float32)
    q = rng.integers(0, 256, (N_BATCH, Q_CAP, 68), dtype=np.uint8)
    blocked0 = rng.integers(0, 2, (N_BATCH, CAP), dtype=np.uint8)
    n = np.zeros(N_BATCH, np.int32); nq = np.zeros(N_BATCH, np.int32)
    for p, (sc, with_keys, with_queries) in enumerate(frames):
        assert len(sc.keys) < CAP and len(sc.queries) < Q_CAP
        if with_keys:
            n[p] = len(sc.keys)
            kps[p, :n[p]] = sc.keys.view(np.uint8).reshape(-1, 28); desc[p, :n[p]] = sc.desc; ur[p, :n[p]] = sc.u_right
            blocked0[p, :n[p]] = sc.blocked0
        if with_queries:
            nq[p] = len(sc.queries)
            q[p, :nq[p]] = sc.queries.view(np.uint8).reshape(-1, 68)
    dev = lambda a: torch.from_numpy(a).cuda()
    t = [dev(a) for a in (kps, desc, n, ur, q, nq)]
    m = matcher()
    mode, nnratio = (0, frames[0][0].nnratio) if form == "points" else (1, 0.0)
    runs = []
    for _ in range(2):      # twice on one handle with fresh outputs: the claim buffers and the histogram carry nothing over
        blocked = dev(blocked0.copy())
        assigned = torch.full((N_BATCH, CAP), -1, dtype=torch.int32, device="cuda")
        nm = torch.full((N_BATCH,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.proj_match_batch(t[0], t[1], t[2], t[3], (0.0, 640.0, 0.0, 480.0), t[4], t[5], mode, nnratio, True, blocked, assigned, nm)
        m.sync()
        runs.append((nm.cpu().numpy(), assigned.cpu().numpy(), blocked.cpu().numpy()))
    total = 0
    for nm, assigned, blocked in runs:
        for p, (sc, with_keys, with_queries) in enumerate(frames):
            if with_keys and with_queries:
                want = sc.walk(check_ori=True)
                same((nm[p], assigned[p, :n[p]], blocked[p, :n[p]]), want, (p, sc.name))
                total += want[0]
            else:
                assert nm[p] == 0 and np.all(assigned[p] == -1) and np.array_equal(blocked[p], blocked0[p]), (p, sc.name)
            # rows beyond n come back as they went in
            assert np.all(assigned[p, n[p]:] == -1) and np.array_equal(blocked[p, n[p]:], blocked0[p, n[p]:]), (p, sc.name)
    assert total > 2 * 400      # the two chains alone bring 265 matches per run
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
