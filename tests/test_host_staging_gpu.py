"""The staging every one-problem host call shares (HostCall in csrc/host_internal.h): one device block with a pinned mirror per calling
thread, one packed upload, one packed download.  Calls of very different staged sizes in turn on one thread (the block and its mirror
are reallocated in between), the same sequence on two threads at once, and the forms that used to stage array by array on frames of
63, 64 and 65 keypoints -- the smallest shapes at which a wrong offset, a region in the wrong group or a fill that moved can show.
Every result is compared with the oracle or the reading its own suite compares it with."""
import threading

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, mapping, optimizer, synth
from refactored_orb_slam2_amd._lib import LAST_POINT_DTYPE
from refactored_orb_slam2_amd.matcher import FrameView, ORBmatcher, make_frustum, search_by_bow_kf, search_for_triangulation
from tests import np_mapping as M
from tests import np_pose as P
from tests import oracle_lib as ol
from tests.test_mapping_gpu import _oracle_search
from tests.test_matcher_gpu import _check_kf, _frustum_and_map, _queries_from_last, _two_frames
from tests.test_pose_gpu import _camera, _compare, _keys, _records

pytestmark = pytest.mark.gpu

W, H = 640, 480


@pytest.fixture(scope="module")
def frames():
    return _two_frames(W, H, 1000)


@pytest.fixture(scope="module")
def scenes(frames):
    """(a) a projection search that stages under 64 KiB, (b) a neighbour loop that stages several times that, a pose scene"""
    k0, d0, k1, d1, sf = frames
    rng = np.random.default_rng(5)
    k1, d1 = k1[:300], d1[:300]
    ur = np.where(rng.random(300) < 0.5, k1["x"] - np.float32(20.0) + rng.normal(0, 3, 300).astype(np.float32), np.float32(-1)).astype(np.float32)
    q = _queries_from_last(k0[:200], d0[:200], sf, 15.0, rng=rng, blocks_p=0.5)
    blocked0 = (rng.random(300) < 0.05).astype(np.uint8)
    return dict(a=(k1, d1, sf, ur, q, blocked0), b=M.make_chain_scene(seed=41, n=300), pose=P.case_scene("standard"))


def _call_a(sc):
    k1, d1, sf, ur, q, blocked0 = sc["a"]
    return ORBmatcher(0.9, True).SearchByProjectionFrame(FrameView(k1, d1, 0, W, 0, H, ur), q, blocked0)


def _call_b(sc):
    A, nbs = sc["b"]["A"], sc["b"]["neighbors"]
    return mapping.create_new_map_points(A["keys"], A["desc"], A["u_right"], A["depth"], A["has_mp"], A["groups"], A["view"], nbs,
                                         monocular=False, check_orientation=True)


def _call_pose(sc):
    s = sc["pose"]
    return optimizer.pose_optimization(_keys(s), s["u_right"], s["assigned"], _records(s, LAST_POINT_DTYPE), _camera(s), s["Tcw_in"])


def _bytes(result):
    return b"".join(np.asarray(x).tobytes() for x in result)


def _sequence(sc):
    """small, large, small, pose, large on a fresh handle of the calling thread; the results in call order"""
    _lib.lib().orbfe_thread_release()
    return [_call_a(sc), _call_b(sc), _call_a(sc), _call_pose(sc), _call_b(sc)]


@pytest.fixture(scope="module")
def single_thread(scenes):
    return _sequence(scenes)


def test_block_regrowth_and_reuse(scenes, single_thread):
    a, b, a2, pose, b2 = single_thread
    assert _bytes(a2) == _bytes(a) and _bytes(b2) == _bytes(b)
    # (a) against the oracle, as test_matcher_gpu.test_search_by_projection_frame
    k1, d1, sf, ur, q, blocked0 = scenes["a"]
    onm, oassigned, oblocked = ol.OracleFrame(k1, d1, sf, 0, W, 0, H, ur).search_by_projection_frame(q, True, blocked0)
    assert a[0] == onm and onm > 30
    np.testing.assert_array_equal(a[1], oassigned)
    np.testing.assert_array_equal(a[2], oblocked)
    # (b) against the replay, as test_mapping_gpu.test_neighbour_loop_against_the_replay
    pts, n_matches, n_new, has = b
    want, w_matches, w_new, w_has, adopted, searched = M.replay_chain(scenes["b"], _oracle_search, device_points=pts)
    assert adopted <= M.NON_PARITY_CAP * 300 * 3
    assert np.array_equal(n_matches, w_matches) and n_matches[0] > 50 and np.array_equal(n_new, w_new) and n_new[0] >= 20
    for k in range(3):
        assert np.array_equal(pts[k]["idx2"], searched[k]), k
        for f in ("code", "path", "idx2"):
            assert np.array_equal(pts[k][f], want[k][f]), (k, f)
    assert np.array_equal(has, w_has)
    # the pose against its reading, as test_pose_gpu.test_host_form_against_the_reading
    _compare("standard", pose[0], pose[1], P.run_case(scenes["pose"]))


def test_two_threads_each_with_its_own_handle(scenes, single_thread):
    got, errors = [None, None], []

    def work(i):
        try:
            got[i] = _sequence(scenes)
        except Exception as e:   # noqa: BLE001 -- reported by the assertion below
            errors.append(e)
        finally:
            _lib.lib().orbfe_thread_release()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for j, (r, w) in enumerate(zip(got[i], single_thread)):
            assert _bytes(r) == _bytes(w), (i, j)


def _kf_scene(k, d, ur, seed):
    """test_matcher_gpu._kf_scene on a given keyframe: a camera looking at it and candidate map points on its keypoints"""
    rng = np.random.default_rng(seed)
    R, t = synth.camera_pose(seed)
    fr = make_frustum(R, t, 517.3, 516.5, 318.6, 255.3, 40.0, (0, W, 0, H), 1.2, 8)
    mp = synth.local_map(k, d, fr, seed + 1, n_extra=30)
    cam = np.zeros(1, _lib.KF_CAMERA_DTYPE)
    for f in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y", "log_scale_factor", "n_levels"):
        cam[f] = fr[f]
    cam["R"] = fr["Rcw"]; cam["t"] = fr["tcw"]; cam["Ow"] = fr["Ow"]; cam["scale_factors"] = fr["scale_factors"]
    pts = np.zeros(len(mp), _lib.KF_POINT_DTYPE)
    for f in ("pos", "normal", "min_distance", "max_distance", "skip", "desc"):
        pts[f] = mp[f]
    pts["angle"] = rng.uniform(0, 360, len(pts)).astype(np.float32)
    return cam, pts


@pytest.mark.parametrize("n", [63, 64, 65])
def test_packed_forms_at_a_wave_boundary(frames, n):
    """Frames of n keypoints: at 63 and 65 the byte-sized regions (valid flags, blocked flags) end off a 4-byte boundary in front of an
    int32 region.  Queries number n + 1, so that the two counts differ."""
    k0, d0, k1, d1, sf = frames
    rng = np.random.default_rng(n)
    kA, dA, kB, dB = k0[:n + 1], d0[:n + 1], k1[:n], d1[:n].copy()
    near = min(n, 40)                       # planted near-duplicates, so that every search has matches to report
    dB[:near] = dA[:near]
    for t in range(near):
        for f in rng.integers(0, 256, 5):
            dB[t, f // 8] ^= np.uint8(1 << (f % 8))
    kB = kB.copy()
    kB["x"][:near] = kA["x"][:near] + np.float32(2.0); kB["y"][:near] = kA["y"][:near]
    kB["octave"][:near] = kA["octave"][:near]; kB["angle"][:near] = kA["angle"][:near]
    ur = np.where(rng.random(n) < 0.5, kB["x"] - np.float32(20.0) + rng.normal(0, 1, n).astype(np.float32), np.float32(-1)).astype(np.float32)
    fv, of = FrameView(kB, dB, 0, W, 0, H, ur), ol.OracleFrame(kB, dB, sf, 0, W, 0, H, ur)
    fvm, ofm = FrameView(kB, dB, 0, W, 0, H), ol.OracleFrame(kB, dB, sf, 0, W, 0, H)
    m = ORBmatcher(0.9, True)

    # SearchByBoW / SearchByBoW(KF, KF): a proper FeatureVector (parallel) and one with features under two nodes (sequential)
    par_a = {7: list(range(near)), **{100 + g: [i for i in range(near, n + 1) if dA[i, 1] % 6 == g] for g in range(6)}}
    par_b = {7: list(range(near)), **{100 + g: [i for i in range(near, n) if dB[i, 1] % 6 == g] for g in range(6)}}
    par_a, par_b = {g: v for g, v in par_a.items() if v}, {g: v for g, v in par_b.items() if v}
    seq_a, seq_b = {**par_a, 300: list(range(5))}, {**par_b, 300: list(range(5))}
    validA, validB = (rng.random(n + 1) < 0.9).astype(np.uint8), (rng.random(n) < 0.85).astype(np.uint8)
    for ga, gb in ((par_a, par_b), (seq_a, seq_b)):
        for check in (True, False):
            nm, mB = ORBmatcher(0.9, check).SearchByBoW(dA, kA["angle"], validA, ga, dB, kB["angle"], gb)
            onm, omB = ol.search_by_bow(dA, kA["angle"], validA, ga, dB, kB["angle"], gb, np.float32(0.9), check)
            assert nm == onm and onm > 10
            np.testing.assert_array_equal(mB, omB)
            nm, mA = search_by_bow_kf(dA, kA["angle"], validA, ga, dB, kB["angle"], validB, gb, 0.9, check)
            onm, omA = ol.search_by_bow_kf(dA, kA["angle"], validA, ga, dB, kB["angle"], validB, gb, np.float32(0.9), check)
            assert nm == onm and onm > 10
            np.testing.assert_array_equal(mA, omA)

    # SearchForTriangulation: the scene of test_matcher_gpu.test_search_for_triangulation
    ep = np.zeros(1, ol.EPIPOLAR_DTYPE)
    ep["F12"][0] = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32) * np.float32(0.37)
    ep["ex"] = 9000.0; ep["ey"] = 240.0
    ep["scale_factors"][0, :len(sf)] = sf
    ep["level_sigma2"][0, :len(sf)] = (sf * sf).astype(np.float32)
    urA = np.where(rng.random(n + 1) < 0.5, kA["x"] - np.float32(20), -1).astype(np.float32)
    hasA, hasB = (rng.random(n + 1) < 0.2).astype(np.uint8), (rng.random(n) < 0.2).astype(np.uint8)
    for ga, only_stereo, check in ((par_a, False, True), (par_a, True, False), (seq_a, False, True)):
        nm, mA = search_for_triangulation(kA, dA, urA, hasA, ga, kB, dB, ur, hasB, par_b, ep, only_stereo, check)
        onm, omA = ol.search_for_triangulation(kA, dA, urA, hasA, ga, kB, dB, ur, hasB, par_b, ep, only_stereo, check)
        assert nm == onm and (only_stereo or onm > 5)
        np.testing.assert_array_equal(mA, omA)

    # the candidate lists and the independent arg-min searches
    q = _queries_from_last(kA, dA, sf, 7.5, shift=(2.0, 0.0), rng=rng)
    q["max_level"] = kA["octave"]
    inv_sigma2 = (np.float32(1) / (sf * sf)).astype(np.float32)
    cand, cnt = m.ProjCandidates(fv, q, max_cand=32)
    for i in range(len(q)):
        idx = of.features_in_area(float(q["u"][i]), float(q["v"][i]), float(q["radius"][i]), int(q["min_level"][i]), int(q["max_level"][i]))
        keep = [j for j in idx if not (ur[j] > 0 and abs(np.float32(q["u_r"][i]) - ur[j]) > q["radius"][i])] if q["valid"][i] else []
        assert cnt[i] == len(keep), i
        np.testing.assert_array_equal(cand[i, :cnt[i]]["idx"], np.asarray(keep, np.int32), err_msg=f"query {i}")
        for c in range(cnt[i]):
            assert cand[i, c]["dist"] == ol.descriptor_distance(q["desc"][i], dB[keep[c]])
    assert cnt.sum() > 10
    for view, oview, inv in ((fv, of, inv_sigma2), (fv, of, None), (fvm, ofm, inv_sigma2)):
        bi, bd = m.ProjBest(view, q, inv)
        obi, obd = oview.proj_best(q, inv)
        np.testing.assert_array_equal(bi, obi); np.testing.assert_array_equal(bd, obd)
    assert (obi >= 0).sum() > 10

    # Tracking::SearchLocalPoints
    fr, mp = _frustum_and_map(kB, dB, W, H, 77, n_extra=30)
    blocked0 = (rng.random(n) < 0.1).astype(np.uint8)
    ntm, nm, track, assigned, blocked = ORBmatcher(0.8).SearchLocalPoints(fv, fr, mp, 3.0, blocked0)
    ontm, onm, otrack, oassigned, oblocked = of.search_local_points(fr, mp, np.float32(3.0), np.float32(0.8), blocked0)
    assert track.tobytes() == otrack.tobytes() and ntm == ontm > 10 and nm == onm > 5
    np.testing.assert_array_equal(assigned, oassigned)
    np.testing.assert_array_equal(blocked, oblocked)

    # orbfe_kf_search: Fuse (independent searches), SearchByProjection(KF, Scw) and the relocalisation search (sequential)
    cam, pts = _kf_scene(kB, dB, ur, 41 + n)
    cam["th"] = 3.0
    nk, res, _ = ORBmatcher(0.8, True).KeyFrameSearch(fv, cam, pts, _lib.KF_FUSE, inv_level_sigma2=inv_sigma2)
    on, ores, _ = ol.kf_search(of, cam, pts, 1, inv_level_sigma2=inv_sigma2)
    _check_kf(res, ores); assert nk == on and on > 10
    cam["th"] = 10.0
    matched0 = (rng.random(n) < 0.15).astype(np.uint8)
    nk, res, blk = ORBmatcher(0.8, True).KeyFrameSearch(fv, cam, pts, _lib.KF_LOOP, blocked=matched0, max_dist=50)
    on, ores, oblk = ol.kf_search(of, cam, pts, 4, matched=matched0, th_low=50)
    _check_kf(res, ores, ("best_idx", "level", "u", "v")); assert nk == on and on > 10
    np.testing.assert_array_equal(blk, oblk)
    nk, res, blk = ORBmatcher(0.9, True).KeyFrameSearch(fvm, cam, pts, _lib.KF_RELOC, blocked=matched0, max_dist=100)
    on, ores, _ = ol.kf_search(ofm, cam, pts, 5, matched=matched0, th_low=100, check_orientation=True)
    _check_kf(res, ores, ("best_idx",)); assert nk == on and on > 5

    # SearchForInitialization: F1 has n + 1 keypoints, F2 n
    prev = np.stack([kA["x"], kA["y"]], axis=1).astype(np.float32)
    f1 = FrameView(kA, dA, 0, W, 0, H)
    for check in (True, False):
        nm, m12, p2 = ORBmatcher(0.9, check).SearchForInitialization(f1, fvm, prev, 30)
        onm, om12, op2 = ol.search_for_initialization(kA, dA, ofm, prev, 30, np.float32(0.9), check)
        assert nm == onm and onm > 5
        np.testing.assert_array_equal(m12, om12)
        np.testing.assert_array_equal(p2, op2)
