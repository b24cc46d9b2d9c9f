"""CPU suite of the keyframe decision and the close stereo points (orbfe_keyframe_insertion*): the yardstick tests/np_keyframe.py against
itself -- the literal loop of Tracking.cc:992-1022 against the closed form on every scene it builds, the decision of :880-961 against a
truth table written a second time here -- and what the library decides before any device call: every limit one step inside and one
step past, null arrays, alignment, flags, struct sizes."""
import ctypes as C
import itertools

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, tracking
from tests import np_keyframe as M


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.fixture(scope="module")
def cases():
    return M.directed_cases()


def _all_frames(cases):
    for name, (problem, *_) in cases.items():
        for fr in problem["frames"]:
            yield name, problem, fr
    seeded = M.seeded_problem(S=6)
    for fr in seeded["frames"]:
        yield "seeded", seeded, fr


def test_literal_loop_equals_closed_form_on_every_scene(cases):
    seen = set()
    for name, problem, fr in _all_frames(cases):
        n, th = fr["n"], problem["scales"]["th_depth"][0]
        visited = M.selection_literal(fr["depth"][:n], th)
        order, Mc, c, Lp = M.selection_closed_form(fr["depth"][:n], th)
        assert visited == list(order[:Lp]), name
        assert Lp == min(Mc, max(100, c) + 1)
        seen.add((Mc <= 100, c < 100, c == 100, c > 100, Lp == Mc))
    assert len(seen) >= 5   # both sides of every comparison in the closed form occurred


def test_directed_cases_hold_what_their_names_say(cases):
    th = M.TH_DEPTH
    def counts(name):
        fr = cases[name][0]["frames"][0]
        return M.selection_closed_form(fr["depth"][:fr["n"]], th), fr
    for Mx, Lx in ((0, 0), (1, 1), (100, 100), (101, 101), (102, 101)):
        (order, Mc, c, Lp), _ = counts(f"M{Mx}_all_far")
        assert (Mc, c, Lp) == (Mx, 0, Lx)
    for cx in (99, 100, 101):
        (order, Mc, c, Lp), _ = counts(f"c{cx}_far_behind")
        assert c == cx and Mc == cx + 20 and Lp == max(100, cx) + 1
    for before in (100, 101):
        (order, Mc, c, Lp), fr = counts(f"at_th_position_{before}")
        assert fr["depth"][order[before]] == th and c == before + 1 and Lp == before + 2   # the loop went on past it
        t, nt = M.close_counts_literal(fr, fr["decision"], th)
        assert t + nt == before                                                             # and the close counts exclude it
    (order, Mc, c, Lp), fr = counts("forty_equal_across_boundary")
    tie = np.flatnonzero(fr["depth"][:fr["n"]] == np.float32(55.0))
    assert len(tie) == 40 and c == 80 and Lp == 101 and list(order[80:101]) == sorted(tie)[:21]
    (order, Mc, c, Lp), fr = counts("zero_negative_nan_inf")
    d = fr["depth"][order]
    assert np.isinf(d[-1]) and np.isinf(d[-2]) and not np.isnan(d).any() and (d > 0).all() and Mc == 34 and d[0] == np.float32(5e-39)
    for name, (problem, mode, flags, new_cap, opt) in cases.items():
        R = M.frame_reading(problem, problem["frames"][0], flags, mode, opt.get("with_outlier", True), opt.get("with_assigned", True))
        assert R["refused"] == name.startswith("refused_"), name
        assert not M.frame_reading(problem, problem["frames"][1], flags, mode)["refused"]
        if name in ("all_observed",):
            assert R["header"]["n_created"] == 0 and R["header"]["L"] > 100
        if name == "temporal_keyframe":
            assert R["header"]["n_cleared"] > 5 and R["header"]["n_created"] > R["header"]["n_cleared"]
        if name == "temporal_last_frame":
            assert R["header"]["n_cleared"] == 0 and R["header"]["n_created"] > 5
        if name in ("need_zero_nothing_created", "n_zero"):
            assert R["header"]["need"] == 0 and not R["ran"]
        elif flags & M.DECISION and not R["refused"] and name.startswith(("M", "c", "at_th", "forty", "zero_", "temporal", "overflow", "octave")):
            assert R["header"]["need"] == 1, name
        if name.startswith("stereo_init"):
            assert R["ran"] == name.endswith("501")
    a = M.frame_reading(*[cases["ref_mixed_min_obs_3"][0]] + [cases["ref_mixed_min_obs_3"][0]["frames"][0], M.ALL, M.KEYFRAME])["header"]
    b = M.frame_reading(*[cases["ref_mixed_min_obs_2"][0]] + [cases["ref_mixed_min_obs_2"][0]["frames"][0], M.ALL, M.KEYFRAME])["header"]
    assert 0 < a["n_ref_matches"] < b["n_ref_matches"]


def _truth(sensor, only_tracking, stopped, idle, queue, n_kfs, c1a, c1b_frames, weak25, weak_ratio, close, enough):
    """the second writing of :880-961: from the truth values of its atoms to (early, conditions, need, interrupt_ba)"""
    if only_tracking:
        return 1, 0, 0, 0
    if stopped:
        return 2, 0, 0, 0
    mono = sensor == M.MONOCULAR
    c1b = c1b_frames and idle
    c1c = (not mono) and (weak25 or close)
    c2 = (weak_ratio or close) and enough
    cond = c1a * 1 + c1b * 2 + c1c * 4 + c2 * 8
    if not ((c1a or c1b or c1c) and c2):
        return 0, cond, 0, 0
    if idle:
        return 0, cond, 1, 0
    return 0, cond, int((not mono) and queue < 3), 1


def test_decision_against_an_independent_truth_table():
    reached, branches = set(), set()
    for sensor, only_tracking, stopped, idle, queue, n_kfs in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1), (2, 3), (1, 2, 3)):
        for last_kf, min_frames, inl, n_ref, tracked, non_tracked in itertools.product((50, 90, 99), (0, 5), (10, 16, 40, 140), (0, 100, 200),
                                                                                    (50, 100), (70, 71)):
            D = M.default_decision(sensor=sensor, only_tracking=only_tracking, mapper_stopped=stopped, accept_keyframes=idle,
                                   keyframes_in_queue=queue, n_kfs=n_kfs, last_keyframe_id=last_kf, min_frames=min_frames, frame_id=100)
            got = M.decide_literal(D, inl, tracked, non_tracked, n_ref)
            ratio = 0.9 if sensor == 0 else 0.4 if n_kfs < 2 else 0.75   # exact in these products: the integers are small
            close = tracked < 100 and non_tracked > 70
            want = _truth(sensor, only_tracking, stopped, idle, queue, n_kfs, 100 >= last_kf + 30, 100 >= last_kf + min_frames,
                          4 * inl < n_ref, np.float32(inl) < np.float32(n_ref) * np.float32(ratio), close, inl > 15)
            assert got == want, (D, inl, tracked, non_tracked, n_ref)
            if got[0] == 0:
                reached.add(got[1])
                branches.add((sensor, idle, queue, n_kfs, got[2], got[3]))
            else:
                branches.add(("early", got[0], sensor))
    # c1c implies nothing about the others only for a non-monocular sensor; every combination of the four bits must have occurred
    assert reached == set(range(16))
    for sensor in (0, 1, 2):
        assert ("early", 1, sensor) in branches and ("early", 2, sensor) in branches
        for queue, n_kfs in itertools.product((2, 3), (1, 2, 3)):
            assert (sensor, 1, queue, n_kfs, 1, 0) in branches                       # idle: inserted
            assert (sensor, 0, queue, n_kfs, int(sensor != 0 and queue < 3), 1) in branches   # not idle: BA interrupted, the queue decides


def test_decision_types_of_the_source():
    # the relocalisation guard: unsigned 32-bit sums that wrap, against a 64-bit frame id
    D = M.default_decision(frame_id=5, last_reloc_frame_id=0xFFFFFFF0, max_frames=30, n_kfs=31)
    assert (0xFFFFFFF0 + 30) & 0xFFFFFFFF == 14 and M.decide_literal(D, 40, 0, 0, 100)[0] == 3 and M.statistics_literal(
        {"n": 0, "assigned": [], "outlier": [], "points": None}, D) == (0, 0)
    D = M.default_decision(frame_id=2 ** 32 + 5, last_reloc_frame_id=0xFFFFFFF0, max_frames=30, n_kfs=31)
    assert M.decide_literal(D, 40, 0, 0, 100)[0] == 0
    D = M.default_decision(frame_id=100, last_reloc_frame_id=90, max_frames=30, n_kfs=30)   # nKFs > mMaxFrames is false
    assert M.decide_literal(D, 40, 0, 0, 100)[0] == 0
    # int < int * float: 3 < 4 * 0.75f is false, 2 < 3 holds; int < int * 0.25 in double
    D = M.default_decision()
    assert M.decide_literal(D, 30, 0, 0, 40)[1] & 8 == 0 and M.decide_literal(D, 29, 0, 0, 40)[1] & 8 == 8
    assert M.decide_literal(D, 25, 0, 0, 100)[1] & 4 == 0 and M.decide_literal(D, 24, 0, 0, 100)[1] & 4 == 4
    # float, not double: 16777217 * 0.75f
    big = 16777217
    assert (M.decide_literal(D, 12582912, 0, 0, big)[1] & 8 == 8) == bool(np.float32(12582912) < np.float32(big) * np.float32(0.75))


def test_constructors_differ_only_in_negative_zero():
    fr = M.make_frame(3, 100, 128, 64)
    fr["cam"]["Rwc"] = np.eye(3, dtype=np.float32).reshape(9)
    fr["cam"]["Ow"] = 0
    fr["keys_un"]["x"][:4] = fr["cam"]["cx"] - np.float32(100)   # x < 0
    fr["keys_un"]["y"][:4] = fr["cam"]["cy"]                      # y == 0, and -0.0 for ... * z * invfy with a negative factor
    fr["keys_un"]["y"][2:4] = fr["cam"]["cy"] - np.float32(0)     # stays +0
    fr["depth"][:100] = 10
    sc = M.make_scales()
    idx = np.arange(100)
    a = M.construct_keyframe_points(fr["cam"], fr["keys_un"], fr["desc"], fr["depth"], idx, sc)
    b = M.construct_frame_points(fr["cam"], fr["keys_un"], fr["desc"], fr["depth"], idx, sc)
    assert (a["observed"] == 1).all() and (b["observed"] == 0).all() and (a["skip"] == 0).all()
    for k in ("pos", "min_distance", "max_distance", "desc"):
        assert a[k].tobytes() == b[k].tobytes()
    assert (a["normal"] == b["normal"]).all()   # as values; as bytes only a -0.0f can differ
    diff = a["normal"].view(np.uint32) != b["normal"].view(np.uint32)
    assert (b["normal"].view(np.uint32)[diff] == 0x80000000).all() and (a["normal"].view(np.uint32)[diff] == 0).all()
    # against np_mappoint's literal UpdateNormalAndDepth for one observation
    from tests import np_mappoint
    for i in (0, 7, 50):
        nrm, mn, mx = np_mappoint.literal_normal_depth(a["pos"][i], [fr["cam"]["Ow"]], 0, fr["keys_un"]["octave"][i], sc["scale_factors"][0][:8])
        assert nrm.tobytes() == a["normal"][i].tobytes() and mn == a["min_distance"][i] and mx == a["max_distance"][i]


def test_struct_sizes_and_constants():
    assert _lib.KF_DECISION_DTYPE.itemsize == 56 and _lib.KF_SCALES_DTYPE.itemsize == 72 and _lib.KF_HEADER_DTYPE.itemsize == 64
    assert C.sizeof(_lib.KfCall) == 208 and _lib.MAP_POINT_DTYPE.itemsize == 72 and tracking.OBSERVED_OFFSET == 36
    assert _lib.LAST_POINT_DTYPE.fields["observed"][1] == 16 and _lib.LM_HEADER_DTYPE.fields["ref_kf"][1] == 12
    txt = open(_lib.HERE + "/../include/orbfe.h").read()
    for name, v in (("MAX_FRAMES", _lib.KF_MAX_FRAMES), ("MAX_CAP", _lib.KF_MAX_CAP), ("MAX_TOTAL_ROWS", _lib.KF_MAX_TOTAL_ROWS),
                    ("STATISTICS", 1), ("DECISION", 2), ("CREATE", 4), ("CLOSE_POINTS", 100), ("INIT_MIN_KEYS", 500)):
        assert f"#define ORBFE_KF_{name} {v}" in txt, name
    assert _lib.KF_MAX_CAP == _lib.POSE_MAX_ROWS


def test_limits_at_the_last_accepted_and_first_refused_value(L):
    gpu = _gpu_present(L)
    ok, bad = (_lib.OK if gpu else _lib.ERR_NO_DEVICE), _lib.ERR_INVALID
    a = np.zeros(128, np.uint8)   # stands for every array: with S == 0 nothing is launched and nothing behind a pointer is read
    base = a.ctypes.data + (-a.ctypes.data % 8)
    scales = M.make_scales()

    def call_of(scales=scales, **kw):
        c = _lib.KfCall()
        for k in _lib.KF_CALL_POINTERS:
            setattr(c, k, kw.pop(k, base))
        d = dict(S=0, cap=1, new_cap=1, p_cap=1, frame_shift=0, point_stride=72, observed_offset=36, ref_kf_stride=4, n_kf=0, n_map_points=0,
                 mode=0, flags=M.ALL)
        d.update(kw)
        for k, v in d.items():
            setattr(c, k, v)
        return c, scales

    def host(**kw):
        c, s = call_of(**kw)
        return L.orbfe_keyframe_insertion(C.byref(c), None if s is None else s.ctypes.data)

    def dev(**kw):
        c, s = call_of(**kw)
        return L.orbfe_keyframe_insertion_batch_device(C.byref(c), None if s is None else s.ctypes.data, None)

    for call in (host, dev):
        assert call() == ok
        assert call(cap=_lib.KF_MAX_CAP, new_cap=_lib.KF_MAX_CAP, n_kf=_lib.COV_MAX_KEYFRAMES, n_map_points=_lib.COV_MAX_POINTS, p_cap=2 ** 30,
                    frame_shift=2 ** 30, point_stride=12, observed_offset=8, ref_kf_stride=32, mode=2) == ok
        assert call(cap=_lib.KF_MAX_CAP + 1, new_cap=1) == bad and b"cap" in L.orbfe_last_error() and call(cap=0) == bad
        assert call(cap=8, new_cap=8) == ok and call(cap=8, new_cap=9) == bad and call(cap=8, new_cap=0) == bad
        assert call(S=_lib.KF_MAX_FRAMES + 1) == bad and call(S=-1) == bad
        assert call(n_kf=_lib.COV_MAX_KEYFRAMES + 1) == bad and call(n_kf=-1) == bad
        assert call(n_map_points=_lib.COV_MAX_POINTS + 1) == bad and call(n_map_points=-1) == bad
        assert call(p_cap=0) == bad and call(frame_shift=-1) == bad
        assert call(point_stride=8) == bad and call(point_stride=14) == bad and call(point_stride=12, observed_offset=-1) == ok
        assert call(observed_offset=-2) == bad and call(observed_offset=34) == bad and call(observed_offset=68) == ok
        assert call(observed_offset=72) == bad and call(ref_kf_stride=0) == bad and call(ref_kf_stride=6) == bad
        assert call(mode=3) == bad and call(mode=-1) == bad
        assert call(flags=0) == bad and call(flags=8) == bad and call(flags=M.DECISION) == bad and call(flags=M.DECISION | M.CREATE) == bad
        for flags in (M.STATISTICS, M.CREATE, M.STATISTICS | M.CREATE, M.STATISTICS | M.DECISION, M.ALL):
            assert call(flags=flags) == ok
        assert call(scales=_levels(1)) == ok and call(scales=_levels(16)) == ok and call(scales=_levels(17)) == bad
        assert call(scales=_levels(0)) == bad and call(scales=None) == bad
        # null arrays: what the flags need with S > 0, the tables with a count > 0
        # (a call that is accepted with S > 0 would run on these stand-in arrays: it is made only where no device exists, and the
        # validation answers ERR_NO_DEVICE behind its last check; with a device the GPU suite makes those calls on real arrays)
        live = (lambda **kw: call(**kw) == ok) if not gpu else (lambda **kw: True)
        for k in ("n", "depth", "headers", "decision", "ref_kf", "keys_un", "desc", "cam", "new_points", "new_index", "n_new"):
            assert call(S=1, **{k: None}) == bad, k
            assert call(S=0, **{k: None}) == ok, k
        for k in ("points", "n_points"):
            assert call(S=1, **{k: None}) == bad and live(S=1, assigned=None, **{k: None})
        assert live(S=1, flags=M.STATISTICS, keys_un=None, desc=None, cam=None, new_points=None, new_index=None, n_new=None, ref_kf=None)
        assert live(S=1, flags=M.CREATE, decision=None, ref_kf=None, keyframes=None)
        assert call(n_kf=1, keyframes=None) == bad and call(n_map_points=1, point_bad=None) == bad
        assert call(n_map_points=1, point_observations=None) == bad and call(n_kf=1, flags=M.CREATE, keyframes=None) == ok
        assert live(S=1, outlier=None, n_points_base=None, depth_selected=None, assigned=None, points=None, n_points=None)
        assert live(S=_lib.KF_MAX_FRAMES)
        # alignment
        for k in _lib.KF_CALL_POINTERS:
            if k not in ("outlier", "point_bad"):
                assert call(**{k: base + 2}) == bad, k
        assert call(decision=base + 4) == bad and call(keyframes=base + 4) == bad and call(outlier=base + 1, point_bad=base + 1) == ok
    # host form: the staged rows
    assert host(S=442, cap=9490, new_cap=1) == bad and b"rows" in L.orbfe_last_error()   # 442 x 9489 <= 4 194 304 < 442 x 9490
    assert host(S=4096, cap=1, p_cap=1025) == bad
    if not gpu:
        assert host(S=442, cap=9489, new_cap=1) == ok and host(S=4096, cap=1, p_cap=1024) == ok
        assert host(S=4096, cap=1, p_cap=1025, assigned=None) == ok and dev(S=442, cap=9490, new_cap=1, p_cap=2 ** 30) == ok
    assert L.orbfe_keyframe_insertion(None, scales.ctypes.data) == bad and L.orbfe_keyframe_insertion_batch_device(None, scales.ctypes.data, None) == bad


def _levels(n):
    s = M.make_scales()
    s["n_levels"] = n
    return s


def test_without_a_device_the_call_is_an_error_not_a_fallback(L, cases):
    problem, mode, flags, _, _ = cases["c100_far_behind"]
    fr = problem["frames"][0]
    run = lambda: tracking.create_new_keyframe(problem["scales"], depth=fr["depth"], n=fr["n"], keys_un=fr["keys_un"], desc=fr["desc"], cam=fr["cam"])
    if _gpu_present(L):
        assert run()["headers"]["n_created"] == 101
        return
    with pytest.raises(_lib.OrbfeError) as e:
        run()
    assert e.value.code == _lib.ERR_NO_DEVICE
