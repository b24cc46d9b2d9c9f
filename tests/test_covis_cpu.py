"""CPU suite of the covisibility graph (KeyFrame::UpdateConnections, the vote of Tracking::UpdateLocalKeyFrames,
LocalMapping::KeyFrameCulling): the two readings of tests/np_covis.py agree on every committed scene; the directed culling scenes give
the verdicts they were built for; csrc/covis_internal.h compiled for the host (tests/cpp_covis/host_arith.cpp) gives the yardstick's
records byte for byte, refusals included; every switchable deviation changes at least three answers; struct sizes, exports and header
text; every limit at the last accepted and the first refused value, checked before a device is touched; ORBFE_ERR_NO_DEVICE."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, covisibility
from tests import np_covis as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_covis", "_build", "libcovis_host.so")
CANARY = 0x5C


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_covis"), "_build/libcovis_host.so"], check=True, capture_output=True)
    h = C.CDLL(HOST_LIB)
    vp, ci = C.c_void_p, C.c_int
    h.covis_host_count.argtypes = [vp, ci, vp, vp, ci, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp]
    h.covis_host_count.restype = None
    h.covis_host_cull.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, ci, vp]
    h.covis_host_cull.restype = None
    return h


@pytest.fixture(scope="module")
def maps():
    return M.committed_maps()


@pytest.fixture(scope="module")
def cull_maps():
    return M.committed_cull_maps()


@pytest.fixture(scope="module")
def count_cases():
    return M.directed_count_cases()


@pytest.fixture(scope="module")
def cull_cases():
    return M.directed_cull_cases()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def canary_entries(S, cap):
    return np.full((S, cap * 8), CANARY, np.uint8).view(M.ENTRY_DTYPE).reshape(S, cap)


# ---- the readings ------------------------------------------------------------------------------------------------------------------
def _count_answers(maps, dev=frozenset()):
    out = []
    for sc in maps:
        for slots, me, mode in M.map_subjects(sc):
            out.append(M.connections_view(sc, slots, me, dev) if mode == M.CONNECTIONS else M.votes_view(sc, slots, dev))
    return out


def _cull_answers(cull_maps, cull_cases, dev=frozenset()):
    out = [M.literal_cull(sc, local, mono, dev) for sc, problems in cull_maps for local, mono in problems]
    out += [M.literal_cull(sc, local, mono, dev) for sc, problems, _ in cull_cases.values() for local, mono in problems]
    return out


def test_the_two_readings_agree_on_every_scene(maps, cull_maps, cull_cases, count_cases):
    n_conn = n_votes = 0
    for sc in maps:
        for slots, me, mode in M.map_subjects(sc):
            if mode == M.CONNECTIONS:
                assert M.connections_view(sc, slots, me) == M.connections_view_of_records(sc, slots, me)
                n_conn += 1
            else:
                assert M.votes_view(sc, slots) == M.votes_view_of_records(sc, slots)
                n_votes += 1
    assert n_conn >= 80 and n_votes >= 30
    for name, (sc, subjects, cap) in count_cases.items():
        if name.startswith("refused") or len(sc["keyframes"]) > 1000:
            continue
        for slots, me, mode in subjects:
            if mode == M.CONNECTIONS:
                assert M.connections_view(sc, slots, me) == M.connections_view_of_records(sc, slots, me), name
            else:
                assert M.votes_view(sc, slots) == M.votes_view_of_records(sc, slots), name
    for sc, problems in cull_maps:
        for local, mono in problems:
            assert M.literal_cull(sc, local, mono) == M.cull_problem(sc, local, mono)
    for name, (sc, problems, _) in cull_cases.items():
        for local, mono in problems:
            assert M.literal_cull(sc, local, mono) == M.cull_problem(sc, local, mono), name


def test_the_scenes_hold_what_the_comparison_needs(maps, cull_maps, cull_cases, count_cases):
    ws = [w for v in _count_answers(maps) if v is not None and len(v[1]) and isinstance(v[0], list) for _, w in v[0]]
    assert {14, 15, 16} <= set(ws)                                            # weights on both sides of the threshold
    verdicts = [v for a in _cull_answers(cull_maps, {}) for _, _, v in a]
    assert verdicts.count(M.CULLED) >= 10 and verdicts.count(M.MARKED) >= 1 and verdicts.count(M.SKIPPED_ID0) >= 3
    for name, (sc, problems, want) in cull_cases.items():                     # the directed scenes give what they were built for
        if want is not None:
            assert [r for local, mono in problems for r in M.cull_problem(sc, local, mono)] == want, name
    h, e = M.count_records(*count_cases["tie_below_15"])
    sc = count_cases["tie_below_15"][0]
    order = [k["order"] for k in sc["keyframes"]]
    tied = [r for r in (1, 2, 4)]
    assert h[0]["single"] == 1 and h[0]["kf_max"] == min(tied, key=lambda r: order[r]) and e[0, 0]["kf"] == max(tied, key=lambda r: order[r])
    h, _ = M.count_records(*count_cases["cap_exact"])
    assert h[0]["status"] == M.OK and h[0]["n_counted"] == 8
    h, _ = M.count_records(*count_cases["cap_plus_one"])
    assert h[0]["status"] == M.OVERFLOW and h[0]["n_counted"] == 9 and h[0]["n_written"] == 8
    h, e = M.count_records(*count_cases["bad_keyframe_max"])
    assert h[0]["kf_max"] == 3 and h[0]["w_max"] == 9 and h[1]["kf_max"] == 2 and 2 not in e[0]["kf"][:h[0]["n_written"]]
    h, _ = M.count_records(*count_cases["refused_between"])
    assert h["status"].tolist() == [M.OK, M.REFUSED, M.OK, M.REFUSED, M.REFUSED, M.REFUSED, M.OK]
    h, _ = M.count_records(*count_cases["highest_row"])
    assert h[0]["kf_max"] == 32767


@pytest.mark.parametrize("dev", M.DEVIATIONS)
def test_each_deviation_changes_at_least_three_answers(maps, cull_maps, cull_cases, dev):
    d = frozenset([dev])
    changed = sum(a != b for a, b in zip(_count_answers(maps, d), _count_answers(maps)))
    changed += sum(a != b for a, b in zip(_cull_answers(cull_maps, cull_cases, d), _cull_answers(cull_maps, cull_cases)))
    assert changed >= 3, (dev, changed)


# ---- the header compiled for the host ----------------------------------------------------------------------------------------------
def host_count(H, sc, subjects, cap, entries=None):
    pack = covisibility.pack_covisibility(sc["keyframes"], sc["points"])
    slots, recs = covisibility.pack_subjects(subjects)
    headers = np.zeros(len(recs), _lib.COV_HEADER_DTYPE)
    entries = canary_entries(len(recs), cap) if entries is None else entries
    H.covis_host_count(_lib.ptr(pack["obs"]), len(pack["obs"]), _lib.ptr(pack["recs"]), _lib.ptr(pack["point_bad"]), len(pack["recs"]),
                       _lib.ptr(pack["kf_order"]), _lib.ptr(pack["kf_bad"]), len(pack["kf_order"]), _lib.ptr(slots), len(slots), _lib.ptr(recs),
                       len(recs), cap, _lib.ptr(headers), _lib.ptr(entries))
    return headers, entries


def host_cull(H, sc, problems):
    pack = covisibility.pack_covisibility(sc["keyframes"], sc["points"])
    local, recs = covisibility.pack_problems(problems)
    out = np.zeros(len(local), _lib.COV_VERDICT_DTYPE)
    H.covis_host_cull(_lib.ptr(pack["obs"]), len(pack["obs"]), _lib.ptr(pack["recs"]), _lib.ptr(pack["point_bad"]), _lib.ptr(pack["n_obs_weighted"]),
                      len(pack["recs"]), _lib.ptr(pack["table"]), len(pack["table"]), _lib.ptr(local), len(local), _lib.ptr(recs), len(recs),
                      _lib.ptr(out))
    return out


def test_host_build_equals_the_yardstick_counts(H, maps, count_cases):
    assert M.HEADER_DTYPE == _lib.COV_HEADER_DTYPE and M.ENTRY_DTYPE == _lib.COV_ENTRY_DTYPE
    for sc in maps:
        subjects = M.map_subjects(sc)
        for cap in (4, 64):
            want_h, want_e = M.count_records(sc, subjects, cap, prior=canary_entries(len(subjects), cap))
            got_h, got_e = host_count(H, sc, subjects, cap)
            assert got_h.tobytes() == want_h.tobytes() and got_e.tobytes() == want_e.tobytes()
    for name, (sc, subjects, cap) in count_cases.items():
        want_h, want_e = M.count_records(sc, subjects, cap, prior=canary_entries(len(subjects), cap))
        got_h, got_e = host_count(H, sc, subjects, cap)
        assert got_h.tobytes() == want_h.tobytes() and got_e.tobytes() == want_e.tobytes(), name


def cull_refusal_scene():
    """a map whose keyframes 1, 2, 3 hold, in this order, a point index outside the table, a point whose list names a keyframe outside
    the table, and a point whose list names a keypoint outside its keyframe; the rows around them are untouched"""
    sc = M.make_cull_map(7, n_kf=30, n_points=560)
    n_pts = len(sc["points"])
    sc["keyframes"][1]["slots"][-1] = n_pts
    p = next(q for q in sc["keyframes"][2]["slots"] if q >= 0)
    sc["points"][p]["obs"][0] = (len(sc["keyframes"]), 0)
    p = next(q for q in sc["keyframes"][3]["slots"] if q >= 0 and all(k not in (1, 2) for k, _ in sc["points"][q]["obs"]))
    k, _ = sc["points"][p]["obs"][-1]
    sc["points"][p]["obs"][-1] = (k, len(sc["keyframes"][k]["slots"]))
    return sc, [([12, 1, 15, 2, 3, 18, 30, -1, 20], False), ([22, 23, 24, 25], True)]


def test_host_build_equals_the_yardstick_culling(H, cull_maps, cull_cases):
    assert M.VERDICT_DTYPE == _lib.COV_VERDICT_DTYPE
    for sc, problems in cull_maps:
        assert host_cull(H, sc, problems).tobytes() == M.cull_records(sc, problems).tobytes()
    for name, (sc, problems, _) in cull_cases.items():
        assert host_cull(H, sc, problems).tobytes() == M.cull_records(sc, problems).tobytes(), name
    sc, problems = cull_refusal_scene()
    want = M.cull_records(sc, problems)
    assert host_cull(H, sc, problems).tobytes() == want.tobytes()
    assert (want["verdict"] == M.ROW_REFUSED).sum() >= 4 and (want["verdict"] != M.ROW_REFUSED).sum() >= 6


def test_host_ratio_is_the_double_comparison(H):
    for n in range(0, 400):
        for r in {0, n, (9 * n) // 10, (9 * n) // 10 + 1, max(0, (9 * n) // 10 - 1)}:
            assert H.covis_host_redundant(r, n) == int(r > 0.9 * n), (r, n)
    assert H.covis_host_threads() == 256


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
NAMES = ("orbfe_covis_count", "orbfe_covis_count_batch_device", "orbfe_covis_cull_keyframes", "orbfe_covis_cull_keyframes_batch_device")


def test_struct_sizes_exports_and_header_text(L):
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    txt = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for name, val in (("ORBFE_COV_MAX_KEYFRAMES", _lib.COV_MAX_KEYFRAMES), ("ORBFE_COV_MAX_CONN", _lib.COV_MAX_CONN),
                      ("ORBFE_COV_MAX_POINTS", _lib.COV_MAX_POINTS), ("ORBFE_COV_MAX_TOTAL_OBS", _lib.COV_MAX_TOTAL_OBS),
                      ("ORBFE_COV_MAX_TOTAL_SLOTS", _lib.COV_MAX_TOTAL_SLOTS), ("ORBFE_COV_MAX_SUBJECTS", _lib.COV_MAX_SUBJECTS),
                      ("ORBFE_COV_MAX_PROBLEMS", _lib.COV_MAX_PROBLEMS), ("ORBFE_COV_MAX_TOTAL_LOCAL", _lib.COV_MAX_TOTAL_LOCAL),
                      ("ORBFE_COV_MAX_KEYS", _lib.COV_MAX_KEYS), ("ORBFE_COV_MAX_TOTAL_KEYS", _lib.COV_MAX_TOTAL_KEYS),
                      ("ORBFE_COV_MAX_TOTAL_ENTRIES", _lib.COV_MAX_TOTAL_ENTRIES), ("ORBFE_COV_TH", _lib.COV_TH), ("ORBFE_COV_IS_ID0", _lib.COV_IS_ID0),
                      ("ORBFE_COV_NOT_ERASE", _lib.COV_NOT_ERASE)):
        assert f"#define {name} {val}\n" in txt or f"#define {name} {val} " in txt, name
    assert _lib.COV_MAX_KEYFRAMES >= 16384 and _lib.COV_MAX_KEYFRAMES * 4 + _lib.COV_MAX_CONN * 12 + 64 <= 160 * 1024
    assert "KeyFrame.cc:268-354" in txt and "Tracking.cc:1115-1159" in txt and "LocalMapping.cc:595-655" in txt
    assert (M.CONNECTIONS, M.VOTES) == (_lib.COV_CONNECTIONS, _lib.COV_VOTES)
    assert (M.OK, M.EMPTY, M.OVERFLOW, M.REFUSED) == (_lib.COV_OK, _lib.COV_EMPTY, _lib.COV_OVERFLOW, _lib.COV_REFUSED)
    assert (M.KEPT, M.CULLED, M.MARKED, M.SKIPPED_ID0, M.ROW_REFUSED) == (_lib.COV_KEPT, _lib.COV_CULLED, _lib.COV_MARKED,
                                                                        _lib.COV_SKIPPED_ID0, _lib.COV_ROW_REFUSED)


def _accepted(L):
    return _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE


def test_count_limits_at_the_last_accepted_and_first_refused_value(L):
    ok, bad = _accepted(L), _lib.ERR_INVALID
    a = np.zeros(64, np.uint8)   # stands for every array: with S == 0 nothing is launched and nothing behind a pointer is read
    base = a.ctypes.data + (-a.ctypes.data % 8)

    def host(S=0, n_obs=0, n_points=0, n_kf=0, n_slots=0, cap=1, p=base):
        return L.orbfe_covis_count(p, n_obs, p, p, n_points, p, p, n_kf, p, n_slots, p, S, cap, p, p)

    def dev(S=0, n_obs=0, n_points=0, n_kf=0, n_slots=0, cap=1, p=base):
        return L.orbfe_covis_count_batch_device(S, p, n_obs, p, p, n_points, p, p, n_kf, p, n_slots, p, cap, p, p, None)

    for call in (host, dev):
        assert call() == ok
        assert call(n_kf=_lib.COV_MAX_KEYFRAMES, n_obs=_lib.COV_MAX_TOTAL_OBS, n_points=_lib.COV_MAX_POINTS, n_slots=_lib.COV_MAX_TOTAL_SLOTS,
                    cap=_lib.COV_MAX_CONN) == ok
        assert call(n_kf=_lib.COV_MAX_KEYFRAMES + 1) == bad and b"n_kf" in L.orbfe_last_error()
        assert call(n_obs=_lib.COV_MAX_TOTAL_OBS + 1) == bad and call(n_points=_lib.COV_MAX_POINTS + 1) == bad
        assert call(n_slots=_lib.COV_MAX_TOTAL_SLOTS + 1) == bad and b"n_slots_total" in L.orbfe_last_error()
        assert call(cap=_lib.COV_MAX_CONN + 1) == bad and call(cap=0) == bad and b"conn_cap" in L.orbfe_last_error()
        assert call(S=_lib.COV_MAX_SUBJECTS + 1) == bad and call(S=-1) == bad
        for k in ("n_obs", "n_points", "n_kf", "n_slots"):
            assert call(**{k: -1}) == bad, k
        assert call(S=1, p=None) == bad and call(n_kf=1, p=None) == bad
    assert dev(p=base + 2) == bad and b"aligned" in L.orbfe_last_error()
    # the subjects of a launch: empty subjects, real arrays
    S = _lib.COV_MAX_SUBJECTS + 1
    subjects = np.zeros(S, _lib.COV_SUBJECT_DTYPE)
    subjects["self"] = -1
    headers, entries = np.zeros(S, _lib.COV_HEADER_DTYPE), np.zeros(S, _lib.COV_ENTRY_DTYPE)
    call = lambda S: L.orbfe_covis_count(None, 0, None, None, 0, None, None, 0, None, 0, _lib.ptr(subjects), S, 1, _lib.ptr(headers), _lib.ptr(entries))
    assert call(_lib.COV_MAX_SUBJECTS) == ok
    if ok == _lib.OK:
        assert (headers["status"][:-1] == M.EMPTY).all() and (headers["kf_max"][:-1] == -1).all()
    assert call(S) == bad
    # the entry block of the host form: S x conn_cap
    cap = _lib.COV_MAX_CONN
    S = _lib.COV_MAX_TOTAL_ENTRIES // cap
    entries = np.zeros((S + 1) * cap, _lib.COV_ENTRY_DTYPE)
    call = lambda S: L.orbfe_covis_count(None, 0, None, None, 0, None, None, 0, None, 0, _lib.ptr(subjects), S, cap, _lib.ptr(headers), _lib.ptr(entries))
    assert S * cap == _lib.COV_MAX_TOTAL_ENTRIES and call(S) == ok
    assert call(S + 1) == bad and b"entries" in L.orbfe_last_error()


def test_cull_limits_at_the_last_accepted_and_first_refused_value(L):
    ok, bad = _accepted(L), _lib.ERR_INVALID
    a = np.zeros(64, np.uint8)
    base = a.ctypes.data + (-a.ctypes.data % 8)

    def host(Q=0, n_obs=0, n_points=0, n_kf=0, n_local=0, p=base):
        return L.orbfe_covis_cull_keyframes(p, n_obs, p, p, p, n_points, p, n_kf, p, n_local, p, Q, p)

    def dev(Q=0, n_obs=0, n_points=0, n_kf=0, n_local=0, p=base):
        return L.orbfe_covis_cull_keyframes_batch_device(Q, p, n_obs, p, p, p, n_points, p, n_kf, p, n_local, p, p, None)

    for call in (host, dev):
        assert call() == ok
        assert call(n_kf=_lib.COV_MAX_KEYFRAMES, n_obs=_lib.COV_MAX_TOTAL_OBS, n_points=_lib.COV_MAX_POINTS, n_local=_lib.COV_MAX_TOTAL_LOCAL) == ok
        assert call(n_kf=_lib.COV_MAX_KEYFRAMES + 1) == bad and call(n_obs=_lib.COV_MAX_TOTAL_OBS + 1) == bad
        assert call(n_points=_lib.COV_MAX_POINTS + 1) == bad
        assert call(n_local=_lib.COV_MAX_TOTAL_LOCAL + 1) == bad and b"n_local_total" in L.orbfe_last_error()
        assert call(Q=_lib.COV_MAX_PROBLEMS + 1) == bad and call(Q=-1) == bad
        for k in ("n_obs", "n_points", "n_kf", "n_local"):
            assert call(**{k: -1}) == bad, k
        assert call(Q=1, p=None) == bad and call(n_kf=1, p=None) == bad
    assert dev(p=base + 4) == bad and dev(p=base + 2) == bad and b"aligned" in L.orbfe_last_error()
    # what the host form reads behind its pointers before a device is touched: a keyframe's size, a problem's range
    keys = np.zeros(_lib.COV_MAX_KEYS + 1, _lib.KP_DTYPE)
    slots = np.full(_lib.COV_MAX_KEYS + 1, -1, np.int32)
    table = np.zeros(1, _lib.COV_KEYFRAME_DTYPE)
    table["keys_un"], table["slots"] = keys.ctypes.data, slots.ctypes.data
    local, out = np.zeros(1, np.int32), np.zeros(1, _lib.COV_VERDICT_DTYPE)
    problem = np.zeros(1, _lib.COV_PROBLEM_DTYPE)
    problem["n_local"], problem["monocular"] = 1, 1
    call = lambda: L.orbfe_covis_cull_keyframes(None, 0, None, None, None, 0, _lib.ptr(table), 1, _lib.ptr(local), 1, _lib.ptr(problem), 1, _lib.ptr(out))
    table["n_keys"] = _lib.COV_MAX_KEYS
    assert call() == ok
    if ok == _lib.OK:
        assert out[0].tolist() == (0, 0, M.KEPT, 0)
    table["n_keys"] = _lib.COV_MAX_KEYS + 1
    assert call() == bad and b"n_keys" in L.orbfe_last_error()
    table["n_keys"] = -1
    assert call() == bad
    table["n_keys"], table["keys_un"] = 4, 0
    assert call() == bad and b"keypoint array" in L.orbfe_last_error()
    table["keys_un"] = keys.ctypes.data
    # the keypoints of the whole table: rows may share their arrays, the host form stages each row's own copy
    n_rows = _lib.COV_MAX_TOTAL_KEYS // _lib.COV_MAX_KEYS + 1
    big = np.zeros(n_rows, _lib.COV_KEYFRAME_DTYPE)
    big["keys_un"], big["slots"], big["n_keys"] = keys.ctypes.data, slots.ctypes.data, _lib.COV_MAX_KEYS
    big["n_keys"][-1] = _lib.COV_MAX_TOTAL_KEYS % _lib.COV_MAX_KEYS
    call_big = lambda: L.orbfe_covis_cull_keyframes(None, 0, None, None, None, 0, _lib.ptr(big), n_rows, _lib.ptr(local), 1, _lib.ptr(problem), 1,
                                                    _lib.ptr(out))
    problem["local_offset"], problem["n_local"] = 0, 1
    assert int(big["n_keys"].sum()) == _lib.COV_MAX_TOTAL_KEYS and call_big() == ok
    big["n_keys"][-1] += 1
    assert call_big() == bad and b"keypoints in all" in L.orbfe_last_error()
    # the problems of a launch: empty problems, real arrays
    many = np.zeros(_lib.COV_MAX_PROBLEMS + 1, _lib.COV_PROBLEM_DTYPE)
    call_q = lambda Q: L.orbfe_covis_cull_keyframes(None, 0, None, None, None, 0, _lib.ptr(table), 1, _lib.ptr(local), 1, _lib.ptr(many), Q, _lib.ptr(out))
    assert call_q(_lib.COV_MAX_PROBLEMS) == ok and call_q(_lib.COV_MAX_PROBLEMS + 1) == bad
    for off, n, want in ((0, 1, ok), (1, 0, ok), (1, 1, bad), (0, 2, bad), (-1, 1, bad), (0, -1, bad)):
        problem["local_offset"], problem["n_local"] = off, n
        assert call() == want, (off, n)


def test_no_device_is_an_error_not_a_fallback(L):
    if _gpu_present(L):
        pytest.skip("a GPU is present")
    sc = M.make_cull_map(1)
    pack = covisibility.pack_covisibility(sc["keyframes"], sc["points"])
    with pytest.raises(_lib.OrbfeError) as e:
        covisibility.covisibility_counts(pack, M.map_subjects(sc)[:2], 8)
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(_lib.OrbfeError) as e:
        covisibility.cull_keyframes(pack, [([1, 2, 3], False)])
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
