"""CPU suite of the local map of a tracked frame (orbfe_local_map*): the two readings of tests/np_localmap.py agree on every directed
case and on seeded maps, every directed case reaches the edges it was built for and together they reach all of np_localmap.EDGES;
csrc/localmap_internal.h compiled for the host under the address and undefined-behaviour sanitizers (tests/cpp_localmap/host_arith.cpp, a
stand-alone program) gives the table reading's bytes; pack_local_map builds the yardstick's tables; every ORBFE_LM_MAX_* and every null
array with a count is refused without a device; the struct sizes are the header's; the host form without a device is an error."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, local_map
from tests import np_localmap as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbfe_local_map", "orbfe_local_map_batch_device")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    return M.directed_cases()


@pytest.fixture(scope="module")
def maps():
    out = {}
    for seed in (1, 2, 3):
        scene, frames = M.make_local_map(seed)
        out["map%d" % seed] = {"scene": scene, "frames": frames, "conn_cap": 64, "kf_cap": 64, "p_cap": 1024, "reaches": set(), "tamper": None}
    return out


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def _literal_agrees(problem, name):
    """the literal reading of every frame the tables accept against the table reading's lists"""
    T = M.tables_of(problem)
    n = 0
    for s, (slots, seen) in enumerate(problem["frames"]):
        status, n_voted, local, ref_kf, stop, points, skip = M.frame_reading(T, s, problem["conn_cap"])
        if status == M.REFUSED:
            continue
        lit = M.literal_local_map(problem["scene"], slots, seen)
        assert lit["empty"] == (status == M.EMPTY), name
        if status == M.EMPTY:
            continue
        assert lit["local_kf"] == local and lit["n_voted"] == n_voted, (name, s)
        assert (-1 if lit["ref_kf"] is None else lit["ref_kf"]) == ref_kf, (name, s)
        assert {"exhausted": M.STOP_EXHAUSTED, "size": M.STOP_SIZE, "parent": M.STOP_PARENT}[lit["stop"]] == stop, (name, s)
        assert lit["local_points"] == points and lit["skip"] == skip, (name, s)
        assert lit["marked_kf"] == sorted(local) and lit["marked_points"] == sorted(points), (name, s)
        assert len(local) <= max(n_voted, 83)
        n += 1
    return n


def test_the_two_readings_agree_on_every_directed_case(cases):
    n = 0
    for name, p in cases.items():
        if p["tamper"] is None:
            n += _literal_agrees(p, name)
    assert n >= 25


def test_the_two_readings_agree_on_seeded_maps(maps):
    stops = set()
    for name, p in maps.items():
        assert _literal_agrees(p, name) == len(p["frames"])
        rec = M.table_reading(M.tables_of(p), p["conn_cap"], p["kf_cap"], p["p_cap"])
        assert (rec["headers"]["status"] == M.OK).all() and (rec["headers"]["n_local_kf"] > rec["headers"]["n_voted"]).any()
        assert (rec["map_points"]["skip"][0, :rec["n_points"][0]] == 1).any() and (rec["map_points"]["skip"][0, :rec["n_points"][0]] == 0).any()
        stops |= set(rec["headers"]["stop"].tolist())
    assert stops >= {M.STOP_EXHAUSTED, M.STOP_PARENT}


def test_the_census_holds(cases):
    reached = set()
    for name, p in cases.items():
        got = M.census_of(p)
        assert p["reaches"] and p["reaches"] <= got, (name, p["reaches"] - got)
        reached |= got
    assert set(M.EDGES) <= reached, set(M.EDGES) - reached
    # one REFUSED frame of each cause, between two frames it does not touch
    for cause in M.REFUSAL_CAUSES:
        p = cases["refused_" + cause]
        rec = M.table_reading(M.tables_of(p), p["conn_cap"], p["kf_cap"], p["p_cap"])
        assert rec["headers"]["status"].tolist() == [M.OK, M.REFUSED, M.OK], cause
        assert rec["headers"][1].tolist()[:5] == (0, 0, 0, -1, 0) and rec["n_points"][1] == 0
        assert (rec["local_kf"][1].view(np.uint8) == M.CANARY).all() and (rec["map_points"][1].view(np.uint8) == M.CANARY).all()
        clean = dict(p, tamper=None, conn_cap=8) if cause not in ("vote_refused", "seen_index", "seen_negative") else None
        if clean:   # without the damage the middle frame is a good one
            assert M.table_reading(M.tables_of(clean), 8, p["kf_cap"], p["p_cap"])["headers"]["status"].tolist() == [M.OK] * 3, cause
    # the caps: exact counts, the first cap written, nothing behind them
    rec = M.table_reading(M.tables_of(cases["p_cap_over"]), 128, 16, cases["p_cap_over"]["p_cap"])
    assert rec["headers"]["status"][0] == M.OVERFLOW and rec["headers"]["n_local_points"][0] == rec["n_points"][0] + 1
    rec = M.table_reading(M.tables_of(cases["kf_cap_over"]), 128, cases["kf_cap_over"]["kf_cap"], 64)
    assert rec["headers"]["status"][0] == M.OVERFLOW and rec["headers"]["n_local_kf"][0] == cases["kf_cap_over"]["kf_cap"] + 1
    assert M.table_reading(M.tables_of(cases["p_cap_exact"]), 128, 16, cases["p_cap_exact"]["p_cap"])["headers"]["status"][0] == M.OK


def test_pack_local_map_builds_the_yardsticks_tables(cases, maps):
    for name, p in list(cases.items()) + list(maps.items()):
        T = M.tables_of(dict(p, tamper=None))
        pack = local_map.pack_local_map(p["scene"]["keyframes"], p["scene"]["points"])
        assert pack["graph"].tobytes() == T["graph"].tobytes() and pack["graph"].dtype == _lib.LM_GRAPH_DTYPE, name
        assert np.array_equal(pack["children"], T["children"]) and pack["children"].dtype == np.int32, name
        assert np.array_equal(pack["kf_bad"], T["kf_bad"]) and np.array_equal(pack["point_bad"], T["point_bad"]), name
        assert np.array_equal(pack["table"]["n_keys"], T["n_keys"]), name
        seen, frames = local_map.pack_seen([s for _, s in p["frames"]])
        assert np.array_equal(seen, T["seen"]) and frames.tobytes() == T["frames"].tobytes(), name


def write_problems(path, problems):
    """the stream tests/cpp_localmap/host_arith.cpp reads"""
    i32 = lambda a: np.ascontiguousarray(a).astype(np.int32).tobytes()
    with open(path, "wb") as f:
        f.write(i32([len(problems)]))
        for p, T in problems:
            S = len(T["subjects"])
            f.write(i32([S, p["conn_cap"], p["kf_cap"], p["p_cap"], len(T["kf_bad"]), len(T["point_bad"]), len(T["children"]),
                         len(T["frame_slots"]), len(T["seen"]), 1]))
            f.write(T["vote_headers"].tobytes() + np.ascontiguousarray(T["vote_entries"]).tobytes() + T["graph"].tobytes())
            f.write(i32(T["children"]) + i32(T["kf_bad"]) + i32(T["point_bad"]) + i32(T["n_keys"]) + i32(T["slots_state"]))
            for sl in T["kf_slots"]:
                f.write(i32([len(sl)]) + i32(sl))
            f.write(i32(T["frame_slots"]) + T["subjects"].tobytes() + i32(T["seen"]) + T["frames"].tobytes() + T["records"].tobytes())


def test_host_build_under_sanitizers_equals_the_table_reading(L, cases, maps, tmp_path):
    """a stand-alone program with its own main; it is started as a process of its own, never loaded into this one"""
    if _gpu_present(L):   # sanitizers stay away from GPUs; the rules are host code and the machines without one check them
        pytest.skip("a GPU is present")
    d = os.path.join(ROOT, "tests", "cpp_localmap")
    subprocess.run(["make", "-C", d, "_build/host_arith"], check=True, capture_output=True)
    problems = [(p, M.tables_of(p)) for p in list(cases.values()) + list(maps.values())]
    src, dst = str(tmp_path / "problems.bin"), str(tmp_path / "answers.bin")
    write_problems(src, problems)
    r = subprocess.run([os.path.join(d, "_build", "host_arith"), src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "local map host arithmetic: %d problems" % len(problems)
    got = open(dst, "rb").read()
    at = 0
    for (p, T), name in zip(problems, list(cases) + list(maps)):
        want = M.table_reading(T, p["conn_cap"], p["kf_cap"], p["p_cap"])
        for key in ("headers", "local_kf", "local_points", "n_points", "map_points"):
            b = want[key].tobytes()
            assert got[at:at + len(b)] == b, (name, key)
            at += len(b)
    assert at == len(got)


def test_struct_sizes_exports_and_header_text(L):
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    txt = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for name, size in (("orbfe_lm_graph", 56), ("orbfe_lm_frame", 8), ("orbfe_lm_header", 32)):   # host_arith.cpp asserts them on the structs
        assert re.search(r"typedef struct %s \{\s*/\*[^*]*\b%d bytes" % (name, size), txt), name
    assert (_lib.LM_GRAPH_DTYPE.itemsize, _lib.LM_FRAME_DTYPE.itemsize, _lib.LM_HEADER_DTYPE.itemsize) == (56, 8, 32)
    for mine, theirs in ((M.GRAPH_DTYPE, _lib.LM_GRAPH_DTYPE), (M.FRAME_DTYPE, _lib.LM_FRAME_DTYPE), (M.HEADER_DTYPE, _lib.LM_HEADER_DTYPE),
                         (M.MAP_POINT_DTYPE, _lib.MAP_POINT_DTYPE), (M.SUBJECT_DTYPE, _lib.COV_SUBJECT_DTYPE)):
        assert mine == theirs
    for name, val in (("ORBFE_LM_MAX_FRAMES", _lib.LM_MAX_FRAMES), ("ORBFE_LM_MAX_TOTAL_SEEN", _lib.LM_MAX_TOTAL_SEEN),
                      ("ORBFE_LM_MAX_TOTAL_RECORDS", _lib.LM_MAX_TOTAL_RECORDS), ("ORBFE_LM_BEST", _lib.LM_BEST), ("ORBFE_LM_SIZE", _lib.LM_SIZE)):
        assert f"#define {name} {val}\n" in txt or f"#define {name} {val} " in txt, name
    for name, other, val in (("ORBFE_LM_MAX_KEYFRAMES", "ORBFE_COV_MAX_KEYFRAMES", _lib.LM_MAX_KEYFRAMES),
                             ("ORBFE_LM_MAX_POINTS", "ORBFE_COV_MAX_POINTS", _lib.LM_MAX_POINTS),
                             ("ORBFE_LM_MAX_TOTAL_SLOTS", "ORBFE_COV_MAX_TOTAL_SLOTS", _lib.LM_MAX_TOTAL_SLOTS),
                             ("ORBFE_LM_MAX_TOTAL_CHILDREN", "ORBFE_COV_MAX_KEYFRAMES", _lib.LM_MAX_TOTAL_CHILDREN),
                             ("ORBFE_LM_MAX_P_CAP", "ORBFE_COV_MAX_POINTS", _lib.LM_MAX_P_CAP)):
        assert f"#define {name} {other}\n" in txt and val == getattr(_lib, other[6:]), name
    assert "#define ORBFE_LM_MAX_KF_CAP (ORBFE_COV_MAX_CONN + 3)\n" in txt and _lib.LM_MAX_KF_CAP == _lib.COV_MAX_CONN + 3
    # the marks, the list and the per-wave counts fit the 160 KiB of LDS one workgroup may claim
    assert _lib.LM_MAX_POINTS // 8 + _lib.LM_MAX_KEYFRAMES // 8 + 4 * (_lib.LM_MAX_KF_CAP + 1) + 4 * 48 <= 160 * 1024
    assert "Tracking.cc:1161-1214" in txt and ":1090-1113" in txt and ":1036-1049" in txt
    assert (M.OK, M.EMPTY, M.OVERFLOW, M.REFUSED) == (_lib.LM_OK, _lib.LM_EMPTY, _lib.LM_OVERFLOW, _lib.LM_REFUSED)
    assert (M.STOP_EXHAUSTED, M.STOP_SIZE, M.STOP_PARENT) == (_lib.LM_STOP_EXHAUSTED, _lib.LM_STOP_SIZE, _lib.LM_STOP_PARENT)
    assert (M.BEST, M.SIZE) == (_lib.LM_BEST, _lib.LM_SIZE)


def test_limits_at_the_last_accepted_and_first_refused_value(L):
    ok, bad = (_lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE), _lib.ERR_INVALID
    a = np.zeros(64, np.uint8)   # stands for every array: with S == 0 nothing is launched and nothing behind a pointer is read
    base = a.ctypes.data + (-a.ctypes.data % 8)
    keys = ("headers", "entries", "graph", "children", "keyframes", "kf_bad", "point_bad", "slots", "subjects", "frames", "seen", "records",
            "lm_headers", "local_kf", "local_points", "n_points_out", "map_points")

    def args(S=0, cap=1, n_children=0, n_kf=0, n_points=0, n_slots=0, n_seen=0, kf_cap=1, p_cap=1, p=base, **ptr):
        q = {k: ptr.get(k, p) for k in keys}
        return S, cap, n_children, n_kf, n_points, n_slots, n_seen, kf_cap, p_cap, q

    def host(**kw):
        S, cap, n_children, n_kf, n_points, n_slots, n_seen, kf_cap, p_cap, q = args(**kw)
        return L.orbfe_local_map(q["headers"], q["entries"], cap, q["graph"], q["children"], n_children, q["keyframes"], q["kf_bad"], n_kf,
                                 q["point_bad"], n_points, q["slots"], n_slots, q["subjects"], q["frames"], q["seen"], n_seen, q["records"], S,
                                 kf_cap, p_cap, q["lm_headers"], q["local_kf"], q["local_points"], q["n_points_out"], q["map_points"])

    def dev(**kw):
        S, cap, n_children, n_kf, n_points, n_slots, n_seen, kf_cap, p_cap, q = args(**kw)
        return L.orbfe_local_map_batch_device(S, q["headers"], q["entries"], cap, q["graph"], q["children"], n_children, q["keyframes"],
                                              q["kf_bad"], n_kf, q["point_bad"], n_points, q["slots"], n_slots, q["subjects"], q["frames"],
                                              q["seen"], n_seen, q["records"], kf_cap, p_cap, q["lm_headers"], q["local_kf"], q["local_points"],
                                              q["n_points_out"], q["map_points"], None)

    for call in (host, dev):
        assert call() == ok
        assert call(cap=_lib.COV_MAX_CONN, n_children=_lib.LM_MAX_TOTAL_CHILDREN, n_kf=_lib.LM_MAX_KEYFRAMES, n_points=_lib.LM_MAX_POINTS,
                    n_slots=_lib.LM_MAX_TOTAL_SLOTS, n_seen=_lib.LM_MAX_TOTAL_SEEN, kf_cap=_lib.LM_MAX_KF_CAP, p_cap=_lib.LM_MAX_P_CAP) == ok
        assert call(n_kf=_lib.LM_MAX_KEYFRAMES + 1) == bad and b"n_kf" in L.orbfe_last_error()
        assert call(n_points=_lib.LM_MAX_POINTS + 1) == bad and call(n_children=_lib.LM_MAX_TOTAL_CHILDREN + 1) == bad
        assert call(n_slots=_lib.LM_MAX_TOTAL_SLOTS + 1) == bad and call(n_seen=_lib.LM_MAX_TOTAL_SEEN + 1) == bad
        assert call(cap=_lib.COV_MAX_CONN + 1) == bad and call(cap=0) == bad and b"conn_cap" in L.orbfe_last_error()
        assert call(kf_cap=_lib.LM_MAX_KF_CAP + 1) == bad and call(kf_cap=0) == bad and b"kf_cap" in L.orbfe_last_error()
        assert call(p_cap=_lib.LM_MAX_P_CAP + 1) == bad and call(p_cap=0) == bad
        assert call(S=_lib.LM_MAX_FRAMES + 1) == bad and call(S=-1) == bad
        for k in ("n_children", "n_kf", "n_points", "n_slots", "n_seen"):
            assert call(**{k: -1}) == bad, k
        # a null array with a count
        for k in ("headers", "entries", "subjects", "lm_headers", "local_kf", "local_points", "n_points_out", "map_points"):
            assert call(S=1, **{k: None}) == bad, k
        for k in ("graph", "keyframes", "kf_bad"):
            assert call(n_kf=1, **{k: None}) == bad, k
        assert call(n_children=1, children=None) == bad and call(n_points=1, point_bad=None) == bad and call(n_slots=1, slots=None) == bad
        assert call(n_seen=1, seen=None) == bad and call(n_seen=1, frames=None) == bad
        assert call(frames=None, seen=None, records=None, map_points=None) == ok   # the optional ones
    for k in keys:
        if k not in ("kf_bad", "point_bad"):
            assert dev(**{k: base + 2}) == bad and b"aligned" in L.orbfe_last_error(), k
    assert dev(keyframes=base + 4) == bad
    # the record block of the host form: S x p_cap
    p_cap = _lib.LM_MAX_P_CAP
    S = _lib.LM_MAX_TOTAL_RECORDS // p_cap
    assert S * p_cap == _lib.LM_MAX_TOTAL_RECORDS and host(S=0, p_cap=p_cap) == ok
    assert host(S=S + 1, p_cap=p_cap) == bad and b"records" in L.orbfe_last_error()
    # what the host form reads behind its pointers before a device is touched: a keyframe's size, the slots of the whole table
    votes = np.zeros(1, _lib.COV_HEADER_DTYPE)
    votes["status"] = _lib.COV_EMPTY
    entries, subjects = np.zeros(1, _lib.COV_ENTRY_DTYPE), np.zeros(1, _lib.COV_SUBJECT_DTYPE)
    slots = np.full(_lib.COV_MAX_KEYS + 1, -1, np.int32)
    n_rows = _lib.COV_MAX_TOTAL_KEYS // _lib.COV_MAX_KEYS + 1
    table, graph, kf_bad = np.zeros(n_rows, _lib.COV_KEYFRAME_DTYPE), np.zeros(n_rows, _lib.LM_GRAPH_DTYPE), np.zeros(n_rows, np.uint8)
    graph["parent"] = -1
    table["slots"], table["n_keys"] = slots.ctypes.data, _lib.COV_MAX_KEYS
    table["n_keys"][-1] = _lib.COV_MAX_TOTAL_KEYS % _lib.COV_MAX_KEYS
    out = {"h": np.zeros(1, _lib.LM_HEADER_DTYPE), "k": np.zeros(1, np.int32), "p": np.zeros(1, np.int32), "n": np.zeros(1, np.int32)}
    call = lambda: L.orbfe_local_map(_lib.ptr(votes), _lib.ptr(entries), 1, _lib.ptr(graph), None, 0, _lib.ptr(table), _lib.ptr(kf_bad), n_rows,
                                     None, 0, None, 0, _lib.ptr(subjects), None, None, 0, None, 1, 1, 1, _lib.ptr(out["h"]), _lib.ptr(out["k"]),
                                     _lib.ptr(out["p"]), _lib.ptr(out["n"]), None)
    assert int(table["n_keys"].sum()) == _lib.COV_MAX_TOTAL_KEYS and call() == ok
    if ok == _lib.OK:
        assert out["h"][0]["status"] == M.EMPTY and out["h"][0]["ref_kf"] == -1
    table["n_keys"][-1] += 1
    assert call() == bad and b"slots in all" in L.orbfe_last_error()
    table["n_keys"][-1] -= 1
    table["n_keys"][0] = _lib.COV_MAX_KEYS + 1
    assert call() == bad and b"n_keys" in L.orbfe_last_error()
    table["n_keys"][0] = -1
    assert call() == bad


def test_no_device_is_an_error_not_a_fallback(L, cases):
    if _gpu_present(L):
        pytest.skip("a GPU is present")
    p = cases["exhausted"]
    T = M.tables_of(p)
    pack = local_map.pack_local_map(p["scene"]["keyframes"], p["scene"]["points"])
    with pytest.raises(_lib.OrbfeError) as e:
        local_map.local_map(pack, (T["vote_headers"], T["vote_entries"]), p["conn_cap"], (T["frame_slots"], T["subjects"]), 16, 64,
                            records=T["records"])
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
