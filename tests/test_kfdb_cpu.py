"""CPU suite of the keyframe database: the two readings of tests/np_kfdb.py agree on every case; the conditions that make the GPU
comparison meaningful (stale-score reads that change a candidate list, a best-neighbour replacement, a de-duplication, an unscored
neighbour that becomes a candidate, a connected set that removes the top-scoring entry, si == minScore, an erase and re-add that
reorders the output, an empty result at each early return, the ordered-sum pair) ASSERTED on the case list; csrc/kfdb_internal.h
compiled for the host against the literal reading bit for bit; struct sizes, exports, header text; what is validated before a
device is touched; ORBFE_ERR_NO_DEVICE from create."""
import ctypes as C
import os

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_kfdb as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_kfdb", "_build", "libkfdb_host.so")
STRIPS = (0, 1, _lib.KFDB_STRIP - 1, _lib.KFDB_STRIP, _lib.KFDB_STRIP + 1)


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    out = {name: f() for name, f in K.CASES.items()}
    for n in STRIPS:
        out[f"strip_{n}"] = K.strip_case(n)
    out["ordered_sum"] = K.ordered_sum_case()[:2]
    return out


@pytest.fixture(scope="module")
def literal(cases):
    return {name: K.run(K.Literal(n_words), ops) for name, (n_words, ops) in cases.items()}


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def _queries(results):
    return [x for r in results if isinstance(r, list) for x in r]


def _events(results, key):
    return sum(x["events"].get(key, 0) for x in _queries(results))


# ---- the readings ------------------------------------------------------------------------------------------------------------------
def test_the_two_readings_agree_on_every_case(cases, literal):
    n_queries = 0
    for name, (n_words, ops) in cases.items():
        assert K.same(literal[name], K.run(K.SetReading(n_words), ops)), name
        n_queries += len(_queries(literal[name]))
    assert n_queries >= 150


def test_stale_scores_are_read_and_change_a_candidate_list(cases, literal):
    for name in ("reloc_sequence", "reloc_edges"):
        n_words, ops = cases[name]
        assert _events(literal[name], "stale_nonzero") >= 2
        zeroed = K.run(K.Literal(n_words, zero_stale=True), ops)
        changed = [a["cand"] != b["cand"] for a, b in zip(_queries(literal[name]), _queries(zeroed))]
        assert any(changed), name
    assert _queries(literal["reloc_edges"])[1]["cand"] == [10]           # the stale neighbour itself, once; Z fell under the threshold
    assert _queries(K.run(K.Literal(2000, zero_stale=True), cases["reloc_edges"][1]))[1]["cand"] == [11, 12, 13]


def test_replacement_deduplication_and_unscored_candidates_occur(literal):
    for name in ("reloc_sequence", "loop_basic", "reloc_edges"):
        assert _events(literal[name], "replacements") > 0 and _events(literal[name], "dedups") > 0, name
    assert _events(literal["reloc_sequence"], "unscored_candidates") > 0 and _events(literal["reloc_edges"], "unscored_candidates") == 1


def test_loop_edges(cases, literal):
    free, without_top, at_min, above_all, disjoint = literal["loop_edges"][0]
    slot_ids = K.Literal(cases["loop_edges"][0])
    K.run(slot_ids, [op for op in cases["loop_edges"][1] if op[0] != "loop"])
    top = max(free["dense"], key=lambda s: free["dense"][s][1])
    assert top in free["dense"] and top not in without_top["dense"]      # the connected set removed the top-scoring entry
    assert slot_ids.slot_ids[top] in free["cand"] and slot_ids.slot_ids[top] not in without_top["cand"]
    assert without_top["info"]["n_sharing"] == free["info"]["n_sharing"] - 1
    assert at_min["events"]["equal_min_score"] == 1 and 0 < at_min["info"]["n_matches"] < at_min["info"]["n_scored"]
    assert above_all["cand"] == [] and above_all["info"]["n_scored"] > 0 and above_all["info"]["n_matches"] == 0        # :138
    assert above_all["info"]["best_acc_score"] == 0 and len(above_all["dense"]) == above_all["info"]["n_scored"]
    assert disjoint["cand"] == [] and disjoint["info"]["n_sharing"] == 0 and disjoint["dense"] == {}                    # :102


def test_reloc_early_return_and_erase_readd(literal):
    c = _queries(literal["reloc_edges"])[2]
    assert c["cand"] == [] and c["info"]["n_sharing"] == 0                                                               # :219
    first, erased, readded = (r[0]["cand"] for r in literal["erase_readd"])
    assert first == [1, 2] and erased == [2] and readded == [2, 1]


def test_the_ordered_sum_pair_rounds_differently_when_summed_in_strides():
    n_words, ops, strided = K.ordered_sum_case()
    got = K.run(K.Literal(n_words), ops)
    ordered = got[0][0]["dense"][0][1]
    assert ordered != strided and got[1][0] == ordered
    assert abs(int(np.float32(ordered).view(np.uint32)) - int(np.float32(strided).view(np.uint32))) == 1


# ---- kfdb_internal.h on the host -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(L):
    import subprocess
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_kfdb"), "_build/libkfdb_host.so"], check=True, capture_output=True)
    H = C.CDLL(HOST_LIB)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    H.kfdb_host_min_common_words.argtypes = [ci]
    H.kfdb_host_score.argtypes = [vp, vp, ci, vp, vp, ci]
    H.kfdb_host_score.restype = cf
    H.kfdb_host_finish_terms.argtypes = [vp, ci]
    H.kfdb_host_finish_terms.restype = cf
    H.kfdb_host_term.argtypes = [C.c_double, C.c_double]
    H.kfdb_host_term.restype = C.c_double
    H.kfdb_host_accumulate.argtypes = [cf, ci, ci, vp, vp, vp, vp]
    H.kfdb_host_min_score_to_retain.argtypes = [cf]
    H.kfdb_host_min_score_to_retain.restype = cf
    return H


def _bits(x):
    return np.float32(x).tobytes()


def test_internal_header_on_the_host_equals_the_reading(cases, literal, host):
    assert host.kfdb_host_strip() == _lib.KFDB_STRIP
    for m in range(0, 4097):
        assert host.kfdb_host_min_common_words(m) == K.min_common_words(m)
    n_scores = n_acc = 0
    for name, (n_words, ops) in cases.items():
        slots, results = [], iter(literal[name])
        for op in ops:
            if op[0] == "add":
                slots.append((np.ascontiguousarray(op[2], np.int32), np.ascontiguousarray(op[3], np.float64)))
            elif op[0] == "clear":
                slots = []
            elif op[0] == "score":
                next(results)
            elif op[0] in ("reloc", "loop"):
                for q, x in zip(op[1], next(results)):
                    qi, qv = np.ascontiguousarray(q["ids"], np.int32), np.ascontiguousarray(q["vals"], np.float64)
                    info = x["info"]
                    assert host.kfdb_host_min_common_words(info["max_common_words"]) == info["min_common_words"]
                    for s, (_, si) in x["dense"].items():
                        ei, ev = slots[s]
                        got = host.kfdb_host_score(_lib.ptr(qi), _lib.ptr(qv), len(qi), _lib.ptr(ei), _lib.ptr(ev), len(ei))
                        assert _bits(got) == _bits(si), (name, s)
                        n_scores += 1
                    if info["n_matches"]:
                        assert _bits(host.kfdb_host_min_score_to_retain(info["best_acc_score"])) == _bits(info["min_score_to_retain"])
                    for si, kid, added, acc, best in x["trace"]:
                        s2 = np.array([a[0] for a in added], np.float32)
                        i2 = np.array([a[1] for a in added], np.int32)
                        a_out, b_out = C.c_float(0), C.c_int32(0)
                        host.kfdb_host_accumulate(float(si), int(kid), len(added), _lib.ptr(s2), _lib.ptr(i2), C.byref(a_out), C.byref(b_out))
                        assert _bits(a_out.value) == _bits(acc) and b_out.value == best, (name, kid)
                        n_acc += 1
    assert n_scores > 400 and n_acc > 400


def test_the_chunked_in_order_sum_of_the_score_pass_is_the_ordered_sum(host):
    n_words, ops, strided = K.ordered_sum_case()
    ids, ev = ops[0][2], ops[0][3]
    qv = ops[1][1][0]["vals"]
    terms = np.array([host.kfdb_host_term(float(a), float(b)) for a, b in zip(qv, ev)], np.float64)
    want = K.l1_score(ids, qv, ids, ev)
    assert _bits(host.kfdb_host_finish_terms(_lib.ptr(terms), len(terms))) == _bits(want) != _bits(strided)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
def test_struct_sizes_exports_and_header_text(L):
    assert _lib.KFDB_INFO_DTYPE.itemsize == 32 and tuple(_lib.KFDB_INFO_DTYPE.names) == K.INFO_FIELDS
    assert _lib.KFDB_INFO_DTYPE.fields["best_acc_score"][1] == 20 and _lib.KFDB_INFO_DTYPE.fields["n_candidates"][1] == 28
    names = [s for s in _lib.EXPORTS if s.startswith("orbfe_kfdb_")]
    assert len(names) == 13 and all(hasattr(L, s) for s in names)
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for text in ("} orbfe_kfdb_query_info;", "/* 32 bytes */", f"#define ORBFE_KFDB_MAX_WORDS {_lib.KFDB_MAX_WORDS} ",
                 f"#define ORBFE_KFDB_NEIGHBOURS {_lib.KFDB_NEIGHBOURS} ", f"#define ORBFE_KFDB_MAX_QUERIES {_lib.KFDB_MAX_QUERIES} ",
                 f"#define ORBFE_KFDB_MAX_SLOTS {_lib.KFDB_MAX_SLOTS} ", f"#define ORBFE_KFDB_MAX_CELLS {_lib.KFDB_MAX_CELLS} ",
                 "#define ORBFE_KFDB_SCORE_UNKNOWN (-1.0f)", "ORBFE_KFDB_L1_NORM = 0"):
        assert text in hdr, text
    for s in names:
        assert f"int {s}(" in hdr, s
    internal = open(os.path.join(ROOT, "refactored_orb_slam2_amd", "csrc", "kfdb_internal.h")).read()
    assert f"#define KFDB_STRIP {_lib.KFDB_STRIP} " in internal
    assert K.NEIGHBOURS == _lib.KFDB_NEIGHBOURS and float(K.SCORE_UNKNOWN) == _lib.KFDB_SCORE_UNKNOWN


def test_create_validates_before_it_looks_for_a_device_and_null_handles_are_refused(L):
    h = C.c_void_p(None)
    assert L.orbfe_kfdb_create(100, _lib.KFDB_L1_NORM, 0, None) == _lib.ERR_INVALID
    for n_words, scoring in ((0, _lib.KFDB_L1_NORM), (-1, _lib.KFDB_L1_NORM), (100, _lib.KFDB_L2_NORM), (100, 5), (100, -1)):
        assert L.orbfe_kfdb_create(n_words, scoring, 0, C.byref(h)) == _lib.ERR_INVALID and not h.value, (n_words, scoring)
    assert b"L1_NORM" in L.orbfe_last_error()
    ids, vals, one = np.zeros(1, np.int32), np.ones(1), np.zeros(2, np.int32)
    out64, out32 = np.zeros(1, np.int64), np.zeros(1, np.int32)
    assert L.orbfe_kfdb_destroy(None) == 0
    assert L.orbfe_kfdb_clear(None) == L.orbfe_kfdb_size(None, None, None) == L.orbfe_kfdb_erase(None, 1) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_add(None, 1, _lib.ptr(ids), _lib.ptr(vals), 1) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_slots(None, _lib.ptr(out64), 1, None) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_set_covisibles(None, 0, None, None) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_score(None, _lib.ptr(ids), _lib.ptr(vals), 1, _lib.ptr(out64), 1, _lib.ptr(out32)) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_detect_relocalization(None, 1, _lib.ptr(one), _lib.ptr(ids), _lib.ptr(vals), 1, _lib.ptr(out64), _lib.ptr(out32),
                                              None, None, None) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_detect_relocalization_device(None, 1, _lib.ptr(one), _lib.ptr(ids), _lib.ptr(vals), 1, _lib.ptr(out64),
                                                     _lib.ptr(out32), None, None, None, None) == _lib.ERR_INVALID
    ms = np.zeros(1, np.float32)
    assert L.orbfe_kfdb_detect_loop(None, 1, _lib.ptr(one), _lib.ptr(ids), _lib.ptr(vals), _lib.ptr(ms), _lib.ptr(one), _lib.ptr(out64), 1,
                                    _lib.ptr(out64), _lib.ptr(out32), None, None, None) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_detect_loop_device(None, 1, _lib.ptr(one), _lib.ptr(ids), _lib.ptr(vals), _lib.ptr(ms), _lib.ptr(one),
                                           _lib.ptr(out64), 1, _lib.ptr(out64), _lib.ptr(out32), None, None, None, None) == _lib.ERR_INVALID


def test_no_device_is_an_error_from_create(L):
    from refactored_orb_slam2_amd.keyframe_database import KeyFrameDatabase
    if _gpu_present(L):
        db = KeyFrameDatabase(100)
        assert db.size() == (0, 0)
        db.close()
        return
    h = C.c_void_p(None)
    assert L.orbfe_kfdb_create(100, _lib.KFDB_L1_NORM, 0, C.byref(h)) == _lib.ERR_NO_DEVICE and not h.value
    with pytest.raises(_lib.OrbfeError) as e:
        KeyFrameDatabase(100)
    assert e.value.code == _lib.ERR_NO_DEVICE
