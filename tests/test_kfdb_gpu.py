"""GPU suite of the keyframe database (kfdb_kernels.hip behind orbfe_kfdb_*) against the literal reading of tests/np_kfdb.py.  Nothing
is compared with a tolerance: candidate ids in order, n_cand, every info field (the two floats as bits), the dense common-word counts
and the dense scores as bits are EQUAL to the reading on every named case (the "shapes" case holds the entry lengths 0, 1, 63, 64, 65,
128, 129, the query lengths 1, 63, 64, 65, 4096, the common word first, last or alone and the word ids 0 and n_words - 1; "interleaved",
"reloc_singles" and "erase_readd" interleave add, erase, clear and re-add with queries and score calls, unknown ids included), for
entry counts around a strip of the common pass, and on the ordered-sum pair.  Then the properties of the call forms: a batch equals
single calls in order byte for byte and differs from the reversed order exactly where the reading does, loop queries do not depend on
their position, the device form equals the host form, sentinels behind every count survive, cand_cap truncates the list only, two
identical databases give identical bytes."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from refactored_orb_slam2_amd.keyframe_database import KeyFrameDatabase, pack_connected, pack_queries
from tests import np_kfdb as K

pytestmark = pytest.mark.gpu
SENTINEL = -7
SENTINEL_BITS = 0xDEADBEEF


class LibraryReading:
    """the ops of a case on the library, results in the shape of K.run"""

    def __init__(self, n_words):
        self.db = KeyFrameDatabase(n_words)

    def add(self, kid, ids, vals):
        self.db.add(kid, ids, vals)

    def erase(self, kid):
        self.db.erase(kid)

    def clear(self):
        self.db.clear()

    def covis(self, kid, row):
        self.db.set_covisibles([kid], [row])

    def score(self, q, kf_ids):
        return self.db.score(q["ids"], q["vals"], kf_ids)

    def _convert(self, det):
        out = []
        for q in range(len(det.n_cand)):
            w, s = det.common_words[q], det.scores[q]
            assert np.array_equal(w == -1, np.isnan(s))          # both dense outputs are written for the same slots, no others
            info = {f: det.info[q][f] for f in K.INFO_FIELDS}
            for f in K.INFO_FIELDS:
                info[f] = np.float32(info[f]) if f in ("best_acc_score", "min_score_to_retain") else int(info[f])
            assert int(det.n_cand[q]) == info["n_candidates"] == len(det.candidates[q])
            out.append(dict(cand=det.candidates[q].tolist(), info=info, dense={int(k): (int(w[k]), s[k]) for k in np.flatnonzero(w != -1)}))
        return out

    def reloc(self, batch):
        return self._convert(self.db.detect_relocalization_batch([(q["ids"], q["vals"]) for q in batch], dense=True))

    def loop(self, batch):
        return self._convert(self.db.detect_loop_batch([(q["ids"], q["vals"]) for q in batch], [q["min_score"] for q in batch],
                                                       [q["connected"] for q in batch], dense=True))


def _check(n_words, ops):
    want = K.run(K.Literal(n_words), ops)
    lib = LibraryReading(n_words)
    got = K.run(lib, ops)
    assert K.same(want, got), _first_difference(want, got)
    return want, lib


def _first_difference(want, got):
    for k, (a, b) in enumerate(zip(want, got)):
        if isinstance(a, np.ndarray):
            if a.tobytes() != b.tobytes():
                return f"op {k}: score {a} != {b}"
            continue
        for q, (x, y) in enumerate(zip(a, b)):
            if not K.same([[x]], [[y]]):
                return f"op {k} query {q}: cand {x['cand']} / {y['cand']}, info {x['info']} / {y['info']}, dense {len(x['dense'])} / {len(y['dense'])}"
    return "lengths differ"


@pytest.mark.parametrize("name", list(K.CASES))
def test_every_output_equals_the_reading(name):
    n_words, ops = K.CASES[name]()
    want, lib = _check(n_words, ops)
    assert any(isinstance(r, list) and any(x["cand"] for x in r) for r in want)
    live = sum(1 for i in lib.db.slots() if i >= 0)
    assert lib.db.size() == (live, len(lib.db.slots()))


@pytest.mark.parametrize("n", [0, 1, _lib.KFDB_STRIP - 1, _lib.KFDB_STRIP, _lib.KFDB_STRIP + 1])
def test_entry_counts_around_a_strip(n):
    _check(*K.strip_case(n))


def test_the_ordered_sum_pair_gives_the_ordered_float():
    n_words, ops, strided = K.ordered_sum_case()
    want, _ = _check(n_words, ops)
    assert want[0][0]["dense"][0][1] != strided and want[1][0] != strided


# ---- raw calls: the caller's arrays filled with sentinels ---------------------------------------------------------------------------
def _database(n_words, ops):
    db = KeyFrameDatabase(n_words)
    for op in ops:
        if op[0] == "add":
            db.add(op[1], op[2], op[3])
        elif op[0] == "covis":
            db.set_covisibles([op[1]], [op[2]])
    return db


def _arrays(Q, n_slots, cap):
    return dict(cand=np.full((Q, cap), SENTINEL, np.int64), n_cand=np.full(Q, SENTINEL, np.int32), info=np.zeros(Q, _lib.KFDB_INFO_DTYPE),
                words=np.full((Q, n_slots), SENTINEL, np.int32), scores=np.full((Q, n_slots), SENTINEL_BITS, np.uint32))


def _inputs(batch, loop):
    off, ids, vals = pack_queries([(q["ids"], q["vals"]) for q in batch])
    if not loop:
        return [off, ids, vals]
    c_off, c_ids = pack_connected([q["connected"] for q in batch])
    return [off, ids, vals, np.array([q["min_score"] for q in batch], np.float32), c_off, c_ids]


def _host(db, batch, loop, cap):
    Q, n = len(batch), db.size()[1]
    a = _arrays(Q, n, cap)
    inp = [_lib.ptr(x) for x in _inputs(batch, loop)]
    f = db._L.orbfe_kfdb_detect_loop if loop else db._L.orbfe_kfdb_detect_relocalization
    _lib.check(f(db._h, Q, *inp, cap, _lib.ptr(a["cand"]), _lib.ptr(a["n_cand"]), _lib.ptr(a["info"]), _lib.ptr(a["words"]),
                 _lib.ptr(a["scores"])), "detect")
    return a


def _device(db, batch, loop, cap):
    import torch
    Q, n = len(batch), db.size()[1]
    a = _arrays(Q, n, cap)
    d_in = [torch.from_numpy(x).cuda() for x in _inputs(batch, loop)]
    d_info = torch.zeros((Q, 32), dtype=torch.uint8, device="cuda")
    d = {k: torch.from_numpy(v.view(np.int32) if k == "scores" else v).cuda() for k, v in a.items() if k != "info"}
    torch.cuda.synchronize()
    f = db.detect_loop_device if loop else db.detect_relocalization_device
    f(Q, *d_in, cap, d["cand"], d["n_cand"], d_info, d["words"], d["scores"])
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out["scores"] = out["scores"].view(np.uint32)
    out["info"] = d_info.cpu().numpy().view(_lib.KFDB_INFO_DTYPE).reshape(Q)
    return out


def _bytes(a, q=None):
    return b"".join((v if q is None else v[q]).tobytes() for _, v in sorted(a.items()))


def _sentinels_survive(a, cap):
    for q in range(len(a["n_cand"])):
        k = min(int(a["n_cand"][q]), cap)
        assert (a["cand"][q, k:] == SENTINEL).all() and (a["cand"][q, :k] >= 0).all()
        untouched = a["words"][q] == SENTINEL
        assert np.array_equal(untouched, a["scores"][q] == SENTINEL_BITS)
        assert (~untouched).sum() == a["info"][q]["n_scored"]


@pytest.fixture(scope="module")
def reloc_scene():
    n_words, ops = K.CASES["reloc_sequence"]()
    return n_words, ops[:-1], ops[-1][1]


@pytest.fixture(scope="module")
def loop_scene():
    n_words, ops = K.CASES["loop_basic"]()
    return n_words, ops[:-1], ops[-1][1]


def test_a_batch_equals_single_calls_in_order_and_the_reversed_order_differs_where_the_reading_does(reloc_scene):
    n_words, ops, batch = reloc_scene
    Q, cap = len(batch), 16
    together = _host(_database(n_words, ops), batch, False, cap)
    twin = _database(n_words, ops)
    singles = [_host(twin, [q], False, cap) for q in batch]
    for q in range(Q):
        assert _bytes(together, q) == _bytes(singles[q], 0), q
    _sentinels_survive(together, cap)
    backwards = _host(_database(n_words, ops), batch[::-1], False, cap)
    fwd = K.run(K.Literal(n_words), ops + [("reloc", batch)])[0]
    rev = K.run(K.Literal(n_words), ops + [("reloc", batch[::-1])])[0]
    differ = 0
    for q in range(Q):
        same_in_reading = K.same([[fwd[q]]], [[rev[Q - 1 - q]]])
        assert (_bytes(together, q) == _bytes(backwards, Q - 1 - q)) == same_in_reading, q
        differ += not same_in_reading
    assert differ > 0


def test_loop_queries_do_not_depend_on_their_position(loop_scene):
    n_words, ops, batch = loop_scene
    db = _database(n_words, ops)
    base = _host(db, batch, True, 16)
    _sentinels_survive(base, 16)
    perm = np.random.default_rng(3).permutation(len(batch))
    moved = _host(db, [batch[i] for i in perm], True, 16)
    for k, i in enumerate(perm):
        assert _bytes(moved, k) == _bytes(base, int(i))
    alone = _host(db, batch[5:6], True, 16)
    assert _bytes(alone, 0) == _bytes(base, 5)


@pytest.mark.parametrize("loop", [False, True])
def test_device_form_equals_host_form_and_cand_cap_truncates_the_list_only(reloc_scene, loop_scene, loop):
    n_words, ops, batch = loop_scene if loop else reloc_scene
    host = _host(_database(n_words, ops), batch, loop, 16)
    dev = _device(_database(n_words, ops), batch, loop, 16)
    assert _bytes(host) == _bytes(dev)
    _sentinels_survive(dev, 16)
    assert host["n_cand"].max() >= 2
    for form in (_host, _device):
        short = form(_database(n_words, ops), batch, loop, 1)
        assert np.array_equal(short["n_cand"], host["n_cand"]) and short["info"].tobytes() == host["info"].tobytes()
        assert np.array_equal(short["cand"][:, 0], host["cand"][:, 0])
        none = form(_database(n_words, ops), batch, loop, 0) if form is _host else None
        assert none is None or np.array_equal(none["n_cand"], host["n_cand"])


def test_two_identical_databases_give_identical_bytes(reloc_scene, loop_scene):
    for (n_words, ops, batch), loop in ((reloc_scene, False), (loop_scene, True)):
        a, b = _host(_database(n_words, ops), batch, loop, 8), _host(_database(n_words, ops), batch, loop, 8)
        assert _bytes(a) == _bytes(b)


def test_score_of_an_unknown_id_is_the_documented_constant():
    db = KeyFrameDatabase(100)
    ids, vals = K.vector(range(10, 30))
    db.add(4, ids, vals)
    db.add(5, *K.vector(range(50, 60)))
    out = db.score(ids, vals, [4, 99, 5, 4])
    assert out[1] == np.float32(_lib.KFDB_SCORE_UNKNOWN) and out[2].tobytes() == np.float32(-0.0).tobytes()
    assert out[0] == out[3] == K.l1_score(ids, vals, ids, vals) and abs(float(out[0]) - 1.0) < 1e-6
    db.erase(4)
    assert db.score(ids, vals, [4])[0] == np.float32(_lib.KFDB_SCORE_UNKNOWN) and db.score(ids, vals, []).shape == (0,)
    assert db.detect_relocalization_candidates(ids, vals) == [] and len(db) == 1


def test_the_measured_alternative_arrangement_gives_the_same_bytes(reloc_scene, loop_scene):
    """orbfe_debug_kfdb_arrangement(1): the common pass scores every pair; host and device forms"""
    L = _lib.lib()
    for (n_words, ops, batch), loop in ((reloc_scene, False), (loop_scene, True)):
        base = _host(_database(n_words, ops), batch, loop, 8)
        try:
            _lib.check(L.orbfe_debug_kfdb_arrangement(1), "orbfe_debug_kfdb_arrangement")
            fused = _host(_database(n_words, ops), batch, loop, 8)
            fused_dev = _device(_database(n_words, ops), batch, loop, 8)
        finally:
            _lib.check(L.orbfe_debug_kfdb_arrangement(0), "orbfe_debug_kfdb_arrangement")
        assert _bytes(base) == _bytes(fused) == _bytes(fused_dev)
    assert L.orbfe_debug_kfdb_arrangement(2) == L.orbfe_debug_kfdb_arrangement(-1) == _lib.ERR_INVALID


def test_every_validation_boundary():
    """what needs a handle: the limits of include/orbfe.h at their last accepted and first refused values, and that a refused call
    changes nothing"""
    L, p = _lib.lib(), _lib.ptr
    n_words = 5000
    db = KeyFrameDatabase(n_words)
    h = db._h
    ids, vals = K.vector(range(0, _lib.KFDB_MAX_WORDS))
    more_ids, more_vals = K.vector(range(0, _lib.KFDB_MAX_WORDS + 1))
    add = lambda kid, i, v, n=None: L.orbfe_kfdb_add(h, kid, p(np.ascontiguousarray(i, np.int32)), p(np.ascontiguousarray(v, np.float64)),
                                                     len(i) if n is None else n)
    assert add(1, ids, vals) == _lib.OK and add(2, more_ids, more_vals) == _lib.ERR_INVALID                    # 4096 / 4097 words
    assert add(3, [], []) == _lib.OK and add(4, [0], [1.0], -1) == _lib.ERR_INVALID                            # 0 / -1 words
    assert add(1, [5], [1.0]) == _lib.ERR_INVALID and add(-1, [5], [1.0]) == _lib.ERR_INVALID                  # live already; id < 0
    assert add(5, [0, n_words - 1], [0.5, 0.5]) == _lib.OK and add(6, [n_words], [1.0]) == _lib.ERR_INVALID    # id range
    assert add(6, [-1], [1.0]) == _lib.ERR_INVALID and add(6, [3, 3], [0.5, 0.5]) == _lib.ERR_INVALID          # ... and order
    assert add(6, [4, 3], [0.5, 0.5]) == _lib.ERR_INVALID
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert add(6, [3], [bad]) == _lib.ERR_INVALID, bad
    assert L.orbfe_kfdb_add(h, 6, None, None, 1) == _lib.ERR_INVALID
    assert db.size() == (3, 3) and db.slots().tolist() == [1, 3, 5]
    assert L.orbfe_kfdb_erase(h, 777) == _lib.OK and db.size() == (3, 3)                                       # unknown: not an error
    row = np.full(10, -1, np.int64)
    one = np.array([1], np.int64)
    assert L.orbfe_kfdb_set_covisibles(h, 1, p(one), p(row)) == _lib.OK and L.orbfe_kfdb_set_covisibles(h, 0, None, None) == _lib.OK
    assert L.orbfe_kfdb_set_covisibles(h, -1, p(one), p(row)) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_set_covisibles(h, 1, None, p(row)) == L.orbfe_kfdb_set_covisibles(h, 1, p(one), None) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_set_covisibles(h, 1, p(np.array([-2], np.int64)), p(row)) == _lib.ERR_INVALID
    out = np.zeros(4, np.float32)
    assert L.orbfe_kfdb_score(h, p(ids), p(vals), len(ids), p(one), 1, p(out)) == _lib.OK
    assert L.orbfe_kfdb_score(h, p(more_ids), p(more_vals), len(more_ids), p(one), 1, p(out)) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_score(h, p(ids), p(vals), len(ids), p(one), -1, p(out)) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_score(h, p(ids), p(vals), len(ids), None, 1, p(out)) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_score(h, p(ids), p(vals), len(ids), p(one), 1, None) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_slots(h, None, 1, None) == L.orbfe_kfdb_slots(h, p(np.zeros(1, np.int64)), -1, None) == _lib.ERR_INVALID

    cand, n_cand = np.zeros(4, np.int64), np.zeros(2, np.int32)
    off = np.array([0, len(ids)], np.int32)

    def reloc(Q=1, off=off, i=ids, v=vals, cap=4, c=cand, n=n_cand):
        return L.orbfe_kfdb_detect_relocalization(h, Q, p(off), p(i), p(v), cap, p(c), p(n), None, None, None)

    assert reloc() == _lib.OK and n_cand[0] == 1 and cand[0] == 1
    assert reloc(Q=0) == _lib.OK and reloc(Q=-1) == _lib.ERR_INVALID and reloc(Q=_lib.KFDB_MAX_QUERIES + 1) == _lib.ERR_INVALID
    assert reloc(off=np.array([0, len(more_ids)], np.int32), i=more_ids, v=more_vals) == _lib.ERR_INVALID
    assert reloc(off=np.array([1, len(ids)], np.int32)) == _lib.ERR_INVALID and reloc(off=np.array([0, -1], np.int32)) == _lib.ERR_INVALID
    assert reloc(off=None) == reloc(i=None) == reloc(v=None) == _lib.ERR_INVALID
    assert reloc(cap=-1) == reloc(c=None) == reloc(n=None) == _lib.ERR_INVALID and reloc(cap=0, c=None) == _lib.OK
    assert reloc(i=np.ascontiguousarray(ids[::-1])) == _lib.ERR_INVALID
    assert reloc(cap=_lib.KFDB_MAX_CELLS + 1) == _lib.ERR_CAPACITY and reloc(cap=4) == _lib.OK

    ms, c_off, c_ids = np.zeros(1, np.float32), np.array([0, 2], np.int32), np.array([3, 5], np.int64)

    def loop(ms=ms, c_off=c_off, c_ids=c_ids):
        return L.orbfe_kfdb_detect_loop(h, 1, p(off), p(ids), p(vals), p(ms), p(c_off), p(c_ids), 4, p(cand), p(n_cand), None, None, None)

    assert loop() == _lib.OK and n_cand[0] == 1 and loop(c_ids=np.array([1, 5], np.int64)) == _lib.OK and n_cand[0] == 0
    for bad in (-1.0, -0.0, float("nan"), float("inf")):
        assert loop(ms=np.array([bad], np.float32)) == _lib.ERR_INVALID, bad
    assert loop(ms=None) == loop(c_off=None) == loop(c_ids=None) == _lib.ERR_INVALID
    assert loop(c_ids=np.array([5, 3], np.int64)) == loop(c_ids=np.array([3, 3], np.int64)) == _lib.ERR_INVALID
    assert loop(c_off=np.array([1, 2], np.int32)) == loop(c_off=np.array([0, -1], np.int32)) == _lib.ERR_INVALID
    assert loop(c_off=np.array([0, 0], np.int32), c_ids=None) == _lib.OK

    import torch
    d = lambda a: torch.from_numpy(a).cuda()
    d_off, d_ids, d_vals, d_cand, d_n = d(off), d(ids), d(vals), d(cand), d(n_cand)
    f = L.orbfe_kfdb_detect_relocalization_device
    assert f(h, 1, p(d_off), p(d_ids), p(d_vals), 4, p(d_cand), p(d_n), None, None, None, None) == _lib.OK
    torch.cuda.synchronize()
    assert d_n.cpu()[0] == 1
    assert f(h, -1, p(d_off), p(d_ids), p(d_vals), 4, p(d_cand), p(d_n), None, None, None, None) == _lib.ERR_INVALID
    assert f(h, 1, None, p(d_ids), p(d_vals), 4, p(d_cand), p(d_n), None, None, None, None) == _lib.ERR_INVALID
    assert f(h, 1, p(d_off), p(d_ids), p(d_vals), 4, None, p(d_n), None, None, None, None) == _lib.ERR_INVALID
    assert f(h, 1, p(d_off), p(d_ids), C.c_void_p(d_vals.data_ptr() + 4), 4, p(d_cand), p(d_n), None, None, None, None) == _lib.ERR_INVALID
    assert f(h, 1, p(d_off), p(d_ids), p(d_vals), _lib.KFDB_MAX_CELLS + 1, p(d_cand), p(d_n), None, None, None, None) == _lib.ERR_CAPACITY
    assert db.size() == (3, 3) and db.detect_relocalization_candidates(ids, vals) == [1]
    db.clear()
    assert db.size() == (0, 0) and db.detect_relocalization_candidates(ids, vals) == [] and add(1, [5], [1.0]) == _lib.OK
