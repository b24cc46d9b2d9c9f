"""Vocabulary training without a device: the two readings of the yardstick (tests/np_vocab_train.py) agree and their trees hold the
invariants of TemplatedVocabulary::create; the draw of the C ABI equals its Python mirror; csrc/vocab_train_internal.h compiled for the
host (tests/cpp_vocabtrain) equals the yardstick's arithmetic on directed values, the retry on a draw of 0 and the pick's
fall-through included; the two writers against the oracle's loader and writer; argument validation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, vocabulary
from tests import np_vocab_train as Y
from tests import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "cpp_vocabtrain", "_build", "libvocabtrain_host.so")
SCENES = Y.scenes()


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_vocabtrain")], check=True, capture_output=True)
    h = C.CDLL(HOST_LIB)
    h.vt_host_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32]; h.vt_host_draw.restype = C.c_uint32
    h.vt_host_first_index.argtypes = [C.c_uint32, C.c_int]
    h.vt_host_cut.argtypes = [C.c_uint32, C.c_int64]; h.vt_host_cut.restype = C.c_double
    h.vt_host_cut_target.argtypes = [C.c_double]; h.vt_host_cut_target.restype = C.c_int64
    h.vt_host_pick.argtypes = [C.c_void_p, C.c_int, C.c_double]
    h.vt_host_majority.argtypes = [C.c_int]
    h.vt_host_hamming.argtypes = [C.c_void_p, C.c_void_p]
    h.vt_host_cut_retry.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int)]; h.vt_host_cut_retry.restype = C.c_double
    h.vt_host_cut_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_int64]; h.vt_host_cut_draw.restype = C.c_double
    return h


@pytest.fixture(scope="module")
def trained():
    """name -> (literal, level order), each computed once"""
    return {name: (Y.train_literal(imgs, k, Lv), Y.train_level_order(imgs, k, Lv)) for name, (k, Lv, imgs) in SCENES.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_two_readings_agree(trained, name):
    (ta, la, sa), (tb, lb, sb) = trained[name]
    for f in ("parent", "is_leaf", "desc"):
        assert np.array_equal(ta[f], tb[f]), f
    assert ta["weight"].tobytes() == tb["weight"].tobytes()
    assert np.array_equal(la, lb) and sa == sb
    assert sa["n_capped_nodes"] == 0


def test_the_scenes_reach_what_they_are_meant_to(trained):
    s = {n: trained[n][1][2] for n in SCENES}
    assert s["a"]["n_empty_clusters"] == 0 and s["b"]["n_empty_clusters"] == 0
    assert s["c"]["n_trivial_nodes"] > 0 and s["c"]["n_short_seedings"] > 0
    assert s["c"]["nodes_per_level"][4] > 0 and sum(trained["c"][1][0]["is_leaf"]) > s["c"]["nodes_per_level"][4]   # leaves above level L
    assert s["d"]["n_empty_clusters"] > 0
    assert s["e"]["n_short_seedings"] > 0 and s["e"]["nodes_per_level"][1] == 3
    assert s["h"]["n_trivial_nodes"] == 1 and s["h"]["n_nodes"] == 8
    assert s["i"]["n_nodes"] == 2 and s["i"]["n_words"] == 1
    assert s["j"]["n_words"] > 32 and s["k"]["n_words"] > 32 and len(SCENES["k"][2]) > 128   # more words than descriptors


@pytest.mark.parametrize("name", sorted(SCENES))
def test_tree_invariants(trained, name):
    k, Lv, imgs = SCENES[name]
    tree, leaf_node, stats = trained[name][0]
    parent, is_leaf, desc = tree["parent"], tree["is_leaf"], tree["desc"]
    n = len(parent)
    assert all(parent[i] < i for i in range(1, n))                # every child id is greater than its parent's
    children = Y._children_of(parent)
    for ch in children:
        assert ch == list(range(ch[0], ch[0] + len(ch))) if ch else True   # children of a node are consecutive
        assert len(ch) <= k
    assert all((not children[i]) == bool(is_leaf[i]) for i in range(1, n))
    # a feature's transform word is the leaf of its group, unless an earlier sibling holds an identical descriptor (a trivial node)
    D = np.concatenate(imgs, 0)
    for i in range(0, len(D), max(1, len(D) // 400)):
        got = Y._descend(children, desc, D[i])
        if got != leaf_node[i]:
            assert parent[got] == parent[leaf_node[i]] and got < leaf_node[i] and np.array_equal(desc[got], desc[leaf_node[i]])
    # weights: log(NDocs / Ni) on the words, 0 on inner nodes
    assert all(tree["weight"][i] == 0.0 for i in range(n) if not is_leaf[i])


def test_draw_equals_the_c_export_and_known_answers(L):
    rng = np.random.default_rng(5)
    for _ in range(3000):
        seed, level, path, j = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 12)), int(rng.integers(0, 20 ** 10)), int(rng.integers(0, 2 ** 32))
        r = vocabulary.training_draw(seed, level, path, j)
        assert 0 <= r <= Y.RAND_MAX and r == L.orbfe_vocabulary_training_draw(seed, level, path, j)
    known = {(0, 1, 0, 0): 1759515523, (0, 1, 0, 1): 203018750, (1, 1, 0, 0): 1689447194, (7, 3, 42, 5): 1858129767,
             (2 ** 64 - 1, 10, 20 ** 10 - 1, 2 ** 32 - 1): 1360876636, (123456789, 6, 99999, 17): 1847777470}
    for a, v in known.items():
        assert vocabulary.training_draw(*a) == v == L.orbfe_vocabulary_training_draw(*a)
    assert vocabulary._splitmix64(0) == 0xE220A8397B1DCDAF      # the first output of the published splitmix64 from state 0


def test_header_arithmetic_on_the_host(H):
    rng = np.random.default_rng(6)
    for a in [(0, 1, 0, 0), (7, 3, 42, 5), (2 ** 64 - 1, 10, 20 ** 10 - 1, 2 ** 32 - 1)]:
        assert H.vt_host_draw(*a) == vocabulary.training_draw(*a)
    # the first centre: the ends of the range of r and sizes up to the limit
    for r in (0, 1, 2 ** 30, Y.RAND_MAX - 1, Y.RAND_MAX, 1759515523):
        for n in (1, 2, 3, 7, 1000, 6400, 2 ** 20 + 1, 2 ** 30):
            i = H.vt_host_first_index(r, n)
            assert i == Y.first_index(r, n) and 0 <= i < n
    # the cut and its integer target
    for r in (0, 1, 5, 2 ** 30, Y.RAND_MAX - 1, Y.RAND_MAX):
        for s in (1, 2, 255, 256, 10 ** 6 + 7, 2 ** 38 - 1):
            cut = H.vt_host_cut(r, s)
            assert cut == Y.cut_value(r, s)
            assert H.vt_host_cut_target(cut) == int(np.ceil(cut))
    assert H.vt_host_cut(0, 12345) == 0.0 and H.vt_host_cut(Y.RAND_MAX, 12345) == 12345.0
    # a draw of 0 gives a cut of 0.0 and is drawn again
    draws = np.array([0, 0, 77, 5], np.uint32); used = C.c_int(0)
    cut = H.vt_host_cut_retry(draws.ctypes.data, 999, C.byref(used))
    seq = iter(draws.tolist())
    ycut, yj = Y.cut_draw(0, 1, 0, 0, 999, draw=lambda *_: next(seq))
    assert used.value == 3 == yj and cut == ycut == Y.cut_value(77, 999)
    j = C.c_uint32(4)
    cut = H.vt_host_cut_draw(9, 2, 3, C.byref(j), 5000)
    ycut, yj = Y.cut_draw(9, 2, 3, 4, 5000)
    assert cut == ycut and j.value == yj
    # the pick: first index whose running sum reaches the cut; zeros never win; none qualifies -> the last index
    for _ in range(200):
        n = int(rng.integers(1, 60))
        md = rng.integers(0, 257, n).astype(np.int32) * (rng.random(n) < 0.7)
        md = md.astype(np.int32)
        total = int(md.sum())
        if total == 0:
            continue
        for cut in (0.5, 1.0, float(total), total - 0.5, float(rng.uniform(0, total)), Y.cut_value(int(rng.integers(1, 2 ** 31)), total)):
            if cut <= 0:
                continue
            assert H.vt_host_pick(md.ctypes.data, n, cut) == Y.pick(md.tolist(), cut)
    md = np.array([3, 0, 4, 0], np.int32)
    assert H.vt_host_pick(md.ctypes.data, 4, 7.0) == 2 and H.vt_host_pick(md.ctypes.data, 4, 3.0) == 0 and H.vt_host_pick(md.ctypes.data, 4, 3.5) == 2
    assert H.vt_host_pick(md.ctypes.data, 4, 7.5) == 3 == Y.pick(md.tolist(), 7.5)          # the fall-through
    # the majority threshold and the distance
    for n in range(1, 40):
        assert H.vt_host_majority(n) == Y.majority(n) == (n + 1) // 2
    for _ in range(100):
        a, b = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
        assert H.vt_host_hamming(a.ctypes.data, b.ctypes.data) == Y.hamming(a, b) == ol.descriptor_distance(a, b)
    assert H.vt_host_chunk() == _lib.VOCAB_TRAIN_CHUNK


def test_writers(L, trained, tmp_path):
    for name in ("a", "c", "h"):
        k, Lv, imgs = SCENES[name]
        tree = trained[name][0][0]
        args = (k, Lv, tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"])
        mine, theirs = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}_oracle.bin")
        vocabulary.write_binary(mine, *args, scoring=1, weighting=2)
        ol.write_vocabulary_binary(theirs, *args, scoring=1, weighting=2)
        assert open(mine, "rb").read() == open(theirs, "rb").read()
        txt = str(tmp_path / f"{name}.txt")
        vocabulary.write_text(txt, *args)
        v = ol.OracleVocabulary.load_text(txt)
        ref = ol.OracleVocabulary.from_arrays(*args)
        assert v.info() == ref.info() == (len(tree["parent"]), int(tree["is_leaf"].sum()))
        D = np.concatenate(imgs, 0)[:300]
        (bow, fv, (w, nd, wt)), (rbow, rfv, (rw, rnd, rwt)) = v.transform(D, 1), ref.transform(D, 1)
        assert bow == rbow and fv == rfv and np.array_equal(w, rw) and np.array_equal(nd, rnd)
        assert wt.tobytes() == rwt.tobytes()                      # the weights come back as the same doubles
        words = np.flatnonzero(tree["is_leaf"])
        assert wt.tobytes() == tree["weight"][words[w]].tobytes()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def _train(L, cfg, desc, start, n_images):
    h = C.c_void_p(None)
    rc = L.orbfe_vocabulary_train(C.byref(cfg) if cfg is not None else None, _lib.ptr(desc), _lib.ptr(start), n_images, -1, None, None, C.byref(h))
    if h.value:
        L.orbfe_vocabulary_destroy(h)
    return rc


def test_argument_validation(L):
    d = np.zeros((8, 32), np.uint8); start = np.array([0, 3, 8], np.int32)
    ok = lambda **kw: _lib.VocabTrainConfig(**{**dict(k=3, L=2, scoring=0, weighting=0, seed=0, max_iterations=0, wide_min=0), **kw})
    for bad in (dict(k=1), dict(k=21), dict(L=0), dict(L=11), dict(scoring=-1), dict(scoring=6), dict(weighting=-1), dict(weighting=4)):
        assert _train(L, ok(**bad), d, start, 2) == _lib.ERR_INVALID, bad
        assert L.orbfe_last_error()
    assert _train(L, ok(), d, np.array([0, 0, 0], np.int32), 2) == _lib.ERR_INVALID          # n_desc < 1
    assert _train(L, ok(), d, start, 0) == _lib.ERR_INVALID                                  # n_images < 1
    assert _train(L, ok(), d, np.array([0, 5, 3], np.int32), 2) == _lib.ERR_INVALID          # not monotone
    assert _train(L, ok(), d, np.array([0, 2 ** 30 + 1], np.int32), 1) == _lib.ERR_INVALID   # more than 2^30 descriptors
    assert _train(L, None, d, start, 2) == _lib.ERR_INVALID
    assert _train(L, ok(), None, start, 2) == _lib.ERR_INVALID and _train(L, ok(), d, None, 2) == _lib.ERR_INVALID
    assert L.orbfe_vocabulary_train(C.byref(ok()), _lib.ptr(d), _lib.ptr(start), 2, -1, None, None, None) == _lib.ERR_INVALID
    need = C.c_size_t(0)
    assert L.orbfe_vocabulary_train_workspace_bytes(C.byref(ok()), 1000, 4, C.byref(need)) == _lib.OK and need.value > 1000 * 32
    assert L.orbfe_vocabulary_train_workspace_bytes(C.byref(ok(k=1)), 1000, 4, C.byref(need)) == _lib.ERR_INVALID
    assert L.orbfe_vocabulary_train_workspace_bytes(C.byref(ok()), 0, 4, C.byref(need)) == _lib.ERR_INVALID
    # the device form: a workspace smaller than asked for, null pointers (nothing is dereferenced before the device is looked for)
    h = C.c_void_p(None); fake = C.c_void_p(0x10000)
    dev = lambda cfg, dd, dn, ws, nbytes: L.orbfe_vocabulary_train_device(C.byref(cfg), dd, dn, 2, 4, ws, nbytes, None, None, None, C.byref(h))
    assert dev(ok(), fake, fake, fake, 16) == _lib.ERR_INVALID and b"workspace" in L.orbfe_last_error()
    assert dev(ok(), None, fake, fake, 1 << 30) == _lib.ERR_INVALID and dev(ok(), fake, None, fake, 1 << 30) == _lib.ERR_INVALID
    assert dev(ok(), fake, fake, None, 1 << 30) == _lib.ERR_INVALID and dev(ok(k=30), fake, fake, fake, 1 << 30) == _lib.ERR_INVALID
    # the writers
    p = np.zeros(2, np.int32); lf = np.array([0, 1], np.uint8); w = np.zeros(2)
    assert L.orbfe_vocabulary_write_text(None, 2, 1, 0, 0, 2, _lib.ptr(p), _lib.ptr(lf), _lib.ptr(d), _lib.ptr(w)) == _lib.ERR_INVALID
    assert L.orbfe_vocabulary_write_binary(b"/nonexistent-directory/x.bin", 2, 1, 0, 0, 2, _lib.ptr(p), _lib.ptr(lf), _lib.ptr(d), _lib.ptr(w)) == _lib.ERR_INVALID
    assert L.orbfe_vocabulary_save_text(None, b"x") == _lib.ERR_INVALID and L.orbfe_vocabulary_nodes(None, None, None, None, None) == _lib.ERR_INVALID


def test_no_device_is_an_error(L):
    if _gpu_present(L):
        pytest.skip("a GPU is present")
    d = np.zeros((8, 32), np.uint8); start = np.array([0, 3, 8], np.int32)
    cfg = _lib.VocabTrainConfig(3, 2, 0, 0, 0, 0, 0)
    assert _train(L, cfg, d, start, 2) == _lib.ERR_NO_DEVICE and b"no CPU fallback" in L.orbfe_last_error()
    h = C.c_void_p(None); fake = C.c_void_p(0x10000)
    assert L.orbfe_vocabulary_train_device(C.byref(cfg), fake, fake, 2, 4, fake, 1 << 30, None, None, None, C.byref(h)) == _lib.ERR_NO_DEVICE
    with pytest.raises(_lib.OrbfeError):
        vocabulary.ORBVocabulary.create([d[:3], d[3:]], 3, 2)
