"""Vocabulary training on the device (include/orbfe.h: orbfe_vocabulary_train) against the yardstick (tests/np_vocab_train.py): the
exported tree, the per-feature leaf and the statistics equal the level-order reading on every scene; the wide and the narrow form give
the same bytes; the device form equals the host form; the trained handle serves Frame::ComputeBoW at once and its weights are
log(NDocs / Ni) of the C oracle's descent; the saved files load; the example runs."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from refactored_orb_slam2_amd.vocabulary import ORBVocabulary
from tests import np_vocab_train as Y
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = Y.scenes()
_REF = {}


def reference(name):
    """the yardstick of a scene, computed once and left unchanged"""
    if name not in _REF:
        k, L, imgs = SCENES[name]
        _REF[name] = Y.train_level_order(imgs, k, L)
    return _REF[name]


def same_tree(got, tree):
    parent, leaf, desc, weight = got
    assert np.array_equal(parent, tree["parent"]) and np.array_equal(leaf, tree["is_leaf"])
    assert np.array_equal(desc, tree["desc"])
    assert len(weight) == len(tree["weight"]) and all(a == b for a, b in zip(weight.tolist(), tree["weight"].tolist()))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_tree_equals_the_yardstick(name):
    k, L, imgs = SCENES[name]
    tree, leaf_node, stats = reference(name)
    v = ORBVocabulary.create(imgs, k, L, return_leaf_nodes=True)
    print(name, v.train_stats)
    same_tree(v.nodes(), tree)
    assert np.array_equal(v.leaf_nodes, leaf_node)
    assert v.train_stats == stats
    assert v.info() == (k, L, stats["n_nodes"], stats["n_words"])
    assert v.train_stats["n_capped_nodes"] == 0
    if name in ("a", "b"):
        assert v.train_stats["n_empty_clusters"] == 0
    if name == "c":
        assert v.train_stats["n_trivial_nodes"] > 0 and v.train_stats["n_short_seedings"] > 0
    if name == "d":
        assert v.train_stats["n_empty_clusters"] > 0
    if name == "e":
        assert v.train_stats["n_short_seedings"] > 0
    if name in ("j", "k"):
        assert v.train_stats["n_words"] > sum(len(i) for i in imgs)     # words that no feature reaches


@pytest.mark.parametrize("weighting", [Y.TF, Y.IDF, Y.BINARY])
def test_other_weightings(weighting):
    k, L, imgs = SCENES["c"]
    tree, _, _ = Y.train_level_order(imgs, k, L, weighting=weighting)
    same_tree(ORBVocabulary.create(imgs, k, L, weighting=weighting).nodes(), tree)


def test_seed_changes_the_tree_and_equals_the_yardstick():
    k, L, imgs = SCENES["a"]
    tree, leaf_node, stats = Y.train_level_order(imgs, k, L, seed=987654321987)
    v = ORBVocabulary.create(imgs, k, L, seed=987654321987, return_leaf_nodes=True)
    same_tree(v.nodes(), tree)
    assert np.array_equal(v.leaf_nodes, leaf_node) and v.train_stats == stats
    assert not np.array_equal(tree["desc"], reference("a")[0]["desc"])


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_wide_and_narrow_forms_give_identical_bytes(name):
    k, L, imgs = SCENES[name]
    out = []
    for wide_min in (1, 300, 0, 2 ** 30):      # 0 and 2^30 both mean 1 025; 300 moves the border into the second level
        v = ORBVocabulary.create(imgs, k, L, wide_min=wide_min, return_leaf_nodes=True)
        forms = v.train_levels()
        if wide_min == 1:
            assert all(lv["narrow"] == 0 for lv in forms) and sum(lv["wide"] for lv in forms) == v.train_stats["n_kmeans_nodes"]
        else:
            assert forms[0]["wide"] == 1 and sum(lv["narrow"] for lv in forms) > 0       # the root is beyond one workgroup
        out.append(b"".join(a.tobytes() for a in v.nodes()) + v.leaf_nodes.tobytes() + repr(v.train_stats).encode())
    assert out[0] == out[1] == out[2] == out[3]
    tree, leaf_node, _ = reference(name)
    assert out[0].startswith(tree["parent"].tobytes() + tree["is_leaf"].tobytes() + tree["desc"].tobytes() + tree["weight"].tobytes())


def test_device_form_equals_host_form():
    import torch
    imgs = Y.scene(31, 12, 60, ragged=True, empty=(4,))
    k, L = 5, 3
    host = ORBVocabulary.create(imgs, k, L, return_leaf_nodes=True)
    cap = max(len(i) for i in imgs) + 7
    rng = np.random.default_rng(3)
    d = rng.integers(0, 256, (len(imgs), cap, 32), dtype=np.uint8)      # garbage behind each count
    for f, im in enumerate(imgs):
        d[f, :len(im)] = im
    cnt = np.array([len(i) for i in imgs], np.int32)
    dev = ORBVocabulary.create((torch.from_numpy(d).cuda(), torch.from_numpy(cnt).cuda()), k, L, return_leaf_nodes=True)
    for a, b in zip(host.nodes(), dev.nodes()):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(dev.leaf_nodes.cpu().numpy(), host.leaf_nodes) and dev.train_stats == host.train_stats
    tree, leaf_node, stats = Y.train_level_order(imgs, k, L)
    same_tree(host.nodes(), tree)
    assert np.array_equal(host.leaf_nodes, leaf_node) and host.train_stats == stats


def test_trained_handle_serves_compute_bow_and_weights_are_idf(tmp_path):
    k, L, imgs = SCENES["b"]
    v = ORBVocabulary.create(imgs, k, L)
    parent, leaf, desc, weight = v.nodes()
    orc = ol.OracleVocabulary.from_arrays(k, L, parent, leaf, desc, weight)
    words = np.flatnonzero(leaf)
    ni = np.zeros(len(words), np.int64)
    for f, im in enumerate(imgs):
        bow, fv, (w, nd, wt) = orc.transform(im, 2)
        if f < 6:   # the handle goes straight into Frame::ComputeBoW
            gbow, gfv, (gw, gnd, gwt) = v.transform(im, 2)
            assert gbow == bow and gfv == fv and np.array_equal(gw, w) and np.array_equal(gnd, nd) and gwt.tobytes() == wt.tobytes()
        ni[np.unique(w)] += 1
    for wi, node in enumerate(words):
        assert weight[node] == (math.log(len(imgs) / ni[wi]) if ni[wi] > 0 else 0.0)
    assert all(weight[i] == 0.0 for i in range(len(parent)) if not leaf[i])
    # save_text -> loadFromTextFile -> the same transform; save_binary bytes = the oracle writer's
    txt, bn, obn = str(tmp_path / "v.txt"), str(tmp_path / "v.bin"), str(tmp_path / "o.bin")
    v.saveToTextFile(txt); v.saveToBinaryFile(bn)
    ol.write_vocabulary_binary(obn, k, L, parent, leaf, desc, weight)
    assert open(bn, "rb").read() == open(obn, "rb").read()
    v2 = ORBVocabulary()
    assert v2.loadFromTextFile(txt) and v2.info() == v.info()
    for a, b in zip(v2.nodes(), v.nodes()):
        assert a.tobytes() == b.tobytes()
    a, b = v2.transform(imgs[7], 2), v.transform(imgs[7], 2)
    assert a[0] == b[0] and a[1] == b[1] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2]))


def test_example_trains_and_its_file_loads(tmp_path):
    out = str(tmp_path / "synthetic.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_vocabulary.py"), "--synthetic", "8", "--width", "320", "--height",
                        "240", "--features", "300", "-k", "6", "-L", "3", "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "level 1" in r.stdout
    v = ORBVocabulary()
    assert v.loadFromTextFile(out)
    k, L, n_nodes, n_words = v.info()
    assert (k, L) == (6, 3) and n_words > 6 and n_nodes > n_words
    orc = ol.OracleVocabulary.load_text(out)
    assert orc.info() == (n_nodes, n_words)
    # the same frames as PNG files in a directory give the same file
    import struct, zlib
    from refactored_orb_slam2_amd import synth
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    os.mkdir(tmp_path / "png")
    for i in range(8):
        img = synth.frame(320, 240, seq=0, f=i)
        raw = b"".join(b"\x00" + img[y].tobytes() for y in range(240))
        with open(tmp_path / "png" / f"{i:04d}.png", "wb") as f:
            f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 320, 240, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) +
                    chunk(b"IEND", b""))
    out2 = str(tmp_path / "from_png.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_vocabulary.py"), str(tmp_path / "png"), "--features", "300",
                        "-k", "6", "-L", "3", "--out", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert open(out2, "rb").read() == open(out, "rb").read()
