"""Host-side mirror of ORB_SLAM2::ORBVocabulary (Source/Libraries/ORB_SLAM2/include/ORBVocabulary.h) for the part
the front end needs: loading the text format and ``transform(descriptors, BowVector, FeatureVector, levelsup)``
(Frame::ComputeBoW, Source/Libraries/ORB_SLAM2/src/Frame.cc:412-417).  The tree descent runs on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def training_draw(seed: int, level: int, path: int, j: int) -> int:
    """The 31-bit draw j of the node (level, path) of a training run: the mirror of orbfe_vocabulary_training_draw
    (csrc/vocab_train_internal.h: vt_draw)."""
    h = _splitmix64(seed & _M64)
    h = _splitmix64(h ^ (level & 0xFFFFFFFF))
    h = _splitmix64(h ^ (path & _M64))
    return _splitmix64(h ^ (j & 0xFFFFFFFF)) >> 33


def _tree_arrays(parent, is_leaf, desc, weight):
    return (np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(is_leaf, np.uint8),
            np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), np.ascontiguousarray(weight, np.float64))


def write_text(filename, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
    """ORBVocabulary::saveToTextFile of a tree given as arrays; the weight is written so that it reads back as the same double."""
    p, l, d, w = _tree_arrays(parent, is_leaf, desc, weight)
    _lib.check(_lib.lib().orbfe_vocabulary_write_text(str(filename).encode(), k, L, scoring, weighting, len(p), _lib.ptr(p), _lib.ptr(l),
                                                      _lib.ptr(d), _lib.ptr(w)), "orbfe_vocabulary_write_text")


def write_binary(filename, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
    """ORBVocabulary::saveToBinaryFile of a tree given as arrays, byte for byte."""
    p, l, d, w = _tree_arrays(parent, is_leaf, desc, weight)
    _lib.check(_lib.lib().orbfe_vocabulary_write_binary(str(filename).encode(), k, L, scoring, weighting, len(p), _lib.ptr(p), _lib.ptr(l),
                                                        _lib.ptr(d), _lib.ptr(w)), "orbfe_vocabulary_write_binary")


class ORBVocabulary:
    def __init__(self):
        self._L = _lib.lib()
        self._h = C.c_void_p(None)
        self.train_stats = None
        self.leaf_nodes = None

    @classmethod
    def create(cls, training_features, k, L, weighting=0, scoring=0, seed=0, wide_min=0, return_leaf_nodes=False, max_iterations=0,
               device=-1):
        """DBoW2::TemplatedVocabulary::create on the device (include/orbfe.h: orbfe_vocabulary_train).  training_features: a list of
        (n_i, 32) uint8 arrays, one per image, or a pair (descriptors, counts) of device tensors (F, cap, 32) uint8 and (F,) int32 as
        orbfe_extract_batch_device leaves them.  The statistics are in .train_stats; with return_leaf_nodes the node of the deepest
        group of every training feature is in .leaf_nodes (a numpy array, or a device tensor for device input)."""
        v = cls()
        cfg = _lib.VocabTrainConfig(k, L, scoring, weighting, seed, max_iterations, wide_min)
        stats = np.zeros(1, _lib.VOCAB_TRAIN_STATS_DTYPE)
        if isinstance(training_features, tuple) and not isinstance(training_features[0], np.ndarray):
            import torch
            d, cnt = training_features
            if d.dtype != torch.uint8 or d.dim() != 3 or d.shape[2] != 32 or not d.is_contiguous():
                raise ValueError("descriptors must be a contiguous (F, cap, 32) uint8 device tensor")
            cnt = cnt.to(torch.int32).contiguous()
            n_frames, cap = int(d.shape[0]), int(d.shape[1])
            need = C.c_size_t(0)
            _lib.check(v._L.orbfe_vocabulary_train_workspace_bytes(C.byref(cfg), max(n_frames * cap, 1), n_frames, C.byref(need)),
                       "orbfe_vocabulary_train_workspace_bytes")
            ws = torch.empty(need.value + 256, dtype=torch.uint8, device=d.device)
            off = (-ws.data_ptr()) % 256
            leaf = torch.zeros(max(n_frames * cap, 1), dtype=torch.int32, device=d.device) if return_leaf_nodes else None
            torch.cuda.synchronize(d.device)
            _lib.check(v._L.orbfe_vocabulary_train_device(C.byref(cfg), _lib.ptr(d), _lib.ptr(cnt), n_frames, cap,
                                                          C.c_void_p(ws.data_ptr() + off), need.value, _lib.ptr(leaf), None,
                                                          _lib.ptr(stats), C.byref(v._h)), "orbfe_vocabulary_train_device")
            if leaf is not None:
                v.leaf_nodes = leaf[: int(cnt.sum().item())]
        else:
            imgs = [np.ascontiguousarray(f, np.uint8).reshape(-1, 32) for f in training_features]
            start = np.zeros(len(imgs) + 1, np.int32)
            if imgs:
                start[1:] = np.cumsum([len(f) for f in imgs])
            d = np.ascontiguousarray(np.concatenate(imgs, 0) if imgs else np.zeros((0, 32), np.uint8))
            leaf = np.zeros(max(len(d), 1), np.int32) if return_leaf_nodes else None
            _lib.check(v._L.orbfe_vocabulary_train(C.byref(cfg), _lib.ptr(d), _lib.ptr(start), len(imgs), device, _lib.ptr(leaf),
                                                   _lib.ptr(stats), C.byref(v._h)), "orbfe_vocabulary_train")
            if leaf is not None:
                v.leaf_nodes = leaf[: len(d)]
        s = stats[0]
        v.train_stats = {n: (s[n].tolist() if n == "nodes_per_level" else int(s[n])) for n in stats.dtype.names}
        return v

    def train_levels(self):
        """Per level of this thread's last create(): (milliseconds, rounds, wide, narrow and trivial segments)."""
        ms = np.zeros(10, np.float64)
        r, w, nr, tr = (np.zeros(10, np.int32) for _ in range(4))
        n = C.c_int(0)
        _lib.check(self._L.orbfe_debug_vocabulary_train_levels(10, _lib.ptr(ms), _lib.ptr(r), _lib.ptr(w), _lib.ptr(nr), _lib.ptr(tr),
                                                               C.byref(n)), "orbfe_debug_vocabulary_train_levels")
        return [dict(level=i + 1, ms=float(ms[i]), rounds=int(r[i]), wide=int(w[i]), narrow=int(nr[i]), trivial=int(tr[i]))
                for i in range(n.value)]

    def nodes(self):
        """The tree in the layout from_arrays takes: (parent, is_leaf, desc, weight)."""
        n = self.info()[2]
        parent = np.zeros(n, np.int32); leaf = np.zeros(n, np.uint8); desc = np.zeros((n, 32), np.uint8); weight = np.zeros(n, np.float64)
        _lib.check(self._L.orbfe_vocabulary_nodes(self._h, _lib.ptr(parent), _lib.ptr(leaf), _lib.ptr(desc), _lib.ptr(weight)),
                   "orbfe_vocabulary_nodes")
        return parent, leaf, desc, weight

    def saveToTextFile(self, filename: str):
        _lib.check(self._L.orbfe_vocabulary_save_text(self._h, str(filename).encode()), "orbfe_vocabulary_save_text")

    def saveToBinaryFile(self, filename: str):
        _lib.check(self._L.orbfe_vocabulary_save_binary(self._h, str(filename).encode()), "orbfe_vocabulary_save_binary")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbfe_vocabulary_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def loadFromTextFile(self, filename: str, device: int = -1) -> bool:
        self.close()
        rc = self._L.orbfe_vocabulary_load_text(filename.encode(), device, C.byref(self._h))
        if rc == _lib.ERR_INVALID:
            return False  # the reference returns false on a malformed file
        _lib.check(rc, "orbfe_vocabulary_load_text")
        return True

    def loadFromBinaryFile(self, filename: str, device: int = -1) -> bool:
        """ORBVocabulary::loadFromBinaryFile (ORBVocabulary.cc:152-213)"""
        self.close()
        rc = self._L.orbfe_vocabulary_load_binary(filename.encode(), device, C.byref(self._h))
        if rc == _lib.ERR_INVALID:
            return False
        _lib.check(rc, "orbfe_vocabulary_load_binary")
        return True

    @classmethod
    def from_arrays(cls, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0, device=-1):
        v = cls()
        parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8); weight = np.ascontiguousarray(weight, np.float64)
        _lib.check(v._L.orbfe_vocabulary_create(k, L, scoring, weighting, len(parent), _lib.ptr(parent), _lib.ptr(is_leaf),
                                                _lib.ptr(desc), _lib.ptr(weight), device, C.byref(v._h)), "orbfe_vocabulary_create")
        return v

    def info(self):
        k, L, n, w = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._L.orbfe_vocabulary_info(self._h, C.byref(k), C.byref(L), C.byref(n), C.byref(w)), "orbfe_vocabulary_info")
        return k.value, L.value, n.value, w.value

    def transform(self, descriptors, levelsup: int = 4):
        """Returns (BowVector {word: value}, FeatureVector {node: [indices]}, per-feature (word, node, weight))."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        word = np.zeros(n, np.int32); node = np.zeros(n, np.int32); weight = np.zeros(n, np.float64)
        bow_ids = np.zeros(max(n, 1), np.int32); bow_vals = np.zeros(max(n, 1), np.float64)
        fv_nodes = (_lib.FeatVecNode * max(n, 1))()
        fv_idx = np.zeros(max(n, 1), np.int32)
        nb, nf = C.c_int(0), C.c_int(0)
        _lib.check(self._L.orbfe_compute_bow(self._h, _lib.ptr(d), n, levelsup, _lib.ptr(word), _lib.ptr(node), _lib.ptr(weight),
                                             _lib.ptr(bow_ids), _lib.ptr(bow_vals), C.byref(nb), C.cast(fv_nodes, C.c_void_p),
                                             _lib.ptr(fv_idx), C.byref(nf)), "orbfe_compute_bow")
        bow = {int(bow_ids[i]): float(bow_vals[i]) for i in range(nb.value)}
        fv = {int(fv_nodes[i].node_id): fv_idx[fv_nodes[i].start: fv_nodes[i].start + fv_nodes[i].count].tolist()
              for i in range(nf.value)}
        return bow, fv, (word, node, weight)
