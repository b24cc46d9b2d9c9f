"""KeyFrameDatabase on the device (include/orbfe.h: orbfe_kfdb_*): the BoW vectors of the map's keyframes in HBM, and
DetectRelocalizationCandidates / DetectLoopCandidates for one query or a batch.  Every output equals a plain reading of the reference
bit for bit (the header states the reading); there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import KFDB_INFO_DTYPE, KFDB_NEIGHBOURS, check, ptr


class Detection(NamedTuple):
    candidates: list            # per query: int64 ids in the reference's order (the first min(n_cand, cand_cap))
    n_cand: np.ndarray          # [Q] full counts
    info: np.ndarray            # [Q] KFDB_INFO_DTYPE
    common_words: Optional[np.ndarray]   # [Q][n_slots], -1 where the slot was not scored (dense=True)
    scores: Optional[np.ndarray]         # [Q][n_slots] float32, NaN where the slot was not scored (dense=True)


def pack_queries(queries: Sequence):
    """[(ids, vals), ...] -> CSR (offsets int32 [Q + 1], ids int32, vals float64)"""
    off = np.zeros(len(queries) + 1, np.int32)
    for k, (ids, _) in enumerate(queries):
        off[k + 1] = off[k] + len(ids)
    ids = np.concatenate([np.asarray(q[0], np.int32) for q in queries]) if queries else np.zeros(0, np.int32)
    vals = np.concatenate([np.asarray(q[1], np.float64) for q in queries]) if queries else np.zeros(0, np.float64)
    return off, np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)


def pack_connected(connected: Sequence):
    """per query the connected keyframe ids -> CSR (offsets int32 [Q + 1], ids int64 ascending)"""
    off = np.zeros(len(connected) + 1, np.int32)
    rows = [np.unique(np.asarray(c, np.int64)) for c in connected]
    for k, r in enumerate(rows):
        off[k + 1] = off[k] + len(r)
    return off, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, np.int64), np.int64)


class KeyFrameDatabase:
    def __init__(self, n_words: int, device: int = 0, scoring: int = _lib.KFDB_L1_NORM):
        self._L = _lib.lib()
        self._h = C.c_void_p(None)
        check(self._L.orbfe_kfdb_create(int(n_words), int(scoring), int(device), C.byref(self._h)), "orbfe_kfdb_create")
        self.n_words = int(n_words)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.orbfe_kfdb_destroy(self._h)
            self._h = C.c_void_p(None)

    __del__ = close

    # ---- entries -----------------------------------------------------------------------------------------------------------------
    def add(self, kf_id: int, ids, vals) -> None:
        ids, vals = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)
        if ids.shape != vals.shape or ids.ndim != 1:
            raise ValueError("ids and vals are 1-d arrays of one length")
        check(self._L.orbfe_kfdb_add(self._h, int(kf_id), ptr(ids), ptr(vals), len(ids)), "orbfe_kfdb_add")

    def erase(self, kf_id: int) -> None:
        check(self._L.orbfe_kfdb_erase(self._h, int(kf_id)), "orbfe_kfdb_erase")

    def clear(self) -> None:
        check(self._L.orbfe_kfdb_clear(self._h), "orbfe_kfdb_clear")

    def set_covisibles(self, kf_ids, rows) -> None:
        """rows[k] = GetBestCovisibilityKeyFrames(10) of kf_ids[k], in its order; shorter rows are padded with -1"""
        kf_ids = np.ascontiguousarray(np.atleast_1d(kf_ids), np.int64)
        table = np.full((len(kf_ids), KFDB_NEIGHBOURS), -1, np.int64)
        rows = [rows] if len(kf_ids) == 1 and np.ndim(rows) == 1 and len(rows) and np.ndim(rows[0]) == 0 else rows
        if len(rows) != len(kf_ids):
            raise ValueError("one row per keyframe id")
        for k, r in enumerate(rows):
            r = np.asarray(r, np.int64)[:KFDB_NEIGHBOURS]
            table[k, : len(r)] = r
        check(self._L.orbfe_kfdb_set_covisibles(self._h, len(kf_ids), ptr(kf_ids), ptr(table)), "orbfe_kfdb_set_covisibles")

    def size(self):
        """(live entries, slots handed out since the last clear)"""
        a, b = C.c_int(0), C.c_int(0)
        check(self._L.orbfe_kfdb_size(self._h, C.byref(a), C.byref(b)), "orbfe_kfdb_size")
        return a.value, b.value

    def __len__(self):
        return self.size()[0]

    def slots(self) -> np.ndarray:
        """the keyframe id of every slot, -1 where erased"""
        n = self.size()[1]
        out = np.full(n, -1, np.int64)
        check(self._L.orbfe_kfdb_slots(self._h, ptr(out), n, None), "orbfe_kfdb_slots")
        return out

    def score(self, ids, vals, kf_ids) -> np.ndarray:
        """Vocabulary::score of (ids, vals) against the listed keyframes; KFDB_SCORE_UNKNOWN where an id is not in the database"""
        ids, vals = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)
        kf_ids = np.ascontiguousarray(kf_ids, np.int64)
        out = np.zeros(len(kf_ids), np.float32)
        check(self._L.orbfe_kfdb_score(self._h, ptr(ids), ptr(vals), len(ids), ptr(kf_ids), len(kf_ids), ptr(out)), "orbfe_kfdb_score")
        return out

    # ---- detection, host form ----------------------------------------------------------------------------------------------------
    def _detect(self, queries, loop, min_scores, connected, cand_cap, dense) -> Detection:
        Q = len(queries)
        off, ids, vals = pack_queries(queries)
        n_slots = self.size()[1]
        cap = max(n_slots, 1) if cand_cap is None else int(cand_cap)
        cand = np.full((Q, cap), -1, np.int64)
        n_cand = np.zeros(Q, np.int32)
        info = np.zeros(Q, KFDB_INFO_DTYPE)
        words = np.full((Q, n_slots), -1, np.int32) if dense else None
        scores = np.full((Q, n_slots), np.nan, np.float32) if dense else None
        if loop:
            ms = np.ascontiguousarray(min_scores, np.float32)
            if ms.shape != (Q,) or len(connected) != Q:
                raise ValueError("one min_score and one connected set per query")
            c_off, c_ids = pack_connected(connected)
            check(self._L.orbfe_kfdb_detect_loop(self._h, Q, ptr(off), ptr(ids), ptr(vals), ptr(ms), ptr(c_off), ptr(c_ids), cap, ptr(cand),
                                                 ptr(n_cand), ptr(info), ptr(words), ptr(scores)), "orbfe_kfdb_detect_loop")
        else:
            check(self._L.orbfe_kfdb_detect_relocalization(self._h, Q, ptr(off), ptr(ids), ptr(vals), cap, ptr(cand), ptr(n_cand), ptr(info),
                                                           ptr(words), ptr(scores)), "orbfe_kfdb_detect_relocalization")
        return Detection([cand[q, : min(int(n_cand[q]), cap)].copy() for q in range(Q)], n_cand, info, words, scores)

    def detect_relocalization_batch(self, queries, cand_cap=None, dense=False) -> Detection:
        """queries = [(ids, vals), ...], applied in index order (the carried mRelocScore of a slot moves with each query that scores it)"""
        return self._detect(queries, False, None, None, cand_cap, dense)

    def detect_loop_batch(self, queries, min_scores, connected, cand_cap=None, dense=False) -> Detection:
        return self._detect(queries, True, min_scores, connected, cand_cap, dense)

    def detect_relocalization_candidates(self, ids, vals) -> list:
        """KeyFrameDatabase::DetectRelocalizationCandidates(F): keyframe ids"""
        return self.detect_relocalization_batch([(ids, vals)]).candidates[0].tolist()

    def detect_loop_candidates(self, ids, vals, min_score: float, connected=()) -> list:
        """KeyFrameDatabase::DetectLoopCandidates(pKF, minScore); connected = ids of pKF->GetConnectedKeyFrames()"""
        return self.detect_loop_batch([(ids, vals)], [min_score], [connected]).candidates[0].tolist()

    # ---- detection, device form --------------------------------------------------------------------------------------------------
    def detect_relocalization_device(self, Q, d_q_offsets, d_q_ids, d_q_vals, cand_cap, d_cand, d_n_cand, d_info=None, d_common_words=None,
                                     d_scores=None, stream=None) -> None:
        """Device tensors (int32 offsets [Q + 1] and ids, float64 values; int64 cand [Q][cand_cap], int32 n_cand [Q], optional uint8
        info [Q][32], int32 / float32 [Q][n_slots]); asynchronous on `stream`"""
        check(self._L.orbfe_kfdb_detect_relocalization_device(self._h, int(Q), ptr(d_q_offsets), ptr(d_q_ids), ptr(d_q_vals), int(cand_cap),
                                                              ptr(d_cand), ptr(d_n_cand), ptr(d_info), ptr(d_common_words), ptr(d_scores),
                                                              _lib.stream_handle(stream)), "orbfe_kfdb_detect_relocalization_device")

    def detect_loop_device(self, Q, d_q_offsets, d_q_ids, d_q_vals, d_min_score, d_conn_offsets, d_conn_ids, cand_cap, d_cand, d_n_cand,
                           d_info=None, d_common_words=None, d_scores=None, stream=None) -> None:
        check(self._L.orbfe_kfdb_detect_loop_device(self._h, int(Q), ptr(d_q_offsets), ptr(d_q_ids), ptr(d_q_vals), ptr(d_min_score),
                                                    ptr(d_conn_offsets), ptr(d_conn_ids), int(cand_cap), ptr(d_cand), ptr(d_n_cand),
                                                    ptr(d_info), ptr(d_common_words), ptr(d_scores), _lib.stream_handle(stream)),
              "orbfe_kfdb_detect_loop_device")
