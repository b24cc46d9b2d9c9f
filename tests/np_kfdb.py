"""Yardstick of the keyframe database (KeyFrameDatabase::DetectRelocalizationCandidates / DetectLoopCandidates,
L/src/KeyFrameDatabase.cc:34-304, with L1Scoring::score, D/src/ScoringObject.cpp:23-68): two independent readings and a seeded
scene builder with named cases.  Nothing here calls the library.

  Literal   python lists and an inverted file, per-keyframe fields mnRelocQuery, mnRelocWords, mRelocScore, mnLoopQuery, mnLoopWords,
            mLoopScore, np.float32 wherever the reference is float.  Expected values come from this reading.
  SetReading  the restatement the device evaluates: per (query, slot) common-word counts and first common words, the sharing set
            ordered by (first common word, slot), the carried relocalisation score per slot.

Both start mRelocScore at 0 when a keyframe is added (the reference leaves it uninitialised): the one documented deviation.

A case is (n_words, ops); an op is one of
  ("add", kf_id, ids, vals)   ("erase", kf_id)   ("clear",)   ("covis", kf_id, row of 10 ids padded with -1)
  ("reloc", [query, ...])     one batch; a query is dict(ids, vals)
  ("loop", [query, ...])      a query is dict(ids, vals, min_score, connected = ascending ids)
  ("score", query, [kf_id, ...])
run(reading, ops) gives one result per query op: a list of per-query dicts (cand, info, dense) or, for "score", a float32 array."""
import numpy as np

F32 = np.float32
NEIGHBOURS = 10
SCORE_UNKNOWN = F32(-1.0)
INFO_FIELDS = ("n_sharing", "max_common_words", "min_common_words", "n_scored", "n_matches", "best_acc_score", "min_score_to_retain",
               "n_candidates")


def l1_score(q_ids, q_vals, e_ids, e_vals):
    """L1Scoring::score followed by the conversion to float of `float si = mpVoc->score(...)`"""
    i = j = 0
    score = 0.0
    nq, ne = len(q_ids), len(e_ids)
    while i < nq and j < ne:
        if q_ids[i] == e_ids[j]:
            vi, wi = float(q_vals[i]), float(e_vals[j])
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif q_ids[i] < e_ids[j]:
            while i < nq and q_ids[i] < e_ids[j]:   # lower_bound
                i += 1
        else:
            while j < ne and e_ids[j] < q_ids[i]:
                j += 1
    return F32(-score / 2.0)


def min_common_words(max_common):
    return int(F32(max_common) * F32(0.8))


def _info(n_sharing=0, maxc=0, minc=0, n_scored=0, n_matches=0, best=F32(0), retain=F32(0), n_cand=0):
    return dict(zip(INFO_FIELDS, (n_sharing, maxc, minc, n_scored, n_matches, F32(best), F32(retain), n_cand)))


def _result(cand, info, dense, events=None, trace=None):
    """trace (literal reading only): per entry of lScoreAndMatch (si, [the neighbour scores added, in order], accScore, pBestKF's id)"""
    info["n_candidates"] = len(cand)
    return dict(cand=list(cand), info=info, dense=dense, events=events or {}, trace=trace or [])


# ---- the literal reading ---------------------------------------------------------------------------------------------------------
class _KF:
    def __init__(self, kid):
        self.id = kid
        self.ids = self.vals = None
        self.neigh = []
        self.slot = -1
        self.mnRelocQuery = self.mnLoopQuery = -1
        self.mnRelocWords = self.mnLoopWords = 0
        self.mRelocScore = self.mLoopScore = F32(0)


class Literal:
    def __init__(self, n_words, zero_stale=False):
        self.n_words = n_words
        self.zero_stale = zero_stale   # a stale mRelocScore reads as 0: only to show that the stale reads matter
        self.clear()

    def clear(self):
        self.inv = [[] for _ in range(self.n_words)]
        self.objs = {}
        self.n_slots = 0
        self.slot_ids = []
        self.next_query = 1

    def _obj(self, kid):
        if kid not in self.objs:
            self.objs[kid] = _KF(kid)
        return self.objs[kid]

    def add(self, kid, ids, vals):
        kf = self._obj(kid)
        kf.ids, kf.vals = np.asarray(ids), np.asarray(vals)
        kf.slot = self.n_slots
        kf.mRelocScore = F32(0)
        self.n_slots += 1
        self.slot_ids.append(kid)
        for w in kf.ids:
            self.inv[w].append(kf)

    def erase(self, kid):
        kf = self.objs.get(kid)
        if kf is None or kf.ids is None or kf.slot < 0 or self.slot_ids[kf.slot] != kid:
            return
        for w in kf.ids:
            lst = self.inv[w]
            for k, o in enumerate(lst):
                if o is kf:
                    del lst[k]
                    break
        self.slot_ids[kf.slot] = -1

    def covis(self, kid, row):
        self._obj(kid).neigh = [int(x) for x in row][:NEIGHBOURS]

    def score(self, q, kf_ids):
        out = []
        for kid in kf_ids:
            kf = self.objs.get(kid)
            live = kf is not None and kf.slot >= 0 and self.slot_ids[kf.slot] == kid
            out.append(l1_score(q["ids"], q["vals"], kf.ids, kf.vals) if live else SCORE_UNKNOWN)
        return np.array(out, F32)

    def reloc(self, batch):
        return [self._reloc(q) for q in batch]

    def loop(self, batch):
        return [self._loop(q) for q in batch]

    def _reloc(self, q):
        qid = self.next_query
        self.next_query += 1
        sharing = []
        for w in q["ids"]:
            for kf in self.inv[w]:
                if kf.mnRelocQuery != qid:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = qid
                    sharing.append(kf)
                kf.mnRelocWords += 1
        if not sharing:
            return _result([], _info(), {})
        maxc = max(kf.mnRelocWords for kf in sharing)
        minc = min_common_words(maxc)
        matches, dense = [], {}
        for kf in sharing:
            if kf.mnRelocWords > minc:
                si = l1_score(q["ids"], q["vals"], kf.ids, kf.vals)
                kf.mRelocScore = si
                matches.append((si, kf))
                dense[kf.slot] = (kf.mnRelocWords, si)
        if not matches:
            return _result([], _info(len(sharing), maxc, minc), {})
        ev = dict(stale_reads=0, stale_nonzero=0, replacements=0, dedups=0, unscored_candidates=0)
        acc_list, best_acc, trace = [], F32(0), []
        for si, kf in matches:
            best, acc, pbest = si, si, kf
            added = []
            for nid in kf.neigh:
                k2 = self.objs.get(nid) if nid >= 0 else None
                if k2 is None or k2.mnRelocQuery != qid:
                    continue
                s2 = k2.mRelocScore
                if not k2.mnRelocWords > minc:
                    ev["stale_reads"] += 1
                    ev["stale_nonzero"] += int(s2 != 0)
                    if self.zero_stale:
                        s2 = F32(0)
                acc = F32(acc + s2)
                added.append((s2, k2.id))
                if s2 > best:
                    pbest, best = k2, s2
                    ev["replacements"] += 1
            acc_list.append((acc, pbest))
            trace.append((si, kf.id, added, acc, pbest.id))
            if acc > best_acc:
                best_acc = acc
        retain = F32(0.75) * best_acc
        cand, seen = [], set()
        for acc, kf in acc_list:
            if acc > retain:
                if kf.id not in seen:
                    cand.append(kf.id)
                    seen.add(kf.id)
                    ev["unscored_candidates"] += int(not kf.mnRelocWords > minc)
                else:
                    ev["dedups"] += 1
        return _result(cand, _info(len(sharing), maxc, minc, len(matches), len(matches), best_acc, retain), dense, ev, trace)

    def _loop(self, q):
        qid = self.next_query
        self.next_query += 1
        connected = set(int(c) for c in q["connected"])
        min_score = F32(q["min_score"])
        sharing = []
        for w in q["ids"]:
            for kf in self.inv[w]:
                if kf.mnLoopQuery != qid:
                    kf.mnLoopWords = 0
                    if kf.id not in connected:
                        kf.mnLoopQuery = qid
                        sharing.append(kf)
                kf.mnLoopWords += 1
        if not sharing:
            return _result([], _info(), {})
        maxc = max(kf.mnLoopWords for kf in sharing)
        minc = min_common_words(maxc)
        matches, dense, nscores = [], {}, 0
        for kf in sharing:
            if kf.mnLoopWords > minc:
                nscores += 1
                si = l1_score(q["ids"], q["vals"], kf.ids, kf.vals)
                kf.mLoopScore = si
                dense[kf.slot] = (kf.mnLoopWords, si)
                if si >= min_score:
                    matches.append((si, kf))
        if not matches:
            return _result([], _info(len(sharing), maxc, minc, nscores), dense)
        ev = dict(replacements=0, dedups=0, equal_min_score=sum(int(si == min_score) for si, _ in matches))
        acc_list, best_acc, trace = [], min_score, []
        for si, kf in matches:
            best, acc, pbest = si, si, kf
            added = []
            for nid in kf.neigh:
                k2 = self.objs.get(nid) if nid >= 0 else None
                if k2 is None:
                    continue
                if k2.mnLoopQuery == qid and k2.mnLoopWords > minc:
                    acc = F32(acc + k2.mLoopScore)
                    added.append((k2.mLoopScore, k2.id))
                    if k2.mLoopScore > best:
                        pbest, best = k2, k2.mLoopScore
                        ev["replacements"] += 1
            acc_list.append((acc, pbest))
            trace.append((si, kf.id, added, acc, pbest.id))
            if acc > best_acc:
                best_acc = acc
        retain = F32(0.75) * best_acc
        cand, seen = [], set()
        for acc, kf in acc_list:
            if acc > retain:
                if kf.id not in seen:
                    cand.append(kf.id)
                    seen.add(kf.id)
                else:
                    ev["dedups"] += 1
        return _result(cand, _info(len(sharing), maxc, minc, nscores, len(matches), best_acc, retain), dense, ev, trace)


# ---- the set reading -------------------------------------------------------------------------------------------------------------
class SetReading:
    def __init__(self, n_words):
        self.n_words = n_words
        self.clear()

    def clear(self):
        self.slots, self.live, self.rows = [], {}, {}

    @property
    def slot_ids(self):
        return [e["id"] if e["live"] else -1 for e in self.slots]

    def add(self, kid, ids, vals):
        self.live[kid] = len(self.slots)
        self.slots.append(dict(id=kid, ids=np.asarray(ids), vals=np.asarray(vals), live=True, state=F32(0)))

    def erase(self, kid):
        if kid in self.live:
            self.slots[self.live.pop(kid)]["live"] = False

    def covis(self, kid, row):
        self.rows[kid] = [int(x) for x in row][:NEIGHBOURS]

    def score(self, q, kf_ids):
        out = []
        for kid in kf_ids:
            if kid in self.live:
                e = self.slots[self.live[kid]]
                out.append(self._score(q, e))
            else:
                out.append(SCORE_UNKNOWN)
        return np.array(out, F32)

    @staticmethod
    def _score(q, e):
        common, iq, ie = np.intersect1d(q["ids"], e["ids"], assume_unique=True, return_indices=True)
        total = 0.0
        for a, b in zip(iq, ie):   # intersect1d returns ascending ids
            vi, wi = float(q["vals"][a]), float(e["vals"][b])
            total += abs(vi - wi) - abs(vi) - abs(wi)
        return F32(-total / 2.0)

    def reloc(self, batch):
        return [self._detect(q, False) for q in batch]

    def loop(self, batch):
        return [self._detect(q, True) for q in batch]

    def _detect(self, q, loop):
        n = len(self.slots)
        words, first = np.zeros(n, np.int64), np.full(n, -1, np.int64)
        connected = set(int(c) for c in q["connected"]) if loop else set()
        for s, e in enumerate(self.slots):
            if e["live"] and e["id"] not in connected:
                common = np.intersect1d(q["ids"], e["ids"], assume_unique=True)
                words[s] = len(common)
                if len(common):
                    first[s] = common[0]
        in_s = words > 0
        if not in_s.any():
            return _result([], _info(), {})
        maxc = int(words.max())
        minc = min_common_words(maxc)
        scored = words > minc
        score = {int(s): self._score(q, self.slots[s]) for s in np.flatnonzero(scored)}
        dense = {s: (int(words[s]), score[s]) for s in score}
        order = sorted(np.flatnonzero(in_s), key=lambda s: (first[s], s))
        min_score = F32(q["min_score"]) if loop else F32(0)
        matches = [int(s) for s in order if scored[s] and (not loop or score[int(s)] >= min_score)]
        state = [e["state"] for e in self.slots]
        if not loop:
            for s, v in score.items():
                self.slots[s]["state"] = v
        if not matches:
            return _result([], _info(int(in_s.sum()), maxc, minc, len(score)), dense)
        acc_list, best_acc = [], min_score
        for s in matches:
            acc = best = score[s]
            pbest = s
            for nid in self.rows.get(self.slots[s]["id"], []):
                s2 = self.live.get(nid, -1) if nid >= 0 else -1
                if s2 < 0 or not in_s[s2]:
                    continue
                if loop and not scored[s2]:
                    continue
                v = score[s2] if scored[s2] else state[s2]
                acc = F32(acc + v)
                if v > best:
                    best, pbest = v, s2
            acc_list.append((acc, pbest))
            best_acc = max(best_acc, acc)
        retain = F32(0.75) * best_acc
        cand = []
        for acc, b in acc_list:
            kid = self.slots[b]["id"]
            if acc > retain and kid not in cand:
                cand.append(kid)
        return _result(cand, _info(int(in_s.sum()), maxc, minc, len(score), len(matches), best_acc, retain), dense)


def run(reading, ops):
    """Applies the ops; one entry per "reloc" / "loop" / "score" op"""
    out = []
    for op in ops:
        kind = op[0]
        if kind == "add":
            reading.add(op[1], op[2], op[3])
        elif kind == "erase":
            reading.erase(op[1])
        elif kind == "clear":
            reading.clear()
        elif kind == "covis":
            reading.covis(op[1], op[2])
        elif kind == "reloc":
            out.append(reading.reloc(op[1]))
        elif kind == "loop":
            out.append(reading.loop(op[1]))
        elif kind == "score":
            out.append(reading.score(op[1], op[2]))
        else:
            raise ValueError(kind)
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def make_vector(rng, pool, n, n_words, noise=0):
    """n words drawn from `pool` (plus `noise` from anywhere), values positive and L1-normalised as DBoW2 leaves them"""
    ids = set(rng.choice(pool, size=min(n, len(pool)), replace=False).tolist())
    while noise > 0 and len(ids) < n + noise:
        ids.add(int(rng.integers(0, n_words)))
    ids = np.array(sorted(ids), np.int32)
    vals = rng.random(len(ids)) + 0.05
    return ids, (vals / vals.sum()).astype(np.float64)


def vector(ids, vals=None):
    ids = np.asarray(ids, np.int32)
    if vals is None:
        vals = np.full(len(ids), 1.0 / max(len(ids), 1))
    return ids, np.asarray(vals, np.float64)


def query(ids, vals=None, min_score=None, connected=()):
    ids, vals = vector(ids, vals)
    q = dict(ids=ids, vals=vals)
    if min_score is not None:
        q["min_score"] = F32(min_score)
        q["connected"] = np.array(sorted(int(c) for c in connected), np.int64)
    return q


def place_pool(p, n_words, width=220, step=90):
    lo = (p * step) % max(n_words - width, 1)
    return np.arange(lo, lo + width)


def make_map(seed, n_kf, n_places, n_words=3000, words=(60, 130), first_id=100):
    """A trajectory through `n_places` places whose word pools overlap their neighbours': keyframe k sits in place k * n_places //
    n_kf, draws its words from that pool and is covisible with up to ten keyframes around it (a few ids name no keyframe)."""
    rng = np.random.default_rng(seed)
    ops, kfs = [], []
    for k in range(n_kf):
        p = k * n_places // n_kf
        ids, vals = make_vector(rng, place_pool(p, n_words), int(rng.integers(*words)), n_words, noise=int(rng.integers(0, 6)))
        kid = first_id + 3 * k
        kfs.append(dict(id=kid, place=p, ids=ids, vals=vals))
        ops.append(("add", kid, ids, vals))
    for k, kf in enumerate(kfs):
        around = [j for j in range(max(0, k - 9), min(n_kf, k + 10)) if j != k]
        pick = rng.permutation(around)[: int(rng.integers(3, 11))]
        row = [kfs[j]["id"] for j in pick]
        if rng.random() < 0.2 and row:
            row[int(rng.integers(len(row)))] = 7   # an id that is never added
        row = (row + [-1] * NEIGHBOURS)[:NEIGHBOURS]
        kf["row"] = row
        ops.append(("covis", kf["id"], row))
    return rng, ops, kfs


def _reloc_queries(rng, kfs, n, n_places, n_words):
    out = []
    for _ in range(n):
        p = int(rng.integers(0, n_places))
        ids, vals = make_vector(rng, place_pool(p, n_words), int(rng.integers(70, 140)), n_words, noise=3)
        out.append(dict(ids=ids, vals=vals))
    return out


def _loop_queries(rng, ops, kfs, n, n_places, n_words):
    """A new keyframe at a place seen before: connected = keyframes around a random one there, minScore = the lowest score against them
    (LoopClosing::DetectLoop, L/src/LoopClosing.cc:112-133), computed by the literal reading"""
    out = []
    for _ in range(n):
        k = int(rng.integers(0, len(kfs)))
        ids, vals = make_vector(rng, place_pool(kfs[k]["place"], n_words), int(rng.integers(70, 140)), n_words, noise=3)
        conn = [kfs[j]["id"] for j in range(max(0, k - 3), min(len(kfs), k + 3))]
        q = query(ids, vals, 0.0, conn)
        scores = [l1_score(ids, vals, kfs[j]["ids"], kfs[j]["vals"]) for j in range(max(0, k - 3), min(len(kfs), k + 3))]
        q["min_score"] = F32(min(scores) * F32(0.5))
        out.append(q)
    return out


def case_reloc_sequence():
    n_words = 3000
    rng, ops, kfs = make_map(11, 150, 14, n_words)
    return n_words, ops + [("reloc", _reloc_queries(rng, kfs, 40, 14, n_words))]


def case_reloc_singles():
    """single-query calls with an erase and a re-add between them"""
    n_words = 3000
    rng, ops, kfs = make_map(12, 60, 6, n_words)
    qs = _reloc_queries(rng, kfs, 10, 6, n_words)
    for i, q in enumerate(qs):
        ops.append(("reloc", [q]))
        if i % 3 == 1:
            ops.append(("erase", kfs[5 * i]["id"]))
        if i % 3 == 2:
            kf = kfs[5 * (i - 1)]
            ops.append(("add", kf["id"], kf["ids"], kf["vals"]))
    return n_words, ops


def case_loop_basic():
    n_words = 3000
    rng, ops, kfs = make_map(13, 120, 10, n_words)
    return n_words, ops + [("loop", _loop_queries(rng, ops, kfs, 20, 10, n_words))]


def case_reloc_edges():
    """Crafted.  X = 10 is scored by query A; in query B it shares one word (in S, not scored) and is the neighbour of Y = 11 and Y2 = 13:
    its stale score joins their sums, beats their own scores (an unscored neighbour becomes the candidate, twice: de-duplicated) and
    lifts bestAccScore so far that Z = 12 falls under the threshold.  Query C shares no word with anything."""
    n_words = 2000
    ops = [("add", 10, *vector(range(0, 50))), ("add", 11, *vector(range(100, 150))), ("add", 12, *vector(range(200, 250))),
           ("add", 13, *vector(range(300, 350))), ("covis", 11, [10] + [-1] * 9), ("covis", 13, [7, 10] + [-1] * 8)]
    a = query(range(0, 50))
    b = query([0] + list(range(100, 150)) + list(range(200, 250)) + list(range(300, 350)))
    c = query(range(1000, 1040))
    return n_words, ops + [("reloc", [a]), ("reloc", [b, c])]


def case_loop_edges():
    """From the loop scene: the connected set holds the top-scoring entry; minScore equals one entry's score exactly; minScore above
    every score (lScoreAndMatch empty); no common word (lKFsSharingWords empty)."""
    n_words = 3000
    rng, ops, kfs = make_map(14, 80, 8, n_words)
    ids, vals = make_vector(rng, place_pool(3, n_words), 110, n_words, noise=2)
    lit = Literal(n_words)
    run(lit, ops)
    free = lit.loop([query(ids, vals, 0.0, [])])[0]
    scores = sorted(((v[1], lit.slot_ids[s]) for s, v in free["dense"].items()), reverse=True)
    top = scores[0][1]
    mid = scores[len(scores) // 2][0]
    unused = np.setdiff1d(np.arange(n_words), np.concatenate([kf["ids"] for kf in kfs]))
    qs = [query(ids, vals, 0.0, []), query(ids, vals, 0.0, [top]), query(ids, vals, mid, []), query(ids, vals, 2.0, []),
          query(unused[:50], None, 0.0, [])]
    return n_words, ops + [("loop", qs)]


def case_erase_readd():
    """A = 1 and B = 2 share the query's first word and score alike: [A, B]; after erase(A), add(A) the list of every word holds B in
    front of A: [B, A]"""
    n_words = 500
    v = vector(range(0, 50))
    ops = [("add", 1, *v), ("add", 2, *v), ("add", 3, *vector(range(25, 75)))]
    q = query(range(0, 50))
    return n_words, ops + [("reloc", [q]), ("erase", 1), ("reloc", [q]), ("add", 1, *v), ("reloc", [q])]


def case_interleaved():
    """add, erase, clear and re-add between queries of both kinds and score calls"""
    n_words = 3000
    rng, ops, kfs = make_map(15, 50, 5, n_words)
    qs = _reloc_queries(rng, kfs, 6, 5, n_words)
    lq = _loop_queries(rng, ops, kfs, 4, 5, n_words)
    listed = [kfs[0]["id"], kfs[7]["id"], 7, kfs[20]["id"]]
    ops += [("reloc", qs[:2]), ("score", qs[0], listed), ("erase", kfs[7]["id"]), ("erase", 424242), ("loop", lq[:2]), ("score", qs[0], listed),
            ("reloc", qs[2:4]), ("clear",), ("reloc", qs[4:5]), ("loop", lq[2:3])]
    for kf in kfs[10:30]:
        ops.append(("add", kf["id"], kf["ids"], kf["vals"]))
    for kf in kfs[10:30]:
        ops.append(("covis", kf["id"], kf["row"]))
    return n_words, ops + [("reloc", qs[4:]), ("loop", lq[2:]), ("score", lq[3], listed)]


def case_shapes():
    """Entry lengths 0, 1, 63, 64, 65, 128, 129 and query lengths 1, 63, 64, 65, 4096; the common word first, last or alone; word ids 0
    and n_words - 1"""
    n_words = 8192
    rng = np.random.default_rng(16)
    ops = []
    lens = (0, 1, 63, 64, 65, 128, 129)
    for k, n in enumerate(lens):
        ids = np.sort(rng.choice(np.arange(1, n_words - 1), size=n, replace=False)).astype(np.int32)
        vals = rng.random(n) + 0.05
        ops.append(("add", 10 + k, ids, vals / max(vals.sum(), 1e-300)))
    ends = np.array([0, n_words - 1], np.int32)
    ops.append(("add", 30, ends, np.array([0.25, 0.75])))
    ops.append(("add", 31, np.arange(0, 4096, dtype=np.int32) * 2, np.full(4096, 1.0 / 4096)))
    e = {op[1]: op for op in ops}
    qs = [query([0]), query([n_words - 1]), query(e[14][2][:1]), query(e[14][2][-1:]), query(e[11][2])]
    for n in (63, 64, 65):
        qs.append(query(np.sort(np.concatenate([e[15][2][: n - 1], [n_words - 1]]))))
        qs.append(query(e[16][2][-n:]))
    big = np.arange(0, 4096, dtype=np.int32) * 2 + 1
    big[0], big[-1] = 0, n_words - 1
    qs.append(query(big, np.random.default_rng(17).random(4096) + 0.01))
    qs.append(query(np.arange(0, 4096, dtype=np.int32) * 2, np.random.default_rng(18).random(4096) + 0.01))
    return n_words, ops + [("reloc", qs), ("loop", [dict(q, min_score=F32(0), connected=np.zeros(0, np.int64)) for q in qs])]


def strip_case(n_entries, seed=19):
    """n_entries entries and a few queries of both kinds: for entry counts around the strip of the common pass"""
    n_words = 1500
    rng, ops, kfs = (np.random.default_rng(seed), [], []) if n_entries == 0 else make_map(seed, n_entries, max(1, n_entries // 12), n_words)
    qs = _reloc_queries(rng, kfs, 3, max(1, n_entries // 12), n_words)
    lq = [dict(q, min_score=F32(0.01), connected=np.array(sorted(k["id"] for k in kfs[:2]), np.int64)) for q in qs]
    return n_words, ops + [("reloc", qs), ("loop", lq)]


def _both_sums(terms):
    ordered = 0.0
    for t in terms:
        ordered += t
    partial = [0.0] * 64
    for k, t in enumerate(terms):
        partial[k % 64] += t
    strided = 0.0
    for p in partial:
        strided += p
    return F32(-ordered / 2.0), F32(-strided / 2.0)


def ordered_sum_case(seed=20, tries=200):
    """One (query, entry) pair whose ascending-order sum rounds to another float than the sum of 64-strided partial sums (lane l adds
    the terms l, l + 64, ... and the partial sums are added in lane order).  The two double sums differ in their last bits, so the
    floats differ only when a rounding boundary of float lies between them: the last common word carries the same value x on both
    sides (its term is exactly -2x), and a seeded search moves x in steps of one double ulp around the value that puts the score on
    the midpoint of two floats.  Returns (n_words, ops, the strided float)."""
    rng = np.random.default_rng(seed)
    n_words = 1000
    for _ in range(tries):
        n = int(rng.integers(130, 400))
        ids = np.sort(rng.choice(n_words, size=n, replace=False)).astype(np.int32)
        qv, ev = rng.random(n) + 0.01, rng.random(n) + 0.01
        qv, ev = qv / qv.sum(), ev / ev.sum()
        terms = [abs(a - b) - abs(a) - abs(b) for a, b in zip(qv.tolist(), ev.tolist())]
        rest = 0.0
        for t in terms[:-1]:
            rest += t
        lo = F32(-rest / 2.0 + 0.02)
        mid = (float(lo) + float(np.nextafter(lo, F32(2)))) / 2.0   # the midpoint of two neighbouring floats above the rest's score
        x = mid + rest / 2.0
        for _ in range(64):
            x = float(np.nextafter(x, 0.0))
        for _ in range(128):
            x = float(np.nextafter(x, 1.0))
            o, st = _both_sums(terms[:-1] + [abs(x - x) - abs(x) - abs(x)])
            if o != st:
                qv[-1] = ev[-1] = x
                q = dict(ids=ids, vals=qv)
                return n_words, [("add", 5, ids, ev), ("reloc", [q]), ("score", q, [5])], st
    raise AssertionError("no pair found")


CASES = {
    "reloc_sequence": case_reloc_sequence, "reloc_singles": case_reloc_singles, "loop_basic": case_loop_basic,
    "reloc_edges": case_reloc_edges, "loop_edges": case_loop_edges, "erase_readd": case_erase_readd, "interleaved": case_interleaved,
    "shapes": case_shapes,
}


def same(a, b):
    """two results of run(): candidate ids in order, every info field (floats as bits), the dense outputs (scores as bits)"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if isinstance(ra, np.ndarray):
            if not np.array_equal(ra.view(np.uint32), rb.view(np.uint32)):
                return False
            continue
        if len(ra) != len(rb):
            return False
        for x, y in zip(ra, rb):
            if x["cand"] != y["cand"] or sorted(x["dense"]) != sorted(y["dense"]):
                return False
            for f in INFO_FIELDS:
                u, v = x["info"][f], y["info"][f]
                if (F32(u).tobytes() != F32(v).tobytes()) if isinstance(u, np.floating) else (u != v):
                    return False
            for s in x["dense"]:
                if x["dense"][s][0] != y["dense"][s][0] or F32(x["dense"][s][1]).tobytes() != F32(y["dense"][s][1]).tobytes():
                    return False
    return True
