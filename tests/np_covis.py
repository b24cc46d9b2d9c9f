"""The yardstick of the covisibility graph (L/ = Source/Libraries/ORB_SLAM2/): KeyFrame::UpdateConnections (L/src/KeyFrame.cc:268-354),
the vote of Tracking::UpdateLocalKeyFrames (L/src/Tracking.cc:1115-1159) and LocalMapping::KeyFrameCulling (L/src/LocalMapping.cc:595-655)
with KeyFrame::SetBadFlag (L/src/KeyFrame.cc:416-434) and MapPoint::EraseObservation / SetBadFlag (L/src/MapPoint.cc:112-176).

Each function is read TWICE.
  literal_*   the reference's statements one by one: dictionaries keyed by `order` stand for std::map<KeyFrame*, ...> (iterating a map
              is iterating ascending order), sort() on (weight, order) pairs and push_front are carried out, and the culling really
              mutates a copy of the map: SetBadFlag erases observations, lowers nObs, turns points bad and clears their slots.
  *_records   the form the device evaluates: a histogram over keyframe rows and one 64-bit sort key per mode; for the culling no mutation
              at all, only the set of rows culled so far, from which a point's state follows off its own list.  These also decide what
              is REFUSED, and they produce the records of include/orbfe.h byte for byte.
tests/test_covis_cpu.py shows the two equal on every scene; the GPU suite compares bytes with the second.

A scene is {"keyframes": [...], "points": [...]} as refactored_orb_slam2_amd.covisibility.pack_covisibility takes it.  Every literal
function takes `dev`, a set of switchable deviations (DEVIATIONS), each a plausible misreading; each must change at least three answers
on the committed scenes."""
import copy

import numpy as np

CONNECTIONS, VOTES = 0, 1
OK, EMPTY, OVERFLOW, REFUSED = 0, 1, 2, 3
KEPT, CULLED, MARKED, SKIPPED_ID0, ROW_REFUSED = 0, 1, 2, 3, 4
TH = 15
HEADER_DTYPE = np.dtype([("n_counted", "<i4"), ("n_ordered", "<i4"), ("kf_max", "<i4"), ("w_max", "<i4"), ("status", "<i4"),
                         ("n_written", "<i4"), ("single", "<i4"), ("reserved", "<i4")])
ENTRY_DTYPE = np.dtype([("kf", "<i4"), ("weight", "<i4")])
VERDICT_DTYPE = np.dtype([("n_mps", "<i4"), ("n_redundant", "<i4"), ("verdict", "<i4"), ("reserved", "<i4")])
DEVIATIONS = ("th14", "th16", "ties_ascending", "last_max", "ge_ratio", "same_octave", "stereo_minus_one", "no_carry")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
class MapBuilder:
    """a map inside the stated domain: slot i of keyframe k holds p exactly when the list of p holds (k, i); lists in map order"""

    def __init__(self, orders=None):
        self.kfs, self.pts, self.orders = [], [], orders

    def keyframe(self, n_keys, th_depth=40.0, id0=False, not_erase=False, bad=False):
        k = len(self.kfs)
        self.kfs.append({"order": k if self.orders is None else int(self.orders[k]), "bad": bad, "slots": [-1] * n_keys,
                         "octaves": [0] * n_keys, "u_right": [-1.0] * n_keys, "depth": [-1.0] * n_keys, "th_depth": th_depth,
                         "id0": id0, "not_erase": not_erase, "_free": 0})
        return k

    def point(self, views, bad=False):
        """views: (keyframe, octave, stereo, depth) each; the keypoint is the keyframe's next free slot.  A bad point keeps no list."""
        p = len(self.pts)
        obs, weighted = [], 0
        for k, octave, stereo, depth in ([] if bad else views):
            K = self.kfs[k]
            i = K["_free"]
            K["_free"] += 1
            K["slots"][i], K["octaves"][i], K["u_right"][i], K["depth"][i] = p, octave, (10.0 if stereo else -1.0), depth
            obs.append((k, i))
            weighted += 2 if stereo else 1
        obs.sort(key=lambda o: self.kfs[o[0]]["order"])
        self.pts.append({"obs": obs, "bad": bad, "n_obs_weighted": weighted})
        return p

    def scene_after(self, made):
        return self.scene(), made

    def scene(self):
        return {"keyframes": [{k: v for k, v in K.items() if k != "_free"} for K in self.kfs], "points": self.pts}


def make_map(seed, n_kf=24, n_points=420, n_keys=150, window=7, stereo=0.5, n_bad=12):
    """a seeded map whose neighbouring keyframes share enough points for weights on both sides of 15"""
    rng = np.random.default_rng(seed)
    B = MapBuilder(rng.permutation(n_kf))
    for k in range(n_kf):
        B.keyframe(n_keys, th_depth=35.0, id0=(k == 0), not_erase=bool(rng.random() < 0.12), bad=bool(k and rng.random() < 0.1))
    for p in range(n_points):
        c = int(rng.integers(0, n_kf))
        near = [k for k in range(max(0, c - window), min(n_kf, c + window + 1)) if B.kfs[k]["_free"] < n_keys]
        n = min(len(near), int(rng.integers(2, 8)))
        if n < 2:
            continue
        base = int(rng.integers(0, 6))
        views = [(int(k), base + int(rng.integers(0, 3)), bool(rng.random() < stereo), float(np.float32(rng.uniform(-2.0, 50.0))))
                 for k in rng.choice(near, n, replace=False)]
        B.point(views)
    for _ in range(n_bad):
        B.point([], bad=True)
    return B.scene()


def make_cull_map(seed, n_kf=14, n_points=260, n_keys=120, stereo=0.5):
    """a seeded map dense enough that several keyframes of a local list are redundant and their culling reaches the next ones"""
    rng = np.random.default_rng(seed)
    B = MapBuilder(rng.permutation(n_kf))
    for k in range(n_kf):
        B.keyframe(n_keys, th_depth=35.0, id0=(k == 0), not_erase=bool(rng.random() < 0.15))
    for p in range(n_points):
        c = int(rng.integers(0, n_kf))
        near = [k for k in range(max(0, c - 3), min(n_kf, c + 4)) if B.kfs[k]["_free"] < n_keys]
        n = min(len(near), int(rng.choice([2, 4, 4, 5, 5, 6])))
        if n < 2:
            continue
        base = int(rng.integers(0, 5))
        views = [(int(k), base + int(rng.integers(0, 2)), bool(rng.random() < stereo), float(np.float32(rng.uniform(0.0, 38.0))))
                 for k in rng.choice(near, n, replace=False)]
        B.point(views)
    return B.scene()


def obs_scene(n):
    """three points with n observations each, by the rows 1 .. n of n + 2; returns the scene and the three slots"""
    B = MapBuilder(np.random.default_rng(n).permutation(n + 2))
    for k in range(n + 2):
        B.keyframe(4)
    return B.scene_after([B.point([(r, 0, False, 1.0) for r in range(1, n + 1)]) for _ in range(3)])


def map_subjects(scene, seed=0):
    """every keyframe as a CONNECTIONS subject (some bad points put into its empty slots, as a stale vector holds them), and frames as
    VOTES subjects: random draws of the map's points, bad ones and empty slots included"""
    rng = np.random.default_rng(seed)
    bad = [i for i, p in enumerate(scene["points"]) if p["bad"]]
    out = []
    for k, K in enumerate(scene["keyframes"]):
        s = list(K["slots"])
        for i in range(len(s)):
            if s[i] == -1 and bad and rng.random() < 0.05:
                s[i] = int(rng.choice(bad))
        out.append((s, k, CONNECTIONS))
    for _ in range(max(4, len(scene["keyframes"]) // 2)):
        n = int(rng.integers(20, 200))
        s = rng.integers(-1, len(scene["points"]), n).tolist()
        out.append((s, -1, VOTES))
    return out


def map_problems(scene, seed=0, n=6):
    """culling problems: windows of rows in a random order, both sensor kinds"""
    rng = np.random.default_rng(seed)
    n_kf = len(scene["keyframes"])
    out = []
    for q in range(n):
        m = int(rng.integers(3, n_kf))
        out.append((rng.permutation(n_kf)[:m].tolist(), q % 3 == 2))
    return out


def weights_scene(n_kf, weights, orders=None, self_row=0, kf_bad=(), n_empty=0):
    """a scene and the slots of one subject whose counter is exactly `weights` ({row: weight}): slot j's point is seen by self_row and by
    every row with a weight > j"""
    B = MapBuilder(orders)
    W = max(list(weights.values()) + [0])
    n_keys = W + n_empty + 1
    for k in range(n_kf):
        B.keyframe(n_keys if (k == self_row or k in weights) else 0, bad=k in kf_bad)
    for j in range(W):
        B.point([(self_row, 0, False, 1.0)] + [(r, 0, False, 1.0) for r, w in weights.items() if w > j])
    return B.scene(), list(B.kfs[self_row]["slots"])


# ---- the literal reading -----------------------------------------------------------------------------------------------------------
def _observations(scene, p):
    """GetObservations(): the map keyed by KeyFrame*, here by order -> (row, idx); the list is given in map order already"""
    kfs = scene["keyframes"]
    return {kfs[k]["order"]: (k, i) for k, i in scene["points"][p]["obs"]}


def literal_connections(scene, slots, self_row, dev=frozenset()):
    """KeyFrame.cc:268-354.  Returns None for the early return, else a dict with weights ({row: w} = mConnectedKeyFrameWeights),
    ordered_kfs, ordered_ws, kf_max, w_max, single."""
    kfs, pts = scene["keyframes"], scene["points"]
    row_of = {K["order"]: k for k, K in enumerate(kfs)}
    KFcounter = {}
    for p in slots:
        if p == -1:
            continue
        if pts[p]["bad"]:
            continue
        observations = _observations(scene, p)
        for order in sorted(observations):
            if observations[order][0] == self_row:        # mit->first->mnId == mnId
                continue
            KFcounter[order] = KFcounter.get(order, 0) + 1
    if not KFcounter:
        return None
    nmax, pKFmax = 0, None
    th = 14 if "th14" in dev else 16 if "th16" in dev else TH
    vPairs = []
    for order in sorted(KFcounter):
        w = KFcounter[order]
        if (w >= nmax and "last_max" in dev) or w > nmax:
            nmax, pKFmax = w, order
        if w >= th:
            vPairs.append((w, order))
    single = not vPairs
    if single:
        vPairs.append((nmax, pKFmax))
    if "ties_ascending" in dev:
        vPairs.sort(key=lambda t: (t[0], -t[1]))
    else:
        vPairs.sort()
    lKFs, lWs = [], []
    for w, order in vPairs:
        lKFs.insert(0, row_of[order])                       # push_front
        lWs.insert(0, w)
    return {"weights": {row_of[o]: w for o, w in KFcounter.items()}, "ordered_kfs": lKFs, "ordered_ws": lWs, "kf_max": row_of[pKFmax],
            "w_max": nmax, "single": single}


def literal_votes(scene, slots, dev=frozenset()):
    """Tracking.cc:1115-1159.  Returns None for the early return, else a dict with counter ({row: w}), local (mvpLocalKeyFrames as
    filled by the vote), kf_max, w_max (None, 0: every voted keyframe is bad)."""
    kfs, pts = scene["keyframes"], scene["points"]
    row_of = {K["order"]: k for k, K in enumerate(kfs)}
    counter = {}
    for p in slots:
        if p != -1:
            if not pts[p]["bad"]:
                for order in sorted(_observations(scene, p)):
                    counter[order] = counter.get(order, 0) + 1
    if not counter:
        return None
    mx, pKFmax, local = 0, None, []
    for order in sorted(counter):
        if kfs[row_of[order]]["bad"]:
            continue
        if (counter[order] >= mx and "last_max" in dev) or counter[order] > mx:
            mx, pKFmax = counter[order], order
        local.append(row_of[order])
    return {"counter": {row_of[o]: w for o, w in counter.items()}, "local": local, "kf_max": None if pKFmax is None else row_of[pKFmax],
            "w_max": mx}


class _Mutable:
    """the part of the map that KeyFrameCulling changes, copied so that it can really be changed"""

    def __init__(self, scene):
        self.kfs = copy.deepcopy(scene["keyframes"])
        self.obs = [dict((self.kfs[k]["order"], (k, i)) for k, i in p["obs"]) for p in scene["points"]]
        self.n_obs = [p["n_obs_weighted"] for p in scene["points"]]
        self.bad = [bool(p["bad"]) for p in scene["points"]]
        self.kf_bad = [False] * len(self.kfs)

    def point_set_bad(self, p):                               # MapPoint::SetBadFlag
        self.bad[p] = True
        obs, self.obs[p] = self.obs[p], {}
        for k, i in obs.values():
            self.kfs[k]["slots"][i] = -1                      # EraseMapPointMatch

    def erase_observation(self, p, k, dev):                   # MapPoint::EraseObservation
        order = self.kfs[k]["order"]
        if order in self.obs[p]:
            idx = self.obs[p][order][1]
            if self.kfs[k]["u_right"] is not None and np.float32(self.kfs[k]["u_right"][idx]) >= 0 and "stereo_minus_one" not in dev:
                self.n_obs[p] -= 2
            else:
                self.n_obs[p] -= 1
            del self.obs[p][order]
            if self.n_obs[p] <= 2:
                self.point_set_bad(p)

    def keyframe_set_bad(self, k, dev):                       # KeyFrame::SetBadFlag, what of it reaches the culling
        K = self.kfs[k]
        if K["id0"]:
            return KEPT
        if K["not_erase"]:
            return MARKED                                     # mbToBeErased
        for i in range(len(K["slots"])):
            if K["slots"][i] != -1:
                self.erase_observation(K["slots"][i], k, dev)
        self.kf_bad[k] = True
        return CULLED


def literal_cull(scene, local, monocular, dev=frozenset()):
    """LocalMapping.cc:603-654 on a copy of the map that is mutated as the reference mutates it.  Returns [(n_mps, n_redundant, verdict)]."""
    M = _Mutable(scene)
    out = []
    for k in local:
        if "no_carry" in dev:
            M = _Mutable(scene)
        K = M.kfs[k]
        if K["id0"]:
            out.append((0, 0, SKIPPED_ID0))
            continue
        vpMapPoints = list(K["slots"])
        nRedundant = nMPs = 0
        for i, p in enumerate(vpMapPoints):
            if p == -1:
                continue
            if M.bad[p]:
                continue
            if not monocular:
                d = np.float32(K["depth"][i])
                if d > np.float32(K["th_depth"]) or d < 0:
                    continue
            nMPs += 1
            if M.n_obs[p] > 3:
                scaleLevel = K["octaves"][i]
                nObs = 0
                for order in sorted(M.obs[p]):
                    ki, ii = M.obs[p][order]
                    if ki == k:
                        continue
                    lim = scaleLevel if "same_octave" in dev else scaleLevel + 1
                    if M.kfs[ki]["octaves"][ii] <= lim:
                        nObs += 1
                        if nObs >= 3:
                            break
                if nObs >= 3:
                    nRedundant += 1
        redundant = nRedundant >= 0.9 * nMPs if "ge_ratio" in dev else nRedundant > 0.9 * nMPs
        out.append((nMPs, nRedundant, M.keyframe_set_bad(k, dev) if redundant else KEPT))
    return out


# ---- the second reading: what the device evaluates, and what it refuses --------------------------------------------------------------
def _key(mode, w, order, kf_bad):
    if w == 0:
        return 0
    if mode == CONNECTIONS:
        return (w << 32) | order
    return 0 if kf_bad else 0xFFFFFFFF - order


def count_subject(scene, slots, self_row, mode, conn_cap):
    """one subject: (header tuple in HEADER_DTYPE order, [(kf, weight)] written)"""
    kfs, pts = scene["keyframes"], scene["points"]
    n_kf = len(kfs)
    refused = ((0, 0, -1, 0, REFUSED, 0, 0, 0), [])
    if mode not in (CONNECTIONS, VOTES) or (mode == CONNECTIONS and not -1 <= self_row < n_kf):
        return refused
    me = -1 if mode == VOTES else self_row
    hist = [0] * n_kf
    for p in slots:
        if p == -1:
            continue
        if p < -1 or p >= len(pts):
            return refused
        if pts[p]["bad"]:
            continue
        for k, _ in pts[p]["obs"]:
            if not 0 <= k < n_kf or not 0 <= kfs[k]["order"] < n_kf:
                return refused
            if k != me:
                hist[k] += 1
    n_counted = sum(1 for w in hist if w)
    ent = [(_key(mode, w, kfs[r]["order"], kfs[r]["bad"]), r) for r, w in enumerate(hist)]
    ent = sorted((e for e in ent if e[0]), reverse=True)
    n_ordered = len(ent) if mode == VOTES else sum(1 for _, r in ent if hist[r] >= TH)
    best = max([((hist[r] << 32) | (0xFFFFFFFF - kfs[r]["order"]), r) for _, r in ent], default=(0, -1))
    status = EMPTY if n_counted == 0 else OVERFLOW if len(ent) > conn_cap else OK
    n_written = min(len(ent), conn_cap)
    single = int(mode == CONNECTIONS and n_ordered == 0 and n_counted > 0)
    return (n_counted, n_ordered, best[1], best[0] >> 32, status, n_written, single, 0), [(r, hist[r]) for _, r in ent[:n_written]]


def count_records(scene, subjects, conn_cap, prior=None):
    """HEADER_DTYPE (S) and ENTRY_DTYPE (S, conn_cap) as orbfe_covis_count* leave them; entries that are not written keep `prior`"""
    S = len(subjects)
    headers = np.zeros(S, HEADER_DTYPE)
    entries = np.zeros((S, conn_cap), ENTRY_DTYPE) if prior is None else prior.copy().reshape(S, conn_cap)
    for s, (slots, me, mode) in enumerate(subjects):
        h, e = count_subject(scene, slots, me, mode, conn_cap)
        headers[s] = h
        for j, (kf, w) in enumerate(e):
            entries[s, j] = (kf, w)
    return headers, entries


def cull_problem(scene, local, monocular):
    """one problem with the culled set in place of the mutation: [(n_mps, n_redundant, verdict)]"""
    kfs, pts = scene["keyframes"], scene["points"]
    n_kf = len(kfs)
    culled = set()
    out = []
    for k in local:
        if not 0 <= k < n_kf:
            out.append((0, 0, ROW_REFUSED))
            continue
        K = kfs[k]
        if K["id0"]:
            out.append((0, 0, SKIPPED_ID0))
            continue
        if len(K["slots"]) and not monocular and K["depth"] is None:
            out.append((0, 0, ROW_REFUSED))
            continue
        n_mps = n_red = 0
        ok = True
        for i, p in enumerate(K["slots"]):
            if p == -1:
                continue
            if p < -1 or p >= len(pts):
                ok = False
                break
            if pts[p]["bad"]:
                continue
            removed = n_obs = 0
            for ko, io in pts[p]["obs"]:
                if not 0 <= ko < n_kf or not 0 <= io < len(kfs[ko]["slots"]):
                    ok = False
                    break
                if ko in culled:
                    ur = kfs[ko]["u_right"]
                    removed += 2 if ur is not None and np.float32(ur[io]) >= 0 else 1
                elif ko != k:
                    if n_obs < 3 and kfs[ko]["octaves"][io] <= K["octaves"][i] + 1:
                        n_obs += 1
            if not ok:
                break
            nw = pts[p]["n_obs_weighted"]
            if removed > 0 and nw - removed <= 2:
                continue
            if not monocular:
                d = np.float32(K["depth"][i])
                if d > np.float32(K["th_depth"]) or d < 0:
                    continue
            n_mps += 1
            n_red += 1 if (nw - removed > 3 and n_obs >= 3) else 0
        if not ok:
            out.append((0, 0, ROW_REFUSED))
            continue
        verdict = KEPT if not float(n_red) > 0.9 * float(n_mps) else MARKED if K["not_erase"] else CULLED
        if verdict == CULLED:
            culled.add(k)
        out.append((n_mps, n_red, verdict))
    return out


def cull_records(scene, problems):
    """VERDICT_DTYPE, one record per element of the concatenated local lists, as orbfe_covis_cull_keyframes* leave them"""
    rows = [r for local, mono in problems for r in cull_problem(scene, local, mono)]
    out = np.zeros(len(rows), VERDICT_DTYPE)
    for j, (a, b, v) in enumerate(rows):
        out[j] = (a, b, v, 0)
    return out


# ---- the two readings side by side -------------------------------------------------------------------------------------------------
def connections_view(scene, slots, self_row, dev=frozenset()):
    """what the literal reading leaves behind, in a form both readings can be brought to"""
    r = literal_connections(scene, slots, self_row, dev)
    if r is None:
        return None
    return (sorted(r["weights"].items()), list(zip(r["ordered_kfs"], r["ordered_ws"])), r["kf_max"], r["w_max"])


def connections_view_of_records(scene, slots, self_row):
    h, e = count_subject(scene, slots, self_row, CONNECTIONS, len(scene["keyframes"]) + 1)
    if h[4] == EMPTY:
        return None
    assert h[4] == OK
    ordered = [(h[2], h[3])] if h[6] else e[:h[1]]
    return (sorted(e), ordered, h[2], h[3])


def votes_view(scene, slots, dev=frozenset()):
    r = literal_votes(scene, slots, dev)
    if r is None:
        return None
    return (len(r["counter"]), [(k, r["counter"][k]) for k in r["local"]], -1 if r["kf_max"] is None else r["kf_max"], r["w_max"])


def votes_view_of_records(scene, slots):
    h, e = count_subject(scene, slots, -1, VOTES, len(scene["keyframes"]) + 1)
    if h[4] == EMPTY:
        return None
    assert h[4] == OK and h[1] == len(e)
    return (h[0], e, h[2], h[3])


# ---- the committed scenes ------------------------------------------------------------------------------------------------------------
def committed_cull_maps():
    """[(scene, problems)]"""
    return [(m, map_problems(m, seed, 4)) for seed, m in ((seed, make_cull_map(seed)) for seed in (1, 2, 3))]


def committed_maps():
    return [make_map(seed) for seed in (1, 2, 3)] + [make_map(4, n_kf=12, n_points=260, n_keys=160, window=4, stereo=0.8)]


def chain_unredundant():
    """culling A leaves the shared points with Observations() == 3, so B is no longer redundant"""
    B = MapBuilder()
    a, b, c, d = (B.keyframe(12) for _ in range(4))
    for _ in range(10):
        B.point([(a, 0, False, 1.0), (b, 0, False, 1.0), (c, 0, False, 1.0), (d, 0, False, 1.0)])
    return B.scene(), [a, b, c, d]


def chain_bad_point():
    """culling A turns X (seen by A and C only) bad; without X, C's nine redundant points of nine pass 0.9"""
    B = MapBuilder()
    a, c, e, f, g = (B.keyframe(24) for _ in range(5))
    for _ in range(10):
        B.point([(a, 0, False, 1.0), (e, 0, False, 1.0), (f, 0, False, 1.0), (g, 0, False, 1.0)])
    B.point([(a, 0, False, 1.0), (c, 0, False, 1.0)])
    for _ in range(9):
        B.point([(c, 0, False, 1.0), (e, 0, False, 1.0), (f, 0, False, 1.0), (g, 0, False, 1.0)])
    return B.scene(), [a, c]


def chain_stereo():
    """A is culled; Y1 held a stereo observation of A (4 -> 2: bad), Y2 a monocular one (4 -> 3: alive, no longer > 3)"""
    B = MapBuilder()
    a, c, e, f, g = (B.keyframe(24) for _ in range(5))
    for _ in range(10):
        B.point([(a, 0, False, 1.0), (e, 0, False, 1.0), (f, 0, False, 1.0), (g, 0, False, 1.0)])
    B.point([(a, 0, True, 1.0), (c, 0, False, 1.0), (e, 0, False, 1.0)])
    B.point([(a, 0, False, 1.0), (c, 0, False, 1.0), (e, 0, False, 1.0), (f, 0, False, 1.0)])
    for _ in range(9):
        B.point([(c, 0, False, 1.0), (e, 0, False, 1.0), (f, 0, False, 1.0), (g, 0, False, 1.0)])
    return B.scene(), [a, c]


def ratio_scene(n_redundant, n_plain=0, octave_step=1, depths=None, th_depth=40.0, flags=None, n_keys=None):
    """keyframe 0 with n_redundant points seen by three more keyframes `octave_step` levels up, and n_plain points seen by two more"""
    B = MapBuilder()
    n = n_redundant + n_plain
    rows = [B.keyframe(n_keys or n + 1, th_depth=th_depth, **(flags or {}))] + [B.keyframe(n + 1) for _ in range(3)]
    for j in range(n):
        depth = 1.0 if depths is None else depths[j]
        others = rows[1:] if j < n_redundant else rows[1:3]
        B.point([(rows[0], 2, False, depth)] + [(r, 2 + octave_step, False, 1.0) for r in others])
    return B.scene(), [rows[0]]


def directed_cull_cases():
    """name -> (scene, [(local, monocular)], the verdicts (n_mps, n_redundant, verdict) the case is there for)"""
    th = np.float32(40.0)
    above, below = float(np.nextafter(th, np.float32(np.inf))), float(np.nextafter(th, np.float32(0)))
    cases = {}
    s, loc = ratio_scene(9, 1)
    cases["nine_of_ten"] = (s, [(loc, False)], [(10, 9, KEPT)])
    s, loc = ratio_scene(10)
    cases["ten_of_ten"] = (s, [(loc, False)], [(10, 10, CULLED)])
    s, loc = ratio_scene(18, 2)
    cases["eighteen_of_twenty"] = (s, [(loc, False)], [(20, 18, KEPT)])
    s, loc = ratio_scene(27, 3)
    cases["twentyseven_of_thirty"] = (s, [(loc, False)], [(30, 27, KEPT)])
    s, loc = ratio_scene(0, 0, n_keys=5)
    cases["no_points"] = (s, [(loc, False)], [(0, 0, KEPT)])
    s, loc = ratio_scene(4, 4)                                      # Observations() of 4 and of 3
    cases["observations_3_and_4"] = (s, [(loc, False)], [(8, 4, KEPT)])
    s, loc = ratio_scene(10, octave_step=1)
    cases["octave_plus_1"] = (s, [(loc, True)], [(10, 10, CULLED)])
    s, loc = ratio_scene(10, octave_step=2)
    cases["octave_plus_2"] = (s, [(loc, True)], [(10, 0, KEPT)])
    depths = [float(th), above, -0.5, below, 0.0, 1.0, 39.0, 2.0, 3.0, 4.0]
    s, loc = ratio_scene(10, depths=depths)
    cases["depth_gate"] = (s, [(loc, False)], [(8, 8, CULLED)])
    cases["depth_gate_monocular"] = (s, [(loc, True)], [(10, 10, CULLED)])
    s, loc = ratio_scene(10, flags={"id0": True})
    cases["id0"] = (s, [(loc, False)], [(0, 0, SKIPPED_ID0)])
    s, loc = chain_unredundant()
    cases["chain_unredundant"] = (s, [(loc, False)], [(10, 10, CULLED), (10, 0, KEPT), (10, 0, KEPT), (10, 0, KEPT)])
    s2 = copy.deepcopy(s)
    s2["keyframes"][loc[0]]["not_erase"] = True                     # MARKED: no carry-over, so B is culled instead
    cases["not_erase"] = (s2, [(loc, False)], [(10, 10, MARKED), (10, 10, CULLED), (10, 0, KEPT), (10, 0, KEPT)])
    s, loc = chain_bad_point()
    cases["chain_bad_point"] = (s, [(loc, False)], [(11, 10, CULLED), (9, 9, CULLED)])
    cases["chain_bad_point_reversed"] = (s, [(loc[::-1], False)], [(10, 9, KEPT), (11, 10, CULLED)])
    s, loc = chain_stereo()
    cases["chain_stereo"] = (s, [(loc, False)], [(12, 11, CULLED), (10, 9, KEPT)])
    # local lists of length 0, 1 and 65, a keyframe with 65 slots and one with more slots than the workgroup has threads
    B = MapBuilder(np.random.default_rng(5).permutation(70))
    rows = [B.keyframe(65 if k == 3 else 300 if k == 4 else 24) for k in range(70)]
    rng = np.random.default_rng(6)
    for p in range(330):
        views = [(4, 1, False, 1.0)] if p < 300 else []
        views += [(3, 1, False, 1.0)] if p < 65 else []
        for k in rng.choice([r for r in rows if r not in (3, 4) and B.kfs[r]["_free"] < 24], 3, replace=False):
            views.append((int(k), int(rng.integers(0, 4)), bool(rng.random() < 0.5), float(rng.uniform(-1, 45))))
        B.point(views)
    s = B.scene()
    long_local = [3, 4] + [r for r in rows if r not in (3, 4)][:63]
    cases["lengths"] = (s, [([], False), ([4], False), (long_local, False), ([3], True), (long_local[::-1], True)], None)
    return cases


def directed_count_cases():
    """name -> (scene, [(slots, self, mode)], conn_cap)"""
    cases = {}
    s, slots = weights_scene(6, {1: 3, 2: 5})
    bad_scene = copy.deepcopy(s)
    for p in bad_scene["points"]:
        p["bad"], p["obs"] = True, []
    cases["no_slots"] = (s, [([], 0, CONNECTIONS), ([], -1, VOTES)], 4)
    cases["all_empty"] = (s, [([-1] * 70, 0, CONNECTIONS), ([-1] * 3, -1, VOTES)], 4)
    cases["all_bad"] = (bad_scene, [(list(range(5)), 0, CONNECTIONS), (list(range(5)), -1, VOTES)], 4)
    s, slots = weights_scene(4, {})
    B = MapBuilder()
    B.keyframe(8), B.keyframe(8)
    for _ in range(5):
        B.point([(0, 0, False, 1.0)])
    cases["only_self"] = (B.scene(), [(list(B.kfs[0]["slots"]), 0, CONNECTIONS), (list(B.kfs[0]["slots"]), -1, VOTES)], 4)
    for n in (1, 63, 64, 65, 257):
        s, slots = weights_scene(9, {1: n, 2: max(1, n // 2), 5: max(1, n - 1), 7: 1}, orders=[3, 8, 0, 1, 2, 7, 6, 5, 4], n_empty=3)
        cases[f"slots_{n}"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 16)
    for n in (1, 64, 65):                                           # observations of one point
        s, slots = obs_scene(n)
        cases[f"obs_{n}"] = (s, [(slots, 0, CONNECTIONS), (slots + [-1], 1, CONNECTIONS), (slots, -1, VOTES)], 128)
    s, slots = weights_scene(6, {1: 14, 2: 15, 3: 16, 5: 2}, orders=[0, 4, 2, 5, 1, 3])
    cases["weights_14_15_16"] = (s, [(slots, 0, CONNECTIONS)], 8)
    s, slots = weights_scene(7, {1: 9, 2: 9, 4: 9, 5: 3}, orders=[6, 4, 1, 0, 5, 3, 2])
    cases["tie_below_15"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 8)
    s, slots = weights_scene(8, {1: 15, 2: 15, 3: 20, 4: 20, 5: 17, 6: 20, 7: 15}, orders=[7, 2, 6, 0, 5, 1, 4, 3])
    cases["ties_from_15"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 8)
    s, slots = weights_scene(12, {r: 3 + (r * 5) % 4 for r in range(1, 9)}, orders=np.random.default_rng(8).permutation(12))
    cases["cap_exact"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 8)
    s, slots = weights_scene(12, {r: 3 + (r * 5) % 4 for r in range(1, 10)}, orders=np.random.default_rng(9).permutation(12))
    cases["cap_plus_one"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 8)
    s, slots = weights_scene(40, {r: 1 + (r * 7) % 19 for r in range(1, 40)}, orders=np.random.default_rng(10).permutation(40))
    cases["overflow_far"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 5)
    top = 32768
    s, slots = weights_scene(top, {top - 1: 5, 3: 5, 17: 2}, orders=np.arange(top)[::-1].copy())
    cases["highest_row"] = (s, [(slots, 0, CONNECTIONS), (slots, -1, VOTES)], 8)
    s, slots = weights_scene(6, {1: 4, 2: 12, 3: 9, 4: 1}, orders=[0, 5, 1, 3, 2, 4], kf_bad=(0, 2))
    cases["bad_keyframe_max"] = (s, [(slots, -1, VOTES), (slots, 0, CONNECTIONS)], 8)
    s, slots = weights_scene(6, {1: 4, 2: 9}, kf_bad=(1, 2))
    cases["all_voted_bad"] = (s, [(slots, -1, VOTES)], 8)
    s, slots = weights_scene(6, {1: 4, 2: 9, 3: 16})
    n_pts = len(s["points"])
    cases["refused_between"] = (s, [(slots, 0, CONNECTIONS), (slots[:3] + [n_pts] + slots[3:], 0, CONNECTIONS), (slots, -1, VOTES),
                                    (slots[:2] + [-2], -1, VOTES), (slots, 6, CONNECTIONS), (slots, 0, 2), (slots, 5, CONNECTIONS)], 8)
    broken = copy.deepcopy(s)
    broken["points"][1]["obs"][0] = (6, 0)                          # a keyframe row outside the table
    cases["refused_row"] = (broken, [(slots[2:], 0, CONNECTIONS), (slots, 0, CONNECTIONS), (slots[:1], -1, VOTES), (slots, -1, VOTES)], 8)
    broken = copy.deepcopy(s)
    broken["keyframes"][2]["order"] = 6                             # an order outside [0, n_kf) on an observed row
    cases["refused_order"] = (broken, [(slots, 0, CONNECTIONS), ([-1, -1], 0, CONNECTIONS)], 8)
    return cases
