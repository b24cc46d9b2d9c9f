"""The yardstick of the local map of a tracked frame (L/ = Source/Libraries/ORB_SLAM2/): Tracking::UpdateLocalKeyFrames
(L/src/Tracking.cc:1115-1214), Tracking::UpdateLocalPoints (:1090-1113) and the first half of Tracking::SearchLocalPoints (:1036-1049,
:1057-1060) with the mnLastFrameSeen that TrackWithMotionModel / TrackReferenceKeyFrame leave on the outliers they discard (:711, :825).

Read TWICE.
  literal_local_map   the reference's statements one by one on objects: KeyFrame and MapPoint carry mnTrackReferenceForFrame and
                      mnLastFrameSeen, the counter is a dict keyed by `order` (iterating a std::map<KeyFrame*, int> is iterating
                      ascending order), the lists are lists and the three loops run with their `break`s.  It also records the CENSUS:
                      which of the edges named in EDGES the run reached.
  table_reading       the form the device evaluates, on the packed tables: one mark bit per keyframe row and per point, the voted
                      entries as the vote left them, graph rows, the children array.  It decides what is REFUSED / OVERFLOW / EMPTY and
                      produces the records of include/orbfe.h byte for byte.
tests/test_localmap_cpu.py shows the two equal on every directed case and on seeded maps; the GPU suite compares bytes with the second.

A scene is np_covis's ({"keyframes": [...], "points": [...]}); a keyframe may also carry parent (row or None), children (rows) and best
(rows in GetVectorCovisibleKeyFrames() order, ANY length: GetBestCovisibilityKeyFrames(10) takes the first ten).  A problem is a dict:
scene, frames [(slots, also-seen point indices)], conn_cap, kf_cap, p_cap, and optionally tamper(tables), which damages the packed tables
(only the table reading and the device see those)."""
import numpy as np

from tests import np_covis as C

OK, EMPTY, OVERFLOW, REFUSED = 0, 1, 2, 3
STOP_EXHAUSTED, STOP_SIZE, STOP_PARENT = 0, 1, 2
BEST, SIZE = 10, 80
GRAPH_DTYPE = np.dtype([("parent", "<i4"), ("child_offset", "<i4"), ("n_children", "<i4"), ("n_best", "<i4"), ("best", "<i4", (10,))])
FRAME_DTYPE = np.dtype([("seen_offset", "<i4"), ("n_seen", "<i4")])
SUBJECT_DTYPE = np.dtype([("slot_offset", "<i4"), ("n_slots", "<i4"), ("self", "<i4"), ("mode", "<i4")])
HEADER_DTYPE = np.dtype([("n_voted", "<i4"), ("n_local_kf", "<i4"), ("n_local_points", "<i4"), ("ref_kf", "<i4"), ("stop", "<i4"),
                         ("status", "<i4"), ("reserved", "<i4", (2,))])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("skip", "<i4"),
                            ("observed", "<i4"), ("desc", "u1", (32,))])
CANARY = 0x5C

# every edge the directed cases must reach at least once (the issue's list)
EDGES = ("stop:exhausted", "stop:size@80voted", "stop:size@81voted", "stop:size@82voted", "stop:size@crossing", "stop:parent@first",
         "stop:parent@later", "best:all_marked", "best:all_bad", "best:tenth", "best:eleventh_eligible", "best:none", "child:none", "child@0",
         "child@63", "child@64", "child@65", "child:bad_passed", "parent:absent", "parent:marked", "parent:bad", "slots:0", "slots:1",
         "slots:63", "slots:64", "slots:65", "slots:1024", "slots:1025", "slots:2049", "point:everywhere", "point:bad", "slot:-1",
         "point:last", "row:highest", "skip:frame_held", "skip:seen", "seen:not_local", "frame:bad_slot", "seen:none", "kf_cap:exact",
         "kf_cap:over1", "p_cap:exact", "p_cap:over1", "status:empty", "vote:overflow")
REFUSAL_CAUSES = ("vote_refused", "vote_overflow", "n_written", "kf_max", "voted_row", "n_best", "best_row", "child_row", "child_slice",
                  "parent_row", "parent_below", "slot_high", "slot_low", "frame_slot", "frame_slice", "seen_index", "seen_negative",
                  "seen_slice", "n_keys", "slots_null", "slots_misaligned")
HIGHEST_ROW = 32767


# ---- the literal reading -----------------------------------------------------------------------------------------------------------
class _KeyFrame:
    def __init__(self, row, K):
        self.row, self.order, self.bad, self.mnTrackReferenceForFrame = row, K["order"], bool(K.get("bad")), -1
        self.parent, self.children, self.ordered = None, [], []
        self.mvpMapPoints = []

    def isBad(self):
        return self.bad

    def GetBestCovisibilityKeyFrames(self, N):
        return list(self.ordered) if len(self.ordered) < N else self.ordered[:N]   # KeyFrame.cc:180-187

    def GetChilds(self):
        return sorted(self.children, key=lambda c: c.order)   # a copy of std::set<KeyFrame*>: iterated in pointer order

    def GetParent(self):
        return self.parent

    def GetMapPointMatches(self):
        return list(self.mvpMapPoints)


class _MapPoint:
    def __init__(self, index, P):
        self.index, self.bad, self.mnTrackReferenceForFrame, self.mnLastFrameSeen = index, bool(P.get("bad")), -1, -1
        self.observations = {}

    def isBad(self):
        return self.bad

    def GetObservations(self):
        return dict(self.observations)


def _objects(scene):
    kfs = [_KeyFrame(k, K) for k, K in enumerate(scene["keyframes"])]
    pts = [_MapPoint(i, P) for i, P in enumerate(scene["points"])]
    for k, K in enumerate(scene["keyframes"]):
        kfs[k].parent = None if K.get("parent") is None or K["parent"] < 0 else kfs[K["parent"]]
        kfs[k].children = [kfs[c] for c in K.get("children", ())]
        kfs[k].ordered = [kfs[b] for b in K.get("best", ())]
        kfs[k].mvpMapPoints = [None if p == -1 else pts[p] for p in K.get("slots", ())]
    for i, P in enumerate(scene["points"]):
        pts[i].observations = {kfs[k]: idx for k, idx in P["obs"]}
    return kfs, pts


def literal_local_map(scene, slots, seen, frame_id=7):
    """One frame.  Returns a dict: empty (the early return :1133: nothing else is set), local_kf (rows), ref_kf (row or None),
    local_points (indices), skip (per local point), frame_slots (mvpMapPoints afterwards, bad points cleared), marked_kf / marked_points
    (who carries mnTrackReferenceForFrame == the frame's id) and census (a set of EDGES)."""
    kfs, pts = _objects(scene)
    census = set()
    mvpMapPoints = [None if p == -1 else pts[p] for p in slots]
    for p in seen:                                   # :711 / :825: the outlier leaves the frame, its mnLastFrameSeen stays
        pts[p].mnLastFrameSeen = frame_id
    if not len(seen):
        census.add("seen:none")
    # UpdateLocalKeyFrames :1115-1159
    keyframeCounter = {}
    for i in range(len(mvpMapPoints)):
        if mvpMapPoints[i] is not None:
            pMP = mvpMapPoints[i]
            if not pMP.isBad():
                for pKF in sorted(pMP.GetObservations(), key=lambda kf: kf.order):
                    keyframeCounter[pKF.order] = keyframeCounter.get(pKF.order, 0) + 1
            else:
                mvpMapPoints[i] = None
                census.add("frame:bad_slot")
    by_order = {kf.order: kf for kf in kfs}
    out = {"empty": not keyframeCounter, "frame_slots": [-1 if m is None else m.index for m in mvpMapPoints], "census": census}
    if not keyframeCounter:
        census.add("status:empty")
        return out
    mx, pKFmax, mvpLocalKeyFrames = 0, None, []
    for order in sorted(keyframeCounter):
        pKF = by_order[order]
        if pKF.isBad():
            continue
        if keyframeCounter[order] > mx:
            mx, pKFmax = keyframeCounter[order], pKF
        mvpLocalKeyFrames.append(pKF)
        pKF.mnTrackReferenceForFrame = frame_id
    # :1161-1209
    n_voted = len(mvpLocalKeyFrames)
    stop = "exhausted"
    for it in range(n_voted):                        # itEndKF is taken before the loop
        if len(mvpLocalKeyFrames) > 80:
            stop = "size"
            census.add("stop:size@%dvoted" % n_voted if n_voted >= 80 else "stop:size@crossing")
            break
        pKF = mvpLocalKeyFrames[it]
        vNeighs = pKF.GetBestCovisibilityKeyFrames(10)
        taken = None
        for j, pNeighKF in enumerate(vNeighs):
            if not pNeighKF.isBad():
                if pNeighKF.mnTrackReferenceForFrame != frame_id:
                    mvpLocalKeyFrames.append(pNeighKF)
                    pNeighKF.mnTrackReferenceForFrame = frame_id
                    taken = j
                    break
        if not vNeighs:
            census.add("best:none")
        elif taken == 9:
            census.add("best:tenth")
        elif taken is None and len(vNeighs) == 10:
            if all(n.isBad() for n in vNeighs):
                census.add("best:all_bad")
            if all(not n.isBad() for n in vNeighs):
                census.add("best:all_marked")
            if len(pKF.ordered) > 10 and not pKF.ordered[10].isBad() and pKF.ordered[10].mnTrackReferenceForFrame != frame_id:
                census.add("best:eleventh_eligible")
        spChilds = pKF.GetChilds()
        if not spChilds:
            census.add("child:none")
        for j, pChildKF in enumerate(spChilds):
            if not pChildKF.isBad():
                if pChildKF.mnTrackReferenceForFrame != frame_id:
                    mvpLocalKeyFrames.append(pChildKF)
                    pChildKF.mnTrackReferenceForFrame = frame_id
                    census.add("child@%d" % j)
                    if any(c.isBad() for c in spChilds[:j]):
                        census.add("child:bad_passed")
                    break
        pParent = pKF.GetParent()
        if pParent is not None:
            if pParent.mnTrackReferenceForFrame != frame_id:
                mvpLocalKeyFrames.append(pParent)
                pParent.mnTrackReferenceForFrame = frame_id
                stop = "parent"
                census.add("stop:parent@first" if it == 0 else "stop:parent@later")
                if pParent.isBad():
                    census.add("parent:bad")
                break                                # :1206 leaves the for over keyframes
            census.add("parent:marked")
        else:
            census.add("parent:absent")
    if stop == "exhausted":
        census.add("stop:exhausted")
    # UpdateLocalPoints :1090-1113
    mvpLocalMapPoints = []
    holders = {}
    for pKF in mvpLocalKeyFrames:
        vpMPs = pKF.GetMapPointMatches()
        census.add("slots:%d" % len(vpMPs))
        if pKF.row == HIGHEST_ROW:
            census.add("row:highest")
        for pMP in vpMPs:
            if pMP is None:
                census.add("slot:-1")
                continue
            holders[pMP.index] = holders.get(pMP.index, 0) + 1
            if pMP.mnTrackReferenceForFrame == frame_id:
                continue
            if not pMP.isBad():
                mvpLocalMapPoints.append(pMP)
                pMP.mnTrackReferenceForFrame = frame_id
            else:
                census.add("point:bad")
    if len(mvpLocalKeyFrames) >= 3 and any(n == len(mvpLocalKeyFrames) for n in holders.values()):
        census.add("point:everywhere")
    if any(pMP.index == len(pts) - 1 for pMP in mvpLocalMapPoints):
        census.add("point:last")
    # SearchLocalPoints :1036-1049, :1057-1060
    held = set()
    for pMP in mvpMapPoints:
        if pMP is not None:                          # the bad ones left the frame above
            pMP.mnLastFrameSeen = frame_id
            held.add(pMP.index)
    skip = [1 if pMP.mnLastFrameSeen == frame_id else 0 for pMP in mvpLocalMapPoints]
    local = {pMP.index for pMP in mvpLocalMapPoints}
    if held & local:
        census.add("skip:frame_held")
    if (set(seen) - held) & local:
        census.add("skip:seen")
    if set(seen) - local:
        census.add("seen:not_local")
    out.update(local_kf=[kf.row for kf in mvpLocalKeyFrames], ref_kf=None if pKFmax is None else pKFmax.row, n_voted=n_voted, stop=stop,
               local_points=[pMP.index for pMP in mvpLocalMapPoints], skip=skip,
               marked_kf=sorted(kf.row for kf in kfs if kf.mnTrackReferenceForFrame == frame_id),
               marked_points=sorted(p.index for p in pts if p.mnTrackReferenceForFrame == frame_id))
    return out


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def point_records(n_points, seed=5):
    """a resident orbfe_map_point table: every byte of a record depends on its index; skip holds what must be replaced"""
    rng = np.random.default_rng(seed)
    r = np.zeros(n_points, MAP_POINT_DTYPE)
    r["pos"], r["normal"] = rng.normal(0, 10, (n_points, 3)), rng.normal(0, 1, (n_points, 3))
    r["min_distance"], r["max_distance"] = rng.uniform(0.1, 2, n_points), rng.uniform(20, 90, n_points)
    r["skip"], r["observed"] = 0x7E7E7E7E, rng.integers(0, 2, n_points)
    r["desc"] = rng.integers(0, 256, (n_points, 32))
    return r


def tables_of(problem):
    """the packed tables of a problem: graph, children, kf_bad, point_bad, kf_slots (a list of int32 arrays), n_keys, slots_state (0 as
    it is, 1 a null address, 2 a misaligned one), frame_slots, subjects, seen, frames, vote_headers, vote_entries (the vote as np_covis
    reads it, unwritten entries a canary), records; then problem["tamper"] has its way with them"""
    scene, frames, cap = problem["scene"], problem["frames"], problem["conn_cap"]
    kfs, pts = scene["keyframes"], scene["points"]
    graph, children = np.zeros(len(kfs), GRAPH_DTYPE), []
    for k, K in enumerate(kfs):
        ch = sorted(K.get("children", ()), key=lambda c: kfs[c]["order"])
        best = list(K.get("best", ()))[:BEST]
        graph[k]["parent"] = -1 if K.get("parent") is None else K["parent"]
        graph[k]["child_offset"], graph[k]["n_children"], graph[k]["n_best"] = len(children), len(ch), len(best)
        graph[k]["best"][:len(best)] = best
        children += ch
    subjects, fr = np.zeros(len(frames), SUBJECT_DTYPE), np.zeros(len(frames), FRAME_DTYPE)
    fslots, fseen = [], []
    for s, (slots, seen) in enumerate(frames):
        subjects[s] = (len(fslots), len(slots), -1, C.VOTES)
        fr[s] = (len(fseen), len(seen))
        fslots += list(slots)
        fseen += list(seen)
    prior = np.full(len(frames) * cap * 8, CANARY, np.uint8).view(C.ENTRY_DTYPE).reshape(len(frames), cap)
    vh, ve = C.count_records(scene, [(list(slots), -1, C.VOTES) for slots, _ in frames], cap, prior=prior)
    T = {"graph": graph, "children": np.asarray(children, np.int32).reshape(-1), "kf_bad": np.array([int(bool(K.get("bad"))) for K in kfs], np.uint8),
         "point_bad": np.array([int(bool(P.get("bad"))) for P in pts], np.uint8),
         "kf_slots": [np.asarray(K.get("slots", ()), np.int32).reshape(-1).copy() for K in kfs],
         "n_keys": np.array([len(K.get("slots", ())) for K in kfs], np.int32), "slots_state": np.zeros(len(kfs), np.int32),
         "frame_slots": np.asarray(fslots, np.int32).reshape(-1), "subjects": subjects, "seen": np.asarray(fseen, np.int32).reshape(-1),
         "frames": fr, "vote_headers": vh.view(C.HEADER_DTYPE), "vote_entries": ve, "records": point_records(len(pts))}
    if problem.get("tamper"):
        problem["tamper"](T)
    return T


# ---- the table reading -------------------------------------------------------------------------------------------------------------
def _slice_ok(offset, n, total):
    return n >= 0 and offset >= 0 and offset <= total - n


def frame_reading(T, s, conn_cap):
    """one frame on the tables: (status, n_voted, local_kf, ref_kf, stop, local_points, skip); REFUSED and EMPTY carry nothing else"""
    n_kf, n_points = len(T["kf_bad"]), len(T["point_bad"])
    V = T["vote_headers"][s]
    nothing = (0, [], -1, 0, [], [])
    if V["status"] == C.EMPTY:
        return (EMPTY,) + nothing
    refused = (REFUSED,) + nothing
    if V["status"] != C.OK or not 0 <= V["n_written"] <= conn_cap or not -1 <= V["kf_max"] < n_kf:
        return refused
    S, F = T["subjects"][s], T["frames"][s]
    if not _slice_ok(int(S["slot_offset"]), int(S["n_slots"]), len(T["frame_slots"])):
        return refused
    if not _slice_ok(int(F["seen_offset"]), int(F["n_seen"]), len(T["seen"])):
        return refused
    n_voted = int(V["n_written"])
    marked = np.zeros(n_kf, bool)
    local = []
    for e in T["vote_entries"][s][:n_voted]:
        if not 0 <= e["kf"] < n_kf:
            return refused
        local.append(int(e["kf"]))
        marked[e["kf"]] = True
    stop = STOP_EXHAUSTED
    for i in range(n_voted):
        if len(local) > SIZE:
            stop = STOP_SIZE
            break
        G = T["graph"][local[i]]
        if not 0 <= G["n_best"] <= BEST or not _slice_ok(int(G["child_offset"]), int(G["n_children"]), len(T["children"])) or \
                not -1 <= G["parent"] < n_kf:
            return refused
        best = [int(b) for b in G["best"][:G["n_best"]]]
        if any(not 0 <= b < n_kf for b in best):
            return refused
        for b in best:
            if not T["kf_bad"][b] and not marked[b]:
                local.append(b)
                marked[b] = True
                break
        ch = [int(c) for c in T["children"][G["child_offset"]:G["child_offset"] + G["n_children"]]]
        for c0 in range(0, len(ch), 64):            # a chunk of 64 is checked whole before one of it is taken
            chunk = ch[c0:c0 + 64]
            if any(not 0 <= c < n_kf for c in chunk):
                return refused
            hit = [c for c in chunk if not T["kf_bad"][c] and not marked[c]]
            if hit:
                local.append(hit[0])
                marked[hit[0]] = True
                break
        if G["parent"] >= 0 and not marked[G["parent"]]:
            local.append(int(G["parent"]))
            marked[G["parent"]] = True
            stop = STOP_PARENT
            break
    fslots = T["frame_slots"][S["slot_offset"]:S["slot_offset"] + S["n_slots"]]
    seen = T["seen"][F["seen_offset"]:F["seen_offset"] + F["n_seen"]]
    for k in local:
        n = int(T["n_keys"][k])
        if n < 0 or (n > 0 and T["slots_state"][k] != 0):
            return refused
        sl = T["kf_slots"][k][:n]
        if ((sl < -1) | (sl >= n_points)).any():
            return refused
    if ((fslots < -1) | (fslots >= n_points)).any() or ((seen < 0) | (seen >= n_points)).any():
        return refused
    pmark = np.zeros(n_points, bool)
    points = []
    for k in local:
        for p in T["kf_slots"][k][:int(T["n_keys"][k])].tolist():
            if p < 0 or pmark[p] or T["point_bad"][p]:
                continue
            pmark[p] = True
            points.append(p)
    last_seen = np.zeros(n_points, bool)
    for p in fslots.tolist():
        if p >= 0 and not T["point_bad"][p]:
            last_seen[p] = True
    last_seen[seen] = True
    return OK, n_voted, local, int(V["kf_max"]), stop, points, [int(last_seen[p]) for p in points]


def table_reading(T, conn_cap, kf_cap, p_cap, with_records=True, frames=None):
    """every frame (or those listed): a dict of the output arrays as orbfe_local_map* leave them, what is not written a canary"""
    idx = list(range(len(T["subjects"]))) if frames is None else list(frames)
    S = len(idx)
    can = lambda shape, dtype: np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, CANARY, np.uint8).view(dtype).reshape(shape)
    out = {"headers": can((S,), HEADER_DTYPE), "local_kf": can((S, kf_cap), np.int32), "local_points": can((S, p_cap), np.int32),
           "n_points": can((S,), np.int32)}
    if with_records:
        out["map_points"] = can((S, p_cap), MAP_POINT_DTYPE)
    for at, s in enumerate(idx):
        status, n_voted, local, ref_kf, stop, points, skip = frame_reading(T, s, conn_cap)
        if status == OK and (len(local) > kf_cap or len(points) > p_cap):
            status = OVERFLOW
        out["headers"][at] = (n_voted, len(local), len(points), ref_kf, stop, status, (0, 0))
        if status == EMPTY:
            continue
        n = min(len(points), p_cap)
        out["n_points"][at] = n
        out["local_kf"][at, :min(len(local), kf_cap)] = local[:kf_cap]
        out["local_points"][at, :n] = points[:n]
        if with_records and n:
            out["map_points"][at, :n] = T["records"][points[:n]]
            out["map_points"]["skip"][at, :n] = skip[:n]
    return out


def census_of(problem):
    """the edges a problem reaches: the literal reading's of every frame the tables do not refuse, and what the records show"""
    T = tables_of(problem)
    got = set()
    rec = table_reading(T, problem["conn_cap"], problem["kf_cap"], problem["p_cap"])
    for s, (slots, seen) in enumerate(problem["frames"]):
        h = rec["headers"][s]
        if T["vote_headers"][s]["status"] == C.OVERFLOW:
            got.add("vote:overflow")
        if h["status"] == REFUSED:
            got.add("refused")
            continue
        if problem.get("tamper") is None or h["status"] == EMPTY:
            got |= literal_local_map(problem["scene"], slots, seen)["census"]
        if h["status"] == EMPTY:
            continue
        for what, n, cap in (("kf_cap", h["n_local_kf"], problem["kf_cap"]), ("p_cap", h["n_local_points"], problem["p_cap"])):
            if n == cap:
                got.add(what + ":exact")
            if n == cap + 1:
                got.add(what + ":over1")
    return got


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def voted_scene(n_kf, voted, n_keys=3, bad=(), orders=None):
    """n_kf keyframes of n_keys slots; every voted row holds one point of its own, and the frame holds exactly those points: the vote is
    `voted`, each with weight 1.  Returns (builder, frame slots)."""
    B = C.MapBuilder(orders)
    for k in range(n_kf):
        B.keyframe(n_keys, bad=k in bad)
    return B, [B.point([(v, 0, False, 1.0)]) for v in voted]


def _problem(B, frames, conn_cap=128, kf_cap=128, p_cap=256, reaches=(), tamper=None):
    return {"scene": B.scene() if hasattr(B, "scene") else B, "frames": frames, "conn_cap": conn_cap, "kf_cap": kf_cap, "p_cap": p_cap,
            "reaches": set(reaches), "tamper": tamper}


def _link(B, parent, child):
    B.kfs[child]["parent"] = parent
    B.kfs[parent].setdefault("children", []).append(child)


def _children_case(pos):
    """the first eligible child of row 0 sits at set position pos; the ones before it are bad"""
    B, slots = voted_scene(70, [0])
    for c in range(1, pos + 3):
        B.kfs[0].setdefault("children", []).append(c)
        if c - 1 < pos:
            B.kfs[c]["bad"] = True
    reach = ["child@%d" % pos] + (["child:bad_passed"] if pos else [])
    return _problem(B, [(slots, [])], reaches=reach)


def union_sizes_case():
    """local keyframes of 0, 1, 63, 64, 65, 1 024, 1 025 and 2 049 slots, some of them empty, a stale bad point among them, and the
    last point of the table in the last slot"""
    sizes = [0, 1, 63, 64, 65, 1024, 1025, 2049]
    B = C.MapBuilder()
    for n in sizes:
        B.keyframe(n)
    B.keyframe(2)                                    # a keyframe outside the local map
    stale = B.point([], bad=True)
    slots = []
    for k, n in enumerate(sizes):
        K, first = B.kfs[k], True
        while K["_free"] < (n - 1 if k == 7 else n):  # the last slot of the last keyframe is kept for the last point
            i = K["_free"]
            if i % 7 == 3 and i != n - 1:
                K["_free"] += 1                      # an empty slot
                continue
            views = [(k, 0, False, 1.0)]
            if k + 1 < len(sizes) and i % 5 == 0 and B.kfs[k + 1]["_free"] < sizes[k + 1] - 1:
                views.append((k + 1, 0, False, 1.0))  # shared with the next keyframe: already marked when that one is walked
            p = B.point(views)
            if first:
                slots.append(p)
                first = False
    B.kfs[5]["slots"][B.kfs[5]["slots"].index(-1)] = stale
    outside = B.point([(8, 0, False, 1.0)])
    last = B.point([(7, 0, False, 1.0)])
    assert B.kfs[7]["slots"][2048] == last and last == len(B.pts) - 1
    B.kfs[0]["best"] = [1, 2, 3, 4, 5, 6, 7]          # row 0 is not voted (it holds nothing): reached never; row 1 brings the rest
    B.kfs[1]["best"] = [0]
    frames = [(slots + [stale, -1], [outside, slots[0]])]
    return _problem(B, frames, p_cap=8192, reaches=["slots:%d" % n for n in sizes] + ["point:bad", "slot:-1", "point:last", "seen:not_local",
                                                                                     "frame:bad_slot", "skip:frame_held"])


def _caps_scene():
    B, slots = voted_scene(12, [0, 1, 2], n_keys=5)
    B.kfs[0]["best"] = [5]
    B.kfs[1]["best"] = [6]
    for k in range(12):
        for _ in range(2):
            B.point([(k, 0, False, 1.0)])
    return B, slots


def refusal_case(cause):
    """three frames: the middle one is REFUSED for `cause`, its neighbours are not touched by it.  Two clusters of keyframes: rows 0-4
    serve frames 0 and 2, rows 5-9 the middle frame, and the damage lies in the second cluster or in the middle frame's own records."""
    B = C.MapBuilder()
    for k in range(10):
        B.keyframe(6)
    a = [B.point([(0, 0, False, 1.0), (1, 0, False, 1.0)]), B.point([(1, 0, False, 1.0)])]
    b = [B.point([(5, 0, False, 1.0), (6, 0, False, 1.0)]), B.point([(6, 0, False, 1.0)]), B.point([(7, 0, False, 1.0)])]
    extra = B.point([(8, 0, False, 1.0)])
    _link(B, 2, 0)
    _link(B, 8, 5)
    _link(B, 5, 9)
    B.kfs[0]["best"], B.kfs[5]["best"] = [3], [8, 9]
    n_kf, n_points = 10, len(B.pts)
    mid_slots, mid_seen = list(b), [extra]
    conn_cap = 8
    tamper = None
    if cause == "vote_refused":
        mid_slots = b + [n_points]
    elif cause == "frame_slot":                      # the vote is handed over as if it had not looked
        def tamper(T): T["frame_slots"][T["subjects"][1]["slot_offset"]] = -2
    elif cause == "vote_overflow":
        conn_cap = 2                                 # the middle frame votes for three rows, its neighbours for two
    elif cause == "n_written":
        def tamper(T): T["vote_headers"]["n_written"][1] = conn_cap + 1
    elif cause == "kf_max":
        def tamper(T): T["vote_headers"]["kf_max"][1] = n_kf
    elif cause == "voted_row":
        def tamper(T): T["vote_entries"]["kf"][1, 1] = n_kf
    elif cause == "n_best":
        def tamper(T): T["graph"]["n_best"][5] = 11
    elif cause == "best_row":
        def tamper(T): T["graph"]["best"][5, 1] = -1
    elif cause == "child_row":
        def tamper(T): T["children"][T["graph"]["child_offset"][5]] = n_kf
    elif cause == "child_slice":
        def tamper(T): T["graph"]["n_children"][5] = len(T["children"]) + 1
    elif cause == "parent_row":
        def tamper(T): T["graph"]["parent"][5] = n_kf
    elif cause == "parent_below":
        def tamper(T): T["graph"]["parent"][5] = -2
    elif cause == "slot_high":
        def tamper(T): T["kf_slots"][6][5] = n_points
    elif cause == "slot_low":
        def tamper(T): T["kf_slots"][8][4] = -2
    elif cause == "frame_slice":
        def tamper(T): T["subjects"]["slot_offset"][1] = len(T["frame_slots"])
    elif cause == "seen_index":
        mid_seen = [n_points]
    elif cause == "seen_negative":
        mid_seen = [-1]
    elif cause == "seen_slice":
        def tamper(T): T["frames"]["n_seen"][1] = len(T["seen"]) + 1
    elif cause == "n_keys":
        def tamper(T): T["n_keys"][7] = -1
    elif cause == "slots_null":
        def tamper(T): T["slots_state"][6] = 1
    elif cause == "slots_misaligned":
        def tamper(T): T["slots_state"][6] = 2
    else:
        raise KeyError(cause)
    if tamper is None:
        tamper = lambda T: None                      # the literal reading has nothing to say about the middle frame
    return _problem(B, [(a, []), (mid_slots, mid_seen), (a, [a[1]])], conn_cap=conn_cap, tamper=tamper, reaches=["refused"])


def directed_cases():
    """name -> problem.  problem["reaches"] is the census the case promises; tests/test_localmap_cpu.py asserts it, and that together
    the cases reach every one of EDGES."""
    out = {}
    B, s = voted_scene(6, [1, 3, 4])
    out["exhausted"] = _problem(B, [(s, [])], reaches=["stop:exhausted", "best:none", "child:none", "parent:absent", "seen:none",
                                                        "skip:frame_held"])
    B, s = voted_scene(90, range(80))
    B.kfs[0]["best"], B.kfs[1]["best"] = [85], [86]
    out["size_80_voted"] = _problem(B, [(s, [])], reaches=["stop:size@80voted"])
    for n in (81, 82):
        B, s = voted_scene(90, range(n))
        B.kfs[0]["best"] = [85]
        out["size_%d_voted" % n] = _problem(B, [(s, [])], reaches=["stop:size@%dvoted" % n])
    # 79 voted, a neighbour and a child appended in the first iteration, the second stops at 81.  (Three appended in one iteration
    # include the parent, and the parent ends the loop: that is the next case.)
    B, s = voted_scene(90, range(79))
    B.kfs[0]["best"], B.kfs[1]["best"] = [85], [87]
    _link(B, 0, 86)
    out["size_crossing"] = _problem(B, [(s, [])], reaches=["stop:size@crossing"])
    B, s = voted_scene(90, range(78))
    B.kfs[0]["best"] = [85]
    _link(B, 0, 86)
    _link(B, 87, 0)
    out["three_in_the_first_iteration"] = _problem(B, [(s, [])], reaches=["stop:parent@first"])
    B, s = voted_scene(8, [0, 1, 2])
    _link(B, 5, 1)
    _link(B, 6, 2)
    out["parent_later"] = _problem(B, [(s, [])], reaches=["stop:parent@later", "parent:absent"])
    B, s = voted_scene(8, [0, 1, 2])
    _link(B, 1, 0)
    out["parent_marked"] = _problem(B, [(s, [])], reaches=["parent:marked", "stop:exhausted"])
    B, s = voted_scene(8, [0, 1], bad=[5])
    _link(B, 5, 0)
    B.point([(5, 0, False, 1.0)])
    out["parent_bad"] = _problem(B, [(s, [])], reaches=["parent:bad", "stop:parent@first"])
    B, s = voted_scene(24, range(11))
    B.kfs[0]["best"] = list(range(1, 11))
    out["best_all_marked"] = _problem(B, [(s, [])], reaches=["best:all_marked"])
    B, s = voted_scene(24, [0], bad=range(1, 11))
    B.kfs[0]["best"] = list(range(1, 11))
    out["best_all_bad"] = _problem(B, [(s, [])], reaches=["best:all_bad"])
    B, s = voted_scene(24, [0, 1, 2, 3], bad=range(4, 10))
    B.kfs[0]["best"] = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12]
    out["best_tenth"] = _problem(B, [(s, [])], reaches=["best:tenth"])
    B, s = voted_scene(24, [0, 1, 2, 3], bad=range(4, 11))
    B.kfs[0]["best"] = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]
    out["best_eleventh"] = _problem(B, [(s, [])], reaches=["best:eleventh_eligible"])
    for pos in (0, 63, 64, 65):
        out["child_at_%d" % pos] = _children_case(pos)
    out["union_sizes"] = union_sizes_case()
    B, s = voted_scene(6, [0, 1, 2], n_keys=4)
    every = B.point([(k, 0, False, 1.0) for k in (0, 1, 2, 3)])
    B.kfs[0]["best"] = [3]
    out["point_everywhere"] = _problem(B, [(s + [every], [])], reaches=["point:everywhere"])
    B = C.MapBuilder()
    for k in range(HIGHEST_ROW + 1):
        B.keyframe(2 if k in (0, HIGHEST_ROW) else 0)
    s = [B.point([(HIGHEST_ROW, 0, False, 1.0)])]
    B.point([(0, 0, False, 1.0), (HIGHEST_ROW, 0, False, 1.0)])
    B.kfs[HIGHEST_ROW]["best"] = [0]
    out["highest_row"] = _problem(B, [(s, [])], reaches=["row:highest"])
    B, s = voted_scene(6, [0, 1])
    other = B.point([(1, 0, False, 1.0)])
    out["also_seen"] = _problem(B, [(s, [other]), (s, []), ([-1, -1], [other]), ([], [])],
                                reaches=["skip:seen", "seen:none", "status:empty", "skip:frame_held"])
    B, s = _caps_scene()
    n_kf, n_p = 5, 3 + 2 * 5
    for name, kc, pc in (("kf_cap_exact", n_kf, 64), ("kf_cap_over", n_kf - 1, 64), ("p_cap_exact", 16, n_p), ("p_cap_over", 16, n_p - 1)):
        out[name] = _problem(B, [(s, [])], kf_cap=kc, p_cap=pc, reaches=[name.replace("_cap_", "_cap:").replace("over", "over1")])
    B, s = voted_scene(6, [0, 1, 2])
    out["vote_overflow"] = _problem(B, [(s[:2], []), (s, []), (s[:1], [])], conn_cap=2, reaches=["vote:overflow", "refused"])
    for cause in REFUSAL_CAUSES:
        out["refused_" + cause] = refusal_case(cause)
    return out


def make_local_map(seed, n_kf=24, n_points=420, n_keys=150, n_frames=8):
    """a seeded map of np_covis.make_map with a spanning tree, ordered covisibles of 0 .. 14 rows and frames that hold draws of the
    points of a window of keyframes, some bad points and empty slots among them, and also-seen points"""
    scene = C.make_map(seed, n_kf=n_kf, n_points=n_points, n_keys=n_keys)
    rng = np.random.default_rng(seed + 1000)
    kfs, pts = scene["keyframes"], scene["points"]
    for k in range(1, n_kf):
        if rng.random() < 0.9:
            parent = int(rng.integers(0, k))
            kfs[k]["parent"] = parent
            kfs[parent].setdefault("children", []).append(k)
    for k in range(n_kf):
        near = [r for r in range(max(0, k - 9), min(n_kf, k + 10)) if r != k]
        kfs[k]["best"] = [int(b) for b in rng.permutation(near)[:int(rng.integers(0, 15))]]
    frames = []
    for _ in range(n_frames):
        c = int(rng.integers(0, n_kf))
        pool = [p for k in range(max(0, c - 2), min(n_kf, c + 3)) for p in kfs[k]["slots"] if p >= 0]
        slots = rng.choice(pool, min(len(pool), int(rng.integers(20, 120))), replace=False).tolist() if pool else []
        slots += [-1] * 5 + [i for i, P in enumerate(pts) if P["bad"]][:2]
        seen = rng.integers(0, len(pts), int(rng.integers(0, 12))).tolist()
        frames.append((slots, seen))
    return scene, frames
