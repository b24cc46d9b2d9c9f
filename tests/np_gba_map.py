"""The yardstick of the map update behind the global bundle adjustment (orbfe_gba_update_map, tests/test_gba_map_*.py): two float32
numpy readings of LoopClosing::RunGlobalBundleAdjustment's block L/src/LoopClosing.cc:648-703 (L/ = Source/Libraries/ORB_SLAM2/) with
KeyFrame::SetPose (L/src/KeyFrame.cc:75-88), and a seeded scene builder.  A helper, not a test file.

The reading of cv::Mat (OpenCV's small-matrix gemm, as csrc/frustum_kernels.hip:96-98 and csrc/host/ORBmatcher.cc:56-75 read it): a
product is a float dot in index order, the epilogue alpha * dot + beta * addend is done in double and rounded once, a zero or one that
takes part in a 4 x 4 dot is multiplied and added like any other term.  numpy's float32 array arithmetic rounds every product and every
sum to float32 and contracts nothing, so the expressions below are that reading.  A pose is 12 floats, the rows of [R | t]; the fourth
row of a 4 x 4 operand is 0 0 0 1, and the fourth row of a product is not kept (with finite operands it is 0 0 0 1 again).

literal()  the reference read literally: a queue from the origins, child sets, the parent's SetPose behind its child loop, then the
           points in map order.  Where the reference would read an empty mTcwGBA (a keyframe that is not optimised and whose parent
           chain ends in no optimised keyframe) the keyframe is left as it is -- the deviation include/orbfe.h states.
rule()     what the device evaluates: a rule per keyframe, in rounds -- an optimised keyframe takes its row, any other one follows
           its parent in the round after the parent is done --, then a rule per point.  It also states what the device form does
           with rows that are out of range, which literal() does not take.
The two agree to the byte on every scene of SCENES (tests/test_gba_map_cpu.py)."""
from __future__ import annotations

import collections
import functools

import numpy as np

F32 = np.float32
OPTIMISED, PROPAGATED, UNREACHED = 0, 1, 2
KEYFRAME_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Twc", "<f4", (12,)), ("Cw", "<f4", (3,)), ("status", "<i4")])
RESULT_FIELDS = ("n_optimised", "n_propagated", "n_unreached", "n_taken", "n_moved", "n_left", "rounds")


# ---- the arithmetic, on rows: every argument is (n, 12) / (n, 3) float32
def mul(A, B):
    """A * B of 4 x 4 operands whose fourth rows are 0 0 0 1"""
    C = np.empty_like(A)
    for r in range(3):
        for c in range(4):
            s = A[:, 4 * r] * B[:, c]
            s = s + A[:, 4 * r + 1] * B[:, 4 + c]
            s = s + A[:, 4 * r + 2] * B[:, 8 + c]
            s = s + A[:, 4 * r + 3] * (F32(1) if c == 3 else F32(0))
            C[:, 4 * r + c] = s
    return C


def set_pose(Tcw, half_baseline):
    """KeyFrame::SetPose: (Twc, Cw) of Tcw"""
    hb = F32(half_baseline)
    Twc = np.empty_like(Tcw)
    Cw = np.empty((len(Tcw), 3), F32)
    t = [Tcw[:, 3], Tcw[:, 7], Tcw[:, 11]]
    for r in range(3):
        for c in range(3):
            Twc[:, 4 * r + c] = Tcw[:, 4 * c + r]                                   # Rwc = Rcw.t()
        d = Tcw[:, r] * t[0]
        d = d + Tcw[:, 4 + r] * t[1]
        d = d + Tcw[:, 8 + r] * t[2]
        Twc[:, 4 * r + 3] = (d.astype(np.float64) * -1.0).astype(F32)               # Ow = -Rwc * tcw
    for r in range(3):                                                              # Cw = Twc * (hb, 0, 0, 1)^T
        s = Twc[:, 4 * r] * hb
        s = s + Twc[:, 4 * r + 1] * F32(0)
        s = s + Twc[:, 4 * r + 2] * F32(0)
        s = s + Twc[:, 4 * r + 3] * F32(1)
        Cw[:, r] = (s.astype(np.float64) * 1.0).astype(F32)
    return Twc, Cw


def gemm3(T, X):
    """R * x + t with [R | t] = T: the float dot, then the epilogue in double"""
    out = np.empty_like(X)
    for r in range(3):
        d = T[:, 4 * r] * X[:, 0]
        d = d + T[:, 4 * r + 1] * X[:, 1]
        d = d + T[:, 4 * r + 2] * X[:, 2]
        out[:, r] = (d.astype(np.float64) * 1.0 + T[:, 4 * r + 3].astype(np.float64) * 1.0).astype(F32)
    return out


def move_points(Tcw_bef, Twc_new, X):
    return gemm3(Twc_new, gemm3(Tcw_bef, X))


def _result(status, n_taken, n_moved, n_left, rounds):
    return dict(n_optimised=int((status == OPTIMISED).sum()), n_propagated=int((status == PROPAGATED).sum()),
                n_unreached=int((status == UNREACHED).sum()), n_taken=int(n_taken), n_moved=int(n_moved), n_left=int(n_left),
                rounds=int(rounds))


def _records(Tcw, hb, status):
    rec = np.zeros(len(Tcw), KEYFRAME_DTYPE)
    rec["Tcw"] = Tcw
    rec["Twc"], rec["Cw"] = set_pose(Tcw, hb)
    rec["status"] = status
    return rec


# ---- the reference read literally
def literal(s):
    """(keyframes, points_out, result) of a scene whose rows are all in range.  `rounds` is the depth of the deepest propagated
    keyframe below its optimised ancestor, which is what the queue's order makes of it."""
    poses, parent, row, hb = s["poses"], s["parent"], s["kf_gba_row"], s["half_baseline"]
    n = len(poses)
    Tcw = poses.copy()
    Twc, _ = set_pose(Tcw, hb)                      # what GetPoseInverse() returns before the walk
    TcwGBA = {k: s["gba_poses"][row[k]].copy() for k in range(n) if row[k] >= 0}
    flag = [row[k] >= 0 for k in range(n)]          # mnBAGlobalForKF == nLoopKF
    childs = [[] for _ in range(n)]
    for k in range(n):
        if parent[k] >= 0:
            childs[parent[k]].append(k)
    status = np.full(n, UNREACHED, np.int32)
    depth = np.zeros(n, np.int64)
    bef = Tcw.copy()
    queue = collections.deque(k for k in range(n) if parent[k] < 0)      # mvpKeyFrameOrigins
    while queue:
        k = queue[0]
        Twc_k = Twc[k:k + 1].copy()
        for c in childs[k]:
            if not flag[c] and k in TcwGBA:         # without the second test the reference reads an empty mTcwGBA
                Tchildc = mul(Tcw[c:c + 1], Twc_k)
                TcwGBA[c] = mul(Tchildc, TcwGBA[k][None])[0]
                flag[c] = True
                status[c] = PROPAGATED
                depth[c] = depth[k] + 1
            queue.append(c)
        if k in TcwGBA:
            bef[k] = Tcw[k]                          # mTcwBefGBA
            Tcw[k] = TcwGBA[k]                       # SetPose(mTcwGBA)
            Twc[k:k + 1], _ = set_pose(Tcw[k:k + 1], hb)
            if status[k] != PROPAGATED:
                status[k] = OPTIMISED
        queue.popleft()
    X, prow, ref = s["points"], s["point_gba_row"], s["ref"]
    out = X.copy()
    taken = moved = left = 0
    for p in range(len(X)):
        if ref[p] < 0 and prow[p] < 0:              # isBad(): the scene gives a bad point neither a row nor a reference keyframe
            left += 1
        elif prow[p] >= 0:
            out[p] = s["gba_points"][prow[p]]
            taken += 1
        elif not flag[ref[p]]:
            left += 1
        else:
            r = ref[p]
            out[p] = move_points(bef[r:r + 1], Twc[r:r + 1], X[p:p + 1])[0]
            moved += 1
    return _records(Tcw, hb, status), out, _result(status, taken, moved, left, depth.max() if n else 0)


# ---- the rule per keyframe and per point
def rule(s):
    """(keyframes, points_out, result) of any scene, rows out of range included (the device form's rules)"""
    poses, parent, row, hb = s["poses"], s["parent"], s["kf_gba_row"], s["half_baseline"]
    n, G = len(poses), len(s["gba_poses"])
    opt = (row >= 0) & (row < G)
    pending = (row < 0) & (parent >= 0) & (parent < n)
    Tcw = poses.copy()
    Tcw[opt] = s["gba_poses"][row[opt]]
    status = np.full(n, UNREACHED, np.int32)
    status[opt] = OPTIMISED
    Twc_old, _ = set_pose(poses, hb)
    Tchildc = np.zeros_like(poses)
    Tchildc[pending] = mul(poses[pending], Twc_old[parent[pending]])
    # the children of every keyframe, so that a round costs what it finishes
    kids = np.flatnonzero(pending)
    order = kids[np.argsort(parent[kids], kind="stable")]
    start = np.searchsorted(parent[order], np.arange(n + 1), "left")
    frontier = np.flatnonzero(opt)
    rounds = 0
    while True:
        if len(frontier) == 0:
            break
        cnt = start[frontier + 1] - start[frontier]
        if cnt.sum() == 0:
            break
        idx = np.concatenate([order[start[f]:start[f + 1]] for f in frontier[cnt > 0]])
        Tcw[idx] = mul(Tchildc[idx], Tcw[parent[idx]])
        status[idx] = PROPAGATED
        frontier = idx
        rounds += 1
    X, prow, ref = s["points"], s["point_gba_row"], s["ref"]
    Q = len(s["gba_points"])
    out = X.copy()
    take = (prow >= 0) & (prow < Q)
    out[take] = s["gba_points"][prow[take]]
    has_ref = (prow < 0) & (ref >= 0) & (ref < n)
    move = has_ref.copy()
    move[has_ref] = status[ref[has_ref]] != UNREACHED
    rec = _records(Tcw, hb, status)
    out[move] = move_points(poses[ref[move]], rec["Twc"][ref[move]], X[move])
    return rec, out, _result(status, take.sum(), move.sum(), len(X) - take.sum() - move.sum(), rounds)


# ---- scenes
def _poses(rng, n):
    """n poses: a rotation about a random axis by up to 0.6 rad, a translation of a few metres"""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-0.6, 0.6, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1],
                                                                             axis[:, 0])
    R = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    T = np.concatenate([R, rng.uniform(-5, 5, (n, 3, 1))], axis=2)
    return np.ascontiguousarray(T.reshape(n, 12).astype(F32))


def make_scene(seed, parent, optimised, n_points, shuffle=True):
    """A scene of len(parent) keyframes.  parent: the parent of every keyframe in the caller's labels (-1: an origin); optimised: which
    ones the adjustment saw.  The rows are the labels shuffled, so a parent's row may lie behind its child's; the rows of the two
    adjustment tables are shuffled too and each table has one row nobody names.  Points cycle through the three kinds -- optimised,
    carried by a reference keyframe drawn from all keyframes (the unreached ones included), bad -- in shuffled order."""
    rng = np.random.default_rng(seed)
    parent = np.asarray(parent, np.int64)
    optimised = np.asarray(optimised, bool)
    n = len(parent)
    perm = rng.permutation(n) if shuffle else np.arange(n)          # label -> row
    par = np.full(n, -1, np.int32)
    par[perm] = np.where(parent >= 0, perm[np.maximum(parent, 0)], -1)
    opt = np.zeros(n, bool)
    opt[perm] = optimised
    poses = _poses(rng, n)
    n_opt = int(opt.sum())
    gba_poses = _poses(rng, n_opt + 1)
    kf_row = np.full(n, -1, np.int32)
    kf_row[opt] = rng.permutation(n_opt + 1)[:n_opt]
    # the adjustment moves a pose a little: start from the old pose of the keyframe that owns the row
    gba_poses[kf_row[opt]] = (poses[opt] + rng.normal(0, 0.01, (n_opt, 12))).astype(F32)
    kind = rng.permutation(np.arange(n_points) % 3)                 # 0 optimised, 1 carried, 2 bad
    n_take = int((kind == 0).sum())
    points = rng.uniform(-20, 20, (n_points, 3)).astype(F32)
    gba_points = rng.uniform(-20, 20, (n_take + 1, 3)).astype(F32)
    prow = np.full(n_points, -1, np.int32)
    prow[kind == 0] = rng.permutation(n_take + 1)[:n_take]
    ref = np.full(n_points, -1, np.int32)
    ref[kind != 2] = rng.integers(0, n, int((kind != 2).sum()))     # an optimised point has a reference keyframe as well
    return dict(poses=poses, parent=par, kf_gba_row=kf_row, gba_poses=gba_poses, half_baseline=F32(0.2685), points=points,
                point_gba_row=prow, ref=ref, gba_points=gba_points)


def chain(n):
    """labels: an optimised origin 0 and a chain of n keyframes that are not optimised under it"""
    return list(range(-1, n)), [True] + [False] * n


def fan(n):
    return [-1] + [0] * n, [True] + [False] * n


def mixed():
    """several origins, flat fans, chains, an optimised child under a propagated parent with a propagated child below it, an origin
    that is not optimised (with a chain and an optimised child under it), and two keyframes that are each other's parent"""
    parent, optimised = [], []

    def add(p, o):
        parent.append(p)
        optimised.append(o)
        return len(parent) - 1
    a = add(-1, True)                                   # origin 1: a fan of optimised and propagated children
    for i in range(9):
        add(a, i % 2 == 0)
    b = add(-1, True)                                   # origin 2: a chain of 5, then an optimised keyframe, then a chain of 3
    k = b
    for i in range(5):
        k = add(k, False)
    k = add(k, True)                                    # optimised child under a propagated parent ...
    for i in range(3):
        k = add(k, False)                               # ... with propagated keyframes below it
    f = add(k, False)
    for i in range(7):
        add(f, False)                                   # a fan at the end of the chain
    c = add(-1, False)                                  # origin 3 is not optimised: unreached, and so is the chain under it
    k = c
    for i in range(3):
        k = add(k, False)
    o = add(c, True)                                    # an optimised keyframe under the unreached origin
    add(o, False)                                       # and its child, which is reached through it
    x = add(-2, False)                                  # a cycle of two: patched below
    y = add(x, False)
    parent[x] = y
    d = add(-1, True)                                   # origin 4, alone
    assert d == len(parent) - 1
    return parent, optimised


# name -> (seed, (parent, optimised), points).  The point counts stand on the edges of a wave (64) and a workgroup (256).
SCENES = {
    "single": (1, ([-1], [True]), 0),
    "chain_1": (2, chain(1), 1),
    "chain_2": (3, chain(2), 63),
    "chain_63": (4, chain(63), 64),
    "chain_64": (5, chain(64), 65),
    "chain_65": (6, chain(65), 256),
    "chain_1025": (7, chain(1025), 257),
    "fan_1025": (8, fan(1025), 1025),
    "two_origins": (9, ([-1, -1, 0, 1, 2, 3, 0], [True, True, False, False, False, False, False]), 65),
    "mixed": (10, mixed(), 1025),
    "unoptimised_origin": (11, ([-1, 0, 1, -1, 3], [False, False, False, True, False]), 64),
    "cycle": (12, ([1, 0, -1, 2], [False, False, True, False]), 64),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """the scene of a name, built once and shared; treat it as read-only"""
    seed, (parent, optimised), n_points = SCENES[name]
    s = make_scene(seed, parent, optimised, n_points)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def reading(name):
    """rule() of a scene, computed once and shared; treat it as read-only"""
    return rule(scene(name))


def out_of_range_scene():
    """the mixed scene with rows only the device form takes: parents and reference keyframes outside 0 .. n_kf - 1, rows of the two
    tables at and beyond their ends, and negative rows other than -1"""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene("mixed").items()}
    n, G, Q = len(s["poses"]), len(s["gba_poses"]), len(s["gba_points"])
    prop = np.flatnonzero(s["kf_gba_row"] < 0)
    opt = np.flatnonzero(s["kf_gba_row"] >= 0)
    s["parent"][prop[0]] = n
    s["parent"][prop[1]] = 2 ** 31 - 1
    s["parent"][prop[2]] = -7
    s["kf_gba_row"][opt[0]] = G
    s["kf_gba_row"][opt[1]] = 2 ** 31 - 1
    s["kf_gba_row"][prop[3]] = -2 ** 31
    s["ref"][0:3] = (n, 2 ** 31 - 1, -9)
    taken = np.flatnonzero(s["point_gba_row"] >= 0)
    s["point_gba_row"][taken[0]] = Q
    s["point_gba_row"][taken[1]] = 2 ** 31 - 1
    s["point_gba_row"][np.flatnonzero(s["point_gba_row"] < 0)[0]] = -5
    return s
