"""The C++ boundary of the essential-graph optimisation: orbfe_host::OptimizeEssentialGraph (csrc/host/Optimizer_hip.h) and
orbfe_host::CorrectLoopPropagate (csrc/host/LoopClosing_hip.h) on the mock Sim3 / KeyFrame / MapPoint / Map of tests/cpp/mock_egraph.

A map of 12 keyframes that exercises every rule of the marshal: a bad keyframe, a loop connection below minFeat, the (current, loop)
pair below minFeat (still inserted), a covisible neighbour that is the parent, one that is a child, one that is a loop edge, one
already inserted as a loop connection, one below minFeat, one that is bad, a point already corrected by the current keyframe, a bad
point and a point whose reference keyframe is bad.  The marshalled lists are compared with a plain Python restatement of
Optimizer.cc:787-985 and need no GPU; with one, the applied poses and points are compared with the reading (tests/np_egraph.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_egraph as G
from tests import np_pose as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_egraph", "_build", "test_egraph_dropin")
MIN_FEAT = 100
NK, LOOP, CUR, BAD = 12, 1, 11, 6
MNID = [3 * k + 1 for k in range(NK)]


@pytest.fixture(scope="module")
def exe():
    _lib.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_egraph")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return EXE


def make_map(fix_scale):
    """The map as plain Python data: keyframes (pose, parent, loop edges, weights), the two pose maps, the loop connections, points"""
    rng = np.random.default_rng(31)
    base = G.make_scene(31, n_kf=NK, band=1, fix_scale=fix_scale, n_corrected=3, loop_kf=LOOP)
    V = base["vertices"]
    kfs = []
    for k in range(NK):
        q, t = V["Snc"][k]["q"], V["Snc"][k]["t"]
        R = np.array(P.quat_to_matrix([float(c) for c in q]))
        pose = np.concatenate([R, t.reshape(3, 1)], 1).astype(np.float32)
        kfs.append(dict(mnId=MNID[k], bad=int(k == BAD), pose=pose, parent=k - 1, loops=[], w={}))
    kfs[7]["parent"], kfs[4]["parent"] = 5, 7                               # 6 is bad; 4 is a child of 7 with a smaller id
    kfs[8]["loops"], kfs[3]["loops"] = [3], [8]

    def w(a, b, v):
        kfs[a]["w"][b] = kfs[b]["w"][a] = v

    for k in range(1, NK):
        w(k, k - 1, 200)                                                    # the parent (or, for 4 and 7, a plain neighbour)
    for k in range(2, NK):
        w(k, k - 2, 120)
    w(8, 3, 150)                                                            # a loop edge
    w(9, 4, 90)                                                             # below minFeat
    w(11, 1, 30)                                                            # (current, loop) below minFeat: still a loop connection
    w(11, 2, 150)                                                           # a loop connection, and a covisible neighbour of 11
    w(11, 0, 40)                                                            # a loop connection below minFeat: dropped
    w(10, 1, 120)
    w(10, 2, 50)                                                            # dropped
    w(7, 4, 140)                                                            # a child
    corrected = {k: V["Scw"][k].copy() for k in (9, 10, 11)}
    noncorrected = {k: V["Snc"][k].copy() for k in (9, 10, 11)}
    conn = {11: [1, 2, 0], 10: [1, 2]}
    pts = []
    for p in range(30):
        ref = int(rng.integers(0, NK))
        if p == 3:
            ref = BAD
        by, cref = (MNID[CUR], MNID[10]) if p in (5, 6) else (0, 0)
        other = (ref + 1) % NK
        pts.append(dict(mnId=100 + p, bad=int(p in (8, 9)), pos=(rng.normal(size=3) * 6).astype(np.float32), ref=ref, by=by, cref=cref,
                        obs=sorted({ref, other})))
    return dict(kfs=kfs, corrected=corrected, noncorrected=noncorrected, conn=conn, pts=pts, fix_scale=fix_scale)


def write_map(path, m, propagate=None):
    b = bytearray()
    i32 = lambda *v: b.extend(struct.pack(f"<{len(v)}i", *[int(x) for x in v]))
    sim3 = lambda rec: b.extend(np.concatenate([rec["q"], rec["t"], [rec["s"]]]).astype("<f8").tobytes())
    i32(m["fix_scale"], NK)
    for k, K in enumerate(m["kfs"]):
        i32(K["mnId"], K["bad"])
        b.extend(K["pose"].astype("<f4").tobytes())
        i32(K["parent"], len(K["loops"]), *K["loops"], len(K["w"]))
        for j, v in sorted(K["w"].items()):
            i32(j, v)
        for table in (m["corrected"], m["noncorrected"]):
            i32(int(k in table))
            if k in table:
                sim3(table[k])
    i32(LOOP, CUR, len(m["conn"]))
    for a, lst in m["conn"].items():
        i32(a, len(lst), *lst)
    i32(len(m["pts"]))
    for Q in m["pts"]:
        i32(Q["mnId"], Q["bad"])
        b.extend(Q["pos"].astype("<f4").tobytes())
        i32(Q["ref"], Q["by"], Q["cref"], len(Q["obs"]), *Q["obs"])
    if propagate is not None:
        i32(len(propagate[0]), *propagate[0])
        sim3(propagate[1])
    open(path, "wb").write(bytes(b))


def restate_marshal(m):
    """Optimizer.cc:787-985 and :1016-1034 in plain Python: (mnIds of the rows, vertices, loop-connection edges as a set, normal edges
    in order, ref, points)"""
    kfs = m["kfs"]
    rows = sorted((k for k in range(NK) if not kfs[k]["bad"]), key=lambda k: kfs[k]["mnId"])
    row = {k: r for r, k in enumerate(rows)}
    V = np.zeros(len(rows), G.VERTEX_DTYPE)
    for r, k in enumerate(rows):
        if k in m["corrected"]:
            V["Scw"][r] = m["corrected"][k]
        else:
            T = kfs[k]["pose"].astype(np.float64)
            V["Scw"][r] = G._sim3_record(T[:, :3], T[:, 3], 1.0)
        V["Snc"][r] = m["noncorrected"][k] if k in m["noncorrected"] else V["Scw"][r]
        V["fixed"][r] = int(k == LOOP)
    inserted, loop_edges, normal = set(), set(), []
    for a, lst in m["conn"].items():
        for j in lst:
            if (a != CUR or j != LOOP) and kfs[a]["w"].get(j, 0) < MIN_FEAT:
                continue
            if a in row and j in row:
                loop_edges.add((row[a], row[j], 1))
            inserted.add((min(kfs[a]["mnId"], kfs[j]["mnId"]), max(kfs[a]["mnId"], kfs[j]["mnId"])))
    for k in rows:
        K = kfs[k]
        par = K["parent"] if K["parent"] >= 0 else None
        children = {c for c in range(NK) if kfs[c]["parent"] == k}
        if par is not None and par in row:
            normal.append((row[k], row[par], 0))
        for l in sorted(K["loops"], key=lambda j: kfs[j]["mnId"]):
            if kfs[l]["mnId"] < K["mnId"] and l in row:
                normal.append((row[k], row[l], 0))
        cov = sorted((j for j, v in K["w"].items() if v >= MIN_FEAT), key=lambda j: (-K["w"][j], kfs[j]["mnId"]))
        for j in cov:
            if j == par or j in children or j in K["loops"]:
                continue
            if kfs[j]["bad"] or not kfs[j]["mnId"] < K["mnId"]:
                continue
            if (min(K["mnId"], kfs[j]["mnId"]), max(K["mnId"], kfs[j]["mnId"])) in inserted:
                continue
            normal.append((row[k], row[j], 0))
    id_row = {kfs[k]["mnId"]: r for k, r in row.items()}
    ref = np.full(len(m["pts"]), -1, np.int32)
    pos = np.zeros((len(m["pts"]), 3), np.float32)
    for p, Q in enumerate(m["pts"]):
        if Q["bad"]:
            continue
        idr = Q["cref"] if Q["by"] == MNID[CUR] else kfs[Q["ref"]]["mnId"]
        if idr in id_row:
            ref[p] = id_row[idr]
            pos[p] = Q["pos"]
    return [kfs[k]["mnId"] for k in rows], V, loop_edges, normal, ref, pos


def read_marshal(path):
    raw = open(path, "rb").read()
    n = struct.unpack_from("<i", raw, 0)[0]
    ids = list(struct.unpack_from(f"<{n}i", raw, 4))
    o = 4 + 4 * n
    V = np.frombuffer(raw, _lib.EG_VERTEX_DTYPE, n, o)
    o += 136 * n
    ne = struct.unpack_from("<i", raw, o)[0]
    E = np.frombuffer(raw, _lib.EG_EDGE_DTYPE, ne, o + 4)
    o += 4 + 12 * ne
    npt = struct.unpack_from("<i", raw, o)[0]
    ref = np.frombuffer(raw, np.int32, npt, o + 4)
    pos = np.frombuffer(raw, np.float32, 3 * npt, o + 4 + 4 * npt).reshape(npt, 3)
    assert o + 4 + 16 * npt == len(raw)
    return ids, V, E, ref, pos


@pytest.mark.parametrize("fix_scale", [False, True])
def test_marshalled_lists_against_the_restatement(exe, tmp_path, fix_scale):
    m = make_map(fix_scale)
    write_map(tmp_path / "in.bin", m)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "marshal"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    ids, V, E, ref, pos = read_marshal(tmp_path / "out.bin")
    want_ids, wV, loop_edges, normal, wref, wpos = restate_marshal(m)
    assert ids == want_ids == sorted(want_ids) and MNID[BAD] not in ids and len(ids) == NK - 1
    assert V["fixed"].tolist() == wV["fixed"].tolist() and V["fixed"].sum() == 1
    for name in ("Scw", "Snc"):
        assert G.sim3_units(V[name], wV[name]) <= 2.0 ** -20, name            # Quaternion(Matrix3) twice: rounding only
    for k in (9, 10, 11):                                                   # an entry of the pose maps is copied, never converted
        r_ = want_ids.index(MNID[k])
        assert V["Scw"][r_].tobytes() == m["corrected"][k].tobytes() and V["Snc"][r_].tobytes() == m["noncorrected"][k].tobytes()
    got = [tuple(int(x) for x in e) for e in E]
    n_loop = len(loop_edges)
    assert set(got[:n_loop]) == loop_edges and got[n_loop:] == normal       # LoopConnections is keyed by pointer: a set; the rest in order
    row = {i: r_ for r_, i in enumerate(want_ids)}
    assert (row[MNID[11]], row[MNID[1]], 1) in loop_edges and (row[MNID[11]], row[MNID[0]], 1) not in loop_edges
    assert (row[MNID[10]], row[MNID[2]], 1) not in loop_edges and n_loop == 3
    assert (row[MNID[8]], row[MNID[3]], 0) in normal and normal.count((row[MNID[8]], row[MNID[3]], 0)) == 1
    assert (row[MNID[11]], row[MNID[2]], 0) not in normal and (row[MNID[7]], row[MNID[4]], 0) not in normal
    assert (row[MNID[4]], row[MNID[7]], 0) in normal and (row[MNID[9]], row[MNID[4]], 0) not in normal
    assert not any(MNID[BAD] in (want_ids[a], want_ids[b]) for a, b, _ in got)
    assert ref.tolist() == wref.tolist() and np.array_equal(pos, wpos)
    assert ref[3] == -1 and ref[8] == -1 and ref[5] == row[MNID[10]]


def _read_state(raw, o, marks):
    kf, pt = [], []
    for _ in range(NK):
        calls = struct.unpack_from("<i", raw, o)[0]
        kf.append((calls, np.frombuffer(raw, np.float32, 12, o + 4).copy()))
        o += 52
    step = 36 + (8 if marks else 0)
    while o < len(raw):
        calls = struct.unpack_from("<i", raw, o)[0]
        f = np.frombuffer(raw, np.float32, 8, o + 4).copy()
        mk = struct.unpack_from("<2i", raw, o + 36) if marks else (0, 0)
        pt.append(dict(calls=calls, pos=f[:3], dist=f[3:5], normal=f[5:8], by=mk[0], cref=mk[1]))
        o += step
    return kf, pt


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [False, True])
def test_applied_poses_and_points_against_the_reading(exe, tmp_path, fix_scale):
    m = make_map(fix_scale)
    write_map(tmp_path / "in.bin", m)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    kf, pt = _read_state(open(tmp_path / "out.bin", "rb").read(), 0, False)
    ids, V, loop_edges, normal, ref, pos = restate_marshal(m)
    E = np.array(sorted(loop_edges) + normal, G.EDGE_DTYPE)
    want = G.essential_graph(V, E, fix_scale)
    moved = G.correct_points(pos, ref, np.ascontiguousarray(V["Scw"]), want["sim3"])
    rows = [k for k in range(NK) if k != BAD]
    poses = np.stack([kf[k][1] for k in rows])
    up = G.pose_units(poses, want["poses"])
    got_pts = np.stack([Q["pos"] for Q in pt])
    live = ref >= 0
    ux = G.point_units(got_pts[live], moved[live])
    print(f"egraph drop-in, fix_scale {fix_scale}: poses {up:.4f} units, points {ux:.4f} units (bound {G.BOUND_UNITS[fix_scale]})")
    assert [kf[k][0] for k in range(NK)] == [0 if k == BAD else 1 for k in range(NK)]
    assert kf[BAD][1].tobytes() == m["kfs"][BAD]["pose"].tobytes()
    assert [Q["calls"] for Q in pt] == [int(x) for x in live]
    for p in np.flatnonzero(~live):
        assert pt[p]["pos"].tobytes() == m["pts"][p]["pos"].tobytes()
    for p in np.flatnonzero(live):                                        # the batch refresh ran: a mean of unit vectors, a distance range
        assert 0 < np.linalg.norm(pt[p]["normal"]) <= 1 + 1e-5 and 0 < pt[p]["dist"][0] < pt[p]["dist"][1]
    assert up <= G.BOUND_UNITS[fix_scale] and ux <= G.BOUND_UNITS[fix_scale]


@pytest.mark.gpu
def test_correct_loop_propagate(exe, tmp_path):
    m = make_map(False)
    Scw = m["corrected"][CUR]
    m["corrected"], m["noncorrected"] = {}, {}
    connected = [10, 9, 8, CUR]
    write_map(tmp_path / "in.bin", m, propagate=(connected, Scw))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "propagate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    n_moved = struct.unpack_from("<i", raw, 0)[0]
    o, tables = 4, []
    for _ in range(2):
        n = struct.unpack_from("<i", raw, o)[0]
        o += 4
        t = {}
        for _ in range(n):
            t[struct.unpack_from("<i", raw, o)[0]] = np.frombuffer(raw, G.SIM3_DTYPE, 1, o + 4)[0].copy()
            o += 68
        tables.append(t)
    corrected, noncorrected = tables
    kf, pt = _read_state(raw, o, True)
    assert sorted(corrected) == sorted(noncorrected) == sorted(MNID[k] for k in connected)
    assert corrected[MNID[CUR]].tobytes() == Scw.tobytes()
    for k in connected:                                                   # NonCorrected is Sim3(Riw, tiw, 1); Corrected is Sic * Scw
        T = m["kfs"][k]["pose"].astype(np.float64)
        assert G.sim3_units(noncorrected[MNID[k]], G._sim3_record(T[:, :3], T[:, 3], 1.0)) <= 2.0 ** -20
        if k != CUR:
            Tc = m["kfs"][CUR]["pose"].astype(np.float64)
            Tic_R = T[:, :3] @ Tc[:, :3].T
            Tic_t = T[:, 3] - Tic_R @ Tc[:, 3]
            sic = G._cols(G._sim3_record(Tic_R, Tic_t, 1.0))
            q, t, s = G.O.sim3_mul(sic, G._cols(Scw))
            want = np.zeros((), G.SIM3_DTYPE)
            want["q"], want["t"], want["s"] = q, t, s
            assert G.sim3_units(corrected[MNID[k]], want) <= 64.0          # the float product Tiw * Twc: a few float ulps at |t| ~ 10
    # the points: each through the tables of the first keyframe (in pointer order, so either of its observers) that reached it
    order = sorted(corrected)
    a = np.array([noncorrected[i] for i in order], G.SIM3_DTYPE)
    b = np.array([corrected[i] for i in order], G.SIM3_DTYPE)
    count = 0
    for p, Q in enumerate(m["pts"]):
        seen = [k for k in Q["obs"] if k in connected]
        if Q["bad"] or Q["by"] == MNID[CUR] or not seen:
            assert pt[p]["calls"] == 0 and pt[p]["pos"].tobytes() == Q["pos"].tobytes()
            continue
        count += 1
        assert pt[p]["calls"] == 1 and pt[p]["by"] == MNID[CUR] and pt[p]["cref"] in [MNID[k] for k in seen]
        want = G.correct_points(Q["pos"][None], [order.index(pt[p]["cref"])], a, b)
        assert G.point_units(pt[p]["pos"], want) <= 1.0
    assert n_moved == count > 0
    for k in range(NK):
        if k in connected:
            assert kf[k][0] == 1 and G.pose_units(kf[k][1], G.poses_of(corrected[MNID[k]], False)) <= 1.0
        else:
            assert kf[k][0] == 0 and kf[k][1].tobytes() == m["kfs"][k]["pose"].tobytes()
