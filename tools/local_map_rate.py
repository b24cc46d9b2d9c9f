#!/usr/bin/env python3
"""Times the local map of a tracked frame (orbfe_local_map_batch_device) on a KITTI-like resident scene.

    python tools/local_map_rate.py [--frames 256] [--iters 25] [--out profiles/local_map.json]

The scene (its actual numbers are printed): a chain of keyframes of 2 000 slots in a random pointer order, every point seen by about 18
neighbouring keyframes, parent = the keyframe before, ten best covisibles = the nearest rows; each frame holds 2 000 slots drawn from
the points around one keyframe, so that about 40 keyframes are voted and about 6 000 points are local.  Three things are timed with
events on one stream, warm, median of --iters (at least 20):
  (a) the local-map launch alone
  (b) the chain vote -> local map -> SearchLocalPoints (local_map.track_local_map_device)
  (c) the route without the kernel for the same chunk: the same vote, a download of its headers and entries, the table reading
      vectorised with numpy on the host, and the upload of the [S][p_cap] records (wall clock around the whole, device work included)
and the SearchLocalPoints launch that (a) feeds, alone.  (a) is set beside its byte bound: the slots of every local keyframe read once
plus the records read and written, over the 6.3 TB/s a streaming kernel reaches on this device.  The records of (a) are compared
with the host route's byte for byte.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refactored_orb_slam2_amd import _lib, covisibility, local_map, synth  # noqa: E402
from refactored_orb_slam2_amd.matcher import Matcher, make_frustum  # noqa: E402

HBM_TBS = 6.3


def build_scene(S, seed=3, n_keys=2000, per_kf=100, reach=10):
    rng = np.random.default_rng(seed)
    n_kf = S + 4 * reach + 40
    n_points = n_kf * per_kf
    order = rng.permutation(n_kf).astype(np.int32)
    slots = np.full((n_kf, n_keys), -1, np.int32)
    for k in range(n_kf):
        lo, hi = max(0, (k - reach) * per_kf), min(n_points, (k + reach) * per_kf)
        pick = rng.permutation(np.arange(lo, hi))[:int(0.9 * n_keys)]
        slots[k, rng.permutation(n_keys)[:len(pick)]] = pick
    kk, ii = np.nonzero(slots >= 0)
    pp = slots[kk, ii]
    by = np.lexsort((order[kk], pp))                      # a point's list in map order: ascending kf_order
    obs = np.zeros(len(by), _lib.MP_OBS_DTYPE)
    obs["kf"], obs["idx"] = kk[by], ii[by]
    recs = np.zeros(n_points, _lib.MP_POINT_DTYPE)
    counts = np.bincount(pp, minlength=n_points)
    recs["n_obs"], recs["obs_offset"] = counts, np.concatenate([[0], np.cumsum(counts)[:-1]])
    point_bad = (rng.random(n_points) < 0.01).astype(np.uint8)   # stale bad points stay in slots; the vote passes them over
    graph = np.zeros(n_kf, _lib.LM_GRAPH_DTYPE)
    graph["parent"] = np.arange(n_kf) - 1
    graph["child_offset"], graph["n_children"] = np.arange(n_kf), (np.arange(n_kf) < n_kf - 1)
    children = np.minimum(np.arange(n_kf) + 1, n_kf - 1).astype(np.int32)
    for k in range(n_kf):
        near = [r for d in range(1, 6) for r in (k - d, k + d) if 0 <= r < n_kf][:10]
        graph["n_best"][k], graph["best"][k, :len(near)] = len(near), near
    at = reach * 2 + 20
    frames = np.full((S, n_keys), -1, np.int32)
    seen = []
    for f in range(S):
        k = at + f
        pool = np.arange((k - reach) * per_kf, (k + reach) * per_kf)
        frames[f, :1500] = rng.choice(pool, 1500, replace=False)
        seen.append(rng.choice(pool, 30, replace=False))
    return dict(n_kf=n_kf, n_points=n_points, n_keys=n_keys, order=order, kf_bad=np.zeros(n_kf, np.uint8), slots=slots, obs=obs, recs=recs,
                point_bad=point_bad, graph=graph, children=children, frames=frames, seen=np.concatenate(seen).astype(np.int32))


def host_route(W, vh, ve, conn_cap, p_cap, records, out):
    """the table reading of tests/np_localmap.py for an accepted chunk, vectorised: returns n_points and fills out [S][p_cap]"""
    S = len(vh)
    n_out = np.zeros(S, np.int32)
    bad = W["point_bad"].astype(bool)
    for s in range(S):
        n_voted = int(vh["n_written"][s])
        local = ve["kf"][s, :n_voted].tolist()
        marked = set(local)
        for i in range(n_voted):
            if len(local) > 80:
                break
            G = W["graph"][local[i]]
            for b in G["best"][:G["n_best"]].tolist():
                if not W["kf_bad"][b] and b not in marked:
                    local.append(b); marked.add(b)
                    break
            for c in W["children"][G["child_offset"]:G["child_offset"] + G["n_children"]].tolist():
                if not W["kf_bad"][c] and c not in marked:
                    local.append(c); marked.add(c)
                    break
            if G["parent"] >= 0 and int(G["parent"]) not in marked:
                local.append(int(G["parent"]))
                break
        p = W["slots"][local].reshape(-1)
        p = p[p >= 0]
        p = p[~bad[p]]
        _, first = np.unique(p, return_index=True)
        p = p[np.sort(first)][:p_cap]
        skip = np.zeros(W["n_points"], bool)
        held = W["frames"][s]
        held = held[held >= 0]
        skip[held[~bad[held]]] = True
        skip[W["seen"][30 * s:30 * s + 30]] = True
        out[s, :len(p)] = records[p]
        out["skip"][s, :len(p)] = skip[p]
        n_out[s] = len(p)
    return n_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.iters = max(20, a.iters)
    import torch
    S, conn_cap, kf_cap, p_cap = a.frames, 64, 96, 8192
    W = build_scene(S)
    n_kf, n_points, n_keys = W["n_kf"], W["n_points"], W["n_keys"]

    def dev(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.uint8).reshape(len(x), -1).copy() if x.dtype.fields else x.copy()).cuda()

    w, h = 1241, 376
    k1 = np.zeros(2000, _lib.KP_DTYPE)
    rng = np.random.default_rng(9)
    k1["x"], k1["y"], k1["octave"] = rng.uniform(20, w - 20, 2000), rng.uniform(20, h - 20, 2000), rng.integers(0, 8, 2000)
    k1["size"], k1["angle"] = 31 * 1.2 ** k1["octave"], rng.uniform(0, 360, 2000)
    d1 = rng.integers(0, 256, (2000, 32)).astype(np.uint8)
    R_, t_ = synth.camera_pose(4)
    fr = make_frustum(R_, t_, 718.856, 718.856, 607.19, 185.2, 386.1448, (0, w, 0, h), 1.2, 8)
    records = np.zeros(n_points, _lib.MAP_POINT_DTYPE)
    records[:] = np.resize(synth.local_map(k1, d1, fr, 5, 4000), n_points)
    records["skip"] = 0

    d_slots_kf = dev(W["slots"].reshape(-1))
    table = np.zeros(n_kf, _lib.COV_KEYFRAME_DTYPE)
    table["n_keys"] = n_keys
    table["slots"] = np.uint64(d_slots_kf.data_ptr()) + np.uint64(4 * n_keys) * np.arange(n_kf, dtype=np.uint64)
    T = {"obs": dev(W["obs"]), "recs": dev(W["recs"]), "point_bad": dev(W["point_bad"]), "kf_order": dev(W["order"]), "kf_bad": dev(W["kf_bad"]),
         "graph": dev(W["graph"]), "children": dev(W["children"]), "table": dev(table), "records": dev(records)}
    f_slots, subjects = covisibility.pack_subjects([(f, -1, _lib.COV_VOTES) for f in W["frames"]])
    frames = np.zeros(S, _lib.LM_FRAME_DTYPE)
    frames["seen_offset"], frames["n_seen"] = 30 * np.arange(S), 30
    d_fslots, d_sub, d_frames, d_seen = dev(f_slots), dev(subjects), dev(frames), dev(W["seen"])
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
    vote_h, vote_e, lm_h = z(S, 32), z(S * conn_cap, 8), z(S, 32)
    local_kf, local_points, n_pts = z(S, kf_cap, dtype=torch.int32), z(S, p_cap, dtype=torch.int32), z(S, dtype=torch.int32)
    map_points, track = z(S, p_cap, 72), z(S, p_cap, 24)
    cap = 2048
    kps, desc = np.zeros((S, cap), _lib.KP_DTYPE), np.zeros((S, cap, 32), np.uint8)
    kps[:, :2000], desc[:, :2000] = k1, d1
    d_kps, d_desc = dev(kps.reshape(-1)).reshape(S, cap, 28), torch.from_numpy(desc).cuda()
    d_n = torch.full((S,), 2000, dtype=torch.int32, device="cuda")
    d_fr = dev(np.repeat(fr, S))
    blocked, assigned = z(S, cap), torch.full((S, cap), -1, dtype=torch.int32, device="cuda")
    ntm, nm = z(S, dtype=torch.int32), z(S, dtype=torch.int32)
    st = torch.cuda.Stream()
    m = Matcher()

    def vote():
        covisibility.covisibility_counts_device(T["obs"], T["recs"], T["point_bad"], T["kf_order"], T["kf_bad"], d_fslots, d_sub, conn_cap, vote_h,
                                                vote_e, stream=st)

    def lm():
        local_map.local_map_device(vote_h, vote_e, conn_cap, T["graph"], T["children"], T["table"], T["kf_bad"], T["point_bad"], d_fslots, d_sub,
                                   d_frames, d_seen, T["records"], kf_cap, p_cap, lm_h, local_kf, local_points, n_pts, map_points, stream=st)

    def lm_lists():   # the same launch without resident records: the lists alone, no gather
        local_map.local_map_device(vote_h, vote_e, conn_cap, T["graph"], T["children"], T["table"], T["kf_bad"], T["point_bad"], d_fslots, d_sub,
                                   d_frames, d_seen, None, kf_cap, p_cap, lm_h, local_kf, local_points, n_pts, None, stream=st)

    def search():
        blocked.zero_(); assigned.fill_(-1)
        m.search_local_points_batch(d_kps, d_desc, d_n, None, (0, w, 0, h), d_fr, map_points, n_pts, 1.0, 0.8, track, blocked, assigned, ntm, nm,
                                    stream=st)

    def chain():
        blocked.zero_(); assigned.fill_(-1)
        local_map.track_local_map_device(m, st, T, d_fslots, d_sub, d_frames, d_seen, conn_cap, kf_cap, vote_h, vote_e, lm_h, local_kf,
                                         local_points, n_pts, map_points, d_kps, d_desc, d_n, None, (0, w, 0, h), d_fr, 1.0, 0.8, track,
                                         blocked, assigned, ntm, nm)

    def timed(launch):
        out = []
        with torch.cuda.stream(st):
            for _ in range(3):
                launch()
            st.synchronize()
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                launch()
                e1.record(st)
                st.synchronize()
                out.append(e0.elapsed_time(e1) * 1000.0)
        return round(float(np.median(out)), 1), round(float(np.min(out)), 1)

    with torch.cuda.stream(st):
        vote()
        lm()
    st.synchronize()
    H = lm_h.cpu().numpy().view(_lib.LM_HEADER_DTYPE).reshape(-1)
    res = {"frames": S, "n_kf": n_kf, "n_points": n_points, "slots_per_keyframe": n_keys, "iters": a.iters,
           "status_ok": int((H["status"] == _lib.LM_OK).sum()), "n_voted_mean": round(float(H["n_voted"].mean()), 1),
           "n_local_kf_mean": round(float(H["n_local_kf"].mean()), 1), "n_local_points_mean": round(float(H["n_local_points"].mean()), 1),
           "stops": np.bincount(H["stop"], minlength=3).tolist()}
    print("scene:", json.dumps(res), flush=True)
    res["vote_us"] = timed(vote)
    res["a_local_map_us"] = timed(lm)
    res["a_lists_only_us"] = timed(lm_lists)
    res["search_local_points_us"] = timed(search)
    res["b_chain_us"] = timed(chain)
    nbytes = int(H["n_local_kf"].sum()) * n_keys * 4 + int(H["n_local_points"].sum()) * (72 * 2 + 4)
    res["a_bytes"] = nbytes
    res["a_byte_bound_us"] = round(nbytes / (HBM_TBS * 1e12) * 1e6, 1)

    # (c) the route without the kernel
    got_records = map_points.cpu().numpy().reshape(S, p_cap, 72).copy().view(_lib.MAP_POINT_DTYPE).reshape(S, p_cap)
    got_n = n_pts.cpu().numpy()
    host_out = np.zeros((S, p_cap), _lib.MAP_POINT_DTYPE)
    staged = torch.from_numpy(host_out.view(np.uint8).reshape(S, p_cap, 72))
    times = []
    for it in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            vote()
        st.synchronize()
        vh = vote_h.cpu().numpy().view(_lib.COV_HEADER_DTYPE).reshape(-1)
        ve = vote_e.cpu().numpy().view(_lib.COV_ENTRY_DTYPE).reshape(S, conn_cap)
        n_host = host_route(W, vh, ve, conn_cap, p_cap, records, host_out)
        up, up_n = staged.cuda(), torch.from_numpy(n_host).cuda()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    res["c_host_route_us"] = [round(float(np.median(times)), 1), round(float(np.min(times)), 1)]
    same = np.array_equal(got_n, n_host) and all(got_records[s, :got_n[s]].tobytes() == host_out[s, :got_n[s]].tobytes() for s in range(S))
    res["records_equal_host_route"] = bool(same)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    m.close()
    return 0 if same and res["status_ok"] == S else 1


if __name__ == "__main__":
    sys.exit(main())
