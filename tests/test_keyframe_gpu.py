"""GPU suite of the keyframe decision and the close stereo points (keyframe_kernels.hip behind orbfe_keyframe_insertion*) against the
reading of tests/np_keyframe.py, which tests/test_keyframe_cpu.py ties to the literal loop and to a second truth table.  Everything is
compared byte for byte: headers, the new point records, their indices, n_new, depth_selected and the assigned rows.  Every output array
starts as a canary: what is not to be written must keep it, and guard rows on both sides of every device array must survive.  The
shapes are the directed frames of np_keyframe.directed_cases in the host form and the device form, each alone and at positions 0, 2
and 4 of a batch of five, twice; a seeded batch of 40 RGB-D-like frames; one frame of 9 500 keypoints; 65 535 frames; the positions
against orbfe_unproject_stereo_device, the records against orbfe_refresh_map_points, depth_selected through
orbfe_track_queries_stereo_device, and the chain local map -> SearchLocalPoints -> PoseOptimization -> this call on one stream."""
import numpy as np
import pytest
import torch

from refactored_orb_slam2_amd import _lib, tracking
from tests import np_keyframe as M

pytestmark = pytest.mark.gpu
GUARD = 3   # canary rows on either side of an output array
CANARY = M.CANARY
CASES = M.directed_cases()
KEYS = ("headers", "new_points", "new_index", "n_new", "depth_selected", "assigned")


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is None:
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)).copy()).cuda()


def _stack(problem, frames, key):
    return np.stack([problem["frames"][f][key] for f in frames])


def _scalars(problem, frames, key, dtype):
    return np.asarray([problem["frames"][f][key] for f in frames], dtype)


class Tables:
    """the reference keyframes of a problem in device memory: every slot array behind one lead word, and the table with their device
    addresses (null and misaligned ones as the problem states them); the same on the host for the host form"""

    def __init__(self, problem):
        T = problem["tables"]
        arrays, n = T["slot_arrays"], [len(a) for a in T["slot_arrays"]]
        offs = np.cumsum([0] + n)
        self.slots = _dev(np.concatenate([np.zeros(1, np.int32)] + arrays).astype(np.int32))
        self.host_slots = [a.copy() for a in arrays]
        dev_table, host_table = np.zeros(len(n), _lib.COV_KEYFRAME_DTYPE), np.zeros(len(n), _lib.COV_KEYFRAME_DTYPE)
        for k in range(len(n)):
            for table, at in ((dev_table, self.slots.data_ptr() + 4 * (1 + int(offs[k]))), (host_table, self.host_slots[k].ctypes.data)):
                table[k]["n_keys"] = T["n_keys"][k]
                table[k]["slots"] = 0 if (T["slots_state"][k] == 1 or not n[k]) else at + 2 if T["slots_state"][k] == 2 else at
        self.table, self.host_table = _dev(dev_table), host_table
        self.point_bad, self.point_observations = _dev(T["point_bad"]), _dev(T["point_observations"])


def run_device(problem, tables, frames, flags, mode, new_cap, with_outlier=True, with_assigned=True, stream=None):
    """one device call over the listed frames: the output arrays with canaries and guards checked"""
    S, cap, p_cap = len(frames), problem["cap"], problem["p_cap"]
    shapes = {"headers": (S, 64), "new_points": (S * new_cap, 72), "new_index": (S * new_cap, 4), "n_new": (S, 4), "depth_selected": (S * cap, 4)}
    buf = {k: torch.full((n + 2 * GUARD, w), CANARY, dtype=torch.uint8).cuda() for k, (n, w) in shapes.items()}
    view = lambda k: buf[k][GUARD:]
    assigned = np.full((S + 2 * GUARD, cap), 0x5A5A5A5A, np.int32)
    assigned[GUARD:GUARD + S] = _stack(problem, frames, "assigned")
    d_assigned = _dev(assigned)
    T = problem["tables"]
    tracking.keyframe_insertion_device(
        problem["scales"], flags, mode, S=S, cap=cap, new_cap=new_cap, depth=_dev(_stack(problem, frames, "depth")),
        n=_dev(_scalars(problem, frames, "n", np.int32)), headers=view("headers"), keys_un=_dev(_stack(problem, frames, "keys_un")),
        desc=_dev(_stack(problem, frames, "desc")), cam=_dev(_stack(problem, frames, "cam")), assigned=d_assigned[GUARD:] if with_assigned else None,
        points=_dev(_stack(problem, frames, "points")), n_points=_dev(_scalars(problem, frames, "n_points", np.int32)), p_cap=p_cap,
        observed_offset=problem["observed_offset"], outlier=_dev(_stack(problem, frames, "outlier")) if with_outlier else None,
        decision=_dev(_stack(problem, frames, "decision")), ref_kf=_dev(_scalars(problem, frames, "ref_kf", np.int32)), keyframes=tables.table,
        n_kf=len(T["slot_arrays"]), point_bad=tables.point_bad, point_observations=tables.point_observations, n_map_points=len(T["point_bad"]),
        n_points_base=_dev(_scalars(problem, frames, "base", np.int32)), new_points=view("new_points"), new_index=view("new_index"),
        n_new=view("n_new"), depth_selected=view("depth_selected"), stream=stream)
    torch.cuda.synchronize()
    out = {}
    for k, (n, w) in shapes.items():
        a = buf[k].cpu().numpy()
        assert (a[:GUARD] == CANARY).all() and (a[GUARD + n:] == CANARY).all(), k + ": written outside the array"
        out[k] = a[GUARD:GUARD + n].copy()
    a = d_assigned.cpu().numpy()
    assert (a[:GUARD] == 0x5A5A5A5A).all() and (a[GUARD + S:] == 0x5A5A5A5A).all(), "assigned: written outside the array"
    if with_assigned:
        out["assigned"] = a[GUARD:GUARD + S].copy()
    return out


def run_host(problem, tables, frames, flags, mode, new_cap, with_outlier=True, with_assigned=True):
    S, cap = len(frames), problem["cap"]
    out = {"headers": M.canary((S,), _lib.KF_HEADER_DTYPE), "new_points": M.canary((S, new_cap), _lib.MAP_POINT_DTYPE),
           "new_index": M.canary((S, new_cap), np.int32), "n_new": M.canary((S,), np.int32), "depth_selected": M.canary((S, cap), np.float32)}
    T = problem["tables"]
    return tracking.keyframe_insertion(
        problem["scales"], flags, mode, depth=_stack(problem, frames, "depth"), n=_scalars(problem, frames, "n", np.int32),
        keys_un=_stack(problem, frames, "keys_un"), desc=_stack(problem, frames, "desc"), cam=_stack(problem, frames, "cam"),
        assigned=_stack(problem, frames, "assigned") if with_assigned else None, points=_stack(problem, frames, "points"),
        n_points=_scalars(problem, frames, "n_points", np.int32), outlier=_stack(problem, frames, "outlier") if with_outlier else None,
        decision=_stack(problem, frames, "decision"), ref_kf=_scalars(problem, frames, "ref_kf", np.int32), keyframes=tables.host_table,
        point_bad=T["point_bad"], point_observations=T["point_observations"], n_points_base=_scalars(problem, frames, "base", np.int32),
        new_cap=new_cap, observed_offset=problem["observed_offset"], depth_selected=True, out=out)


def _same(got, want, what):
    ok = True
    for k in KEYS:
        if k in want and k in got and bytes(got[k].tobytes()) != want[k].tobytes():
            g, w = np.frombuffer(got[k].tobytes(), np.uint8), np.frombuffer(want[k].tobytes(), np.uint8)
            at = int(np.flatnonzero(g != w)[0])
            print(what, k, "first differing byte", at, "of", len(g), "\n got ", got[k].reshape(-1)[:16], "\n want", want[k].reshape(-1)[:16])
            ok = False
    return ok


def _new_cap(problem, mode, flags, new_cap, opt):
    if new_cap == -1:   # one short of what the frame creates
        R = M.frame_reading(problem, problem["frames"][0], flags, mode, opt.get("with_outlier", True), opt.get("with_assigned", True))
        assert len(R["created"]) > 10
        return len(R["created"]) - 1
    return problem["cap"] if new_cap is None else new_cap


@pytest.mark.parametrize("name", sorted(CASES))
def test_directed_frame_alone_and_in_a_batch_both_forms(name):
    problem, mode, flags, new_cap, opt = CASES[name]
    new_cap = _new_cap(problem, mode, flags, new_cap, opt)
    tables = Tables(problem)
    ok = True
    for frames in ([0], [0, 1, 0, 1, 0]):
        want = M.reading(problem, frames, flags, mode, new_cap, **opt)
        if name.startswith("refused_"):
            assert want["headers"]["status"][0] == M.REFUSED and (want["headers"]["status"][1:2] != M.REFUSED).all()
        if name == "overflow_one_short":
            assert want["headers"]["status"][0] == M.OVERFLOW and want["n_new"][0] == new_cap == want["headers"]["n_created"][0] - 1
        for rep in range(2 if len(frames) > 1 else 1):
            ok = _same(run_device(problem, tables, frames, flags, mode, new_cap, **opt), want, f"{name} device {frames} run {rep}") and ok
        ok = _same(run_host(problem, tables, frames, flags, mode, new_cap, **opt), want, f"{name} host {frames}") and ok
    assert ok


def test_seeded_batch_of_40_rgbd_like_frames():
    problem = M.seeded_problem()
    tables = Tables(problem)
    frames = list(range(len(problem["frames"])))
    want = M.reading(problem, frames, M.ALL, M.KEYFRAME, 400)
    need = want["headers"]["need"]
    assert 5 < need.sum() < len(frames) - 5 and (want["headers"]["status"] == M.OVERFLOW).any() and (want["headers"]["status"] == M.OK).any()
    depth = np.stack([f["depth"] for f in problem["frames"]])
    assert len(np.unique(depth)) < depth.size / 4   # ties are the rule
    assert _same(run_device(problem, tables, frames, M.ALL, M.KEYFRAME, 400), want, "seeded keyframe")
    assert _same(run_host(problem, tables, frames[:6], M.ALL, M.KEYFRAME, 400), M.reading(problem, frames[:6], M.ALL, M.KEYFRAME, 400), "seeded host")
    want = M.reading(problem, frames, M.CREATE, M.LAST_FRAME, problem["cap"])
    assert (want["headers"]["n_created"] > 100).all()
    assert _same(run_device(problem, tables, frames, M.CREATE, M.LAST_FRAME, problem["cap"]), want, "seeded last frame")


def test_one_frame_of_9500_keypoints_all_with_depth():
    rng = np.random.default_rng(3)
    cap = _lib.KF_MAX_CAP
    depth = (np.round(rng.uniform(0.5, 80, cap) / 0.01) * 0.01).astype(np.float32)
    fr = M.make_frame(17, cap, cap, 4096, depth=depth, occupied=0.3, tracked_tail=0)
    assert (fr["depth"] > 0).all()
    problem = M.make_problem([fr], cap, 4096, th_depth=np.float32(3.5))
    tables = Tables(problem)
    want = M.reading(problem, [0], M.CREATE | M.STATISTICS, M.KEYFRAME, cap)
    assert want["headers"]["M"][0] == cap and 200 < want["headers"]["L"][0] < 1000
    assert _same(run_device(problem, tables, [0], M.CREATE | M.STATISTICS, M.KEYFRAME, cap), want, "9500")
    big = M.make_problem([fr], cap, 4096, th_depth=np.float32(100))   # every candidate is close: the whole sorted order is written
    want = M.reading(big, [0], M.CREATE, M.LAST_FRAME, cap)
    assert want["headers"]["L"][0] == cap and want["headers"]["n_created"][0] > 6000
    assert _same(run_device(big, tables, [0], M.CREATE, M.LAST_FRAME, cap), want, "9500 all close")


def test_grid_limit_65535_frames_of_four_keypoints():
    rng = np.random.default_rng(9)
    kinds = []
    for k in range(16):
        d = rng.choice([0.0, 3.0, 3.0, 7.5, 45.0, np.nan], 4).astype(np.float32)
        kinds.append(M.make_frame(100 + k, 4, 4, 4, depth=d, occupied=0.5, tracked_tail=0, n_points=4, base=k))
    problem = M.make_problem(kinds, 4, 4)
    tables = Tables(problem)
    S = _lib.KF_MAX_FRAMES
    frames = [f % 16 for f in range(S)]
    one = M.reading(problem, list(range(16)), M.ALL, M.KEYFRAME, 4)
    two = M.reading(problem, list(range(16)), M.CREATE, M.KEYFRAME, 4)
    assert two["headers"]["n_created"].sum() > 16
    tile = lambda a: np.concatenate([a] * (S // 16 + 1))[:S]
    assert _same(run_device(problem, tables, frames, M.ALL, M.KEYFRAME, 4), {k: tile(v) for k, v in one.items()}, "65535 all")
    assert _same(run_device(problem, tables, frames, M.CREATE, M.KEYFRAME, 4), {k: tile(v) for k, v in two.items()}, "65535 create")


def _healthy(n=700, cap=768, p_cap=512, seed=23):
    fr = M.make_frame(seed, n, cap, p_cap, occupied=0.4, tracked_tail=0)
    return M.make_problem([fr], cap, p_cap), fr


def test_created_positions_equal_unproject_stereo_device_rows():
    from refactored_orb_slam2_amd import matcher
    problem, fr = _healthy()
    cap = problem["cap"]
    got = run_device(problem, Tables(problem), [0], M.CREATE, M.KEYFRAME, cap)
    points = torch.zeros((1, cap, 60), dtype=torch.uint8).cuda()
    s = torch.cuda.Stream()
    matcher.unproject_stereo_batch(_dev(fr["keys_un"][None]), _dev(fr["desc"][None]), _dev(np.asarray([fr["n"]], np.int32)),
                                   _dev(fr["depth"][None]), _dev(np.array([fr["cam"]], _lib.UNPROJECT_CAM_DTYPE)), 1, points, s)
    s.synchronize()
    rows = points.cpu().numpy().reshape(-1).view(_lib.LAST_POINT_DTYPE)
    n_new = int(got["n_new"].view(np.int32).reshape(-1)[0])
    idx = got["new_index"].view(np.int32).reshape(-1)[:n_new]
    new = got["new_points"].reshape(-1).view(_lib.MAP_POINT_DTYPE)[:n_new]
    assert n_new > 100 and (rows["valid"][idx] == 1).all()
    assert new["pos"].tobytes() == rows["pos"][idx].tobytes() and new["desc"].tobytes() == rows["desc"][idx].tobytes()


def test_keyframe_records_equal_refresh_map_points_of_one_observation():
    from refactored_orb_slam2_amd import map_point
    problem, fr = _healthy(seed=29)
    cap = problem["cap"]
    got = run_device(problem, Tables(problem), [0], M.CREATE, M.KEYFRAME, cap)
    n_new = int(got["n_new"].view(np.int32).reshape(-1)[0])
    idx = got["new_index"].view(np.int32).reshape(-1)[:n_new]
    new = got["new_points"].reshape(-1).view(_lib.MAP_POINT_DTYPE)[:n_new]
    kfs = [{"desc": fr["desc"], "bad": 0, "Ow": fr["cam"]["Ow"]}]
    pts = [{"obs": [(0, int(i))], "pos": new["pos"][j], "ref": 0, "ref_octave": int(fr["keys_un"]["octave"][i])} for j, i in enumerate(idx)]
    up = map_point.refresh_map_points(kfs, pts, problem["scales"]["scale_factors"][0][:8])
    assert n_new > 100 and (up["status"] == _lib.MP_UPDATED).all()
    for k in ("normal", "min_distance", "max_distance", "desc"):
        assert up[k].tobytes() == new[k].tobytes(), k


def test_depth_selected_feeds_track_queries_like_the_masked_depth():
    from refactored_orb_slam2_amd import matcher
    problem = M.seeded_problem(seed=8, S=4, n=900, cap=1024, p_cap=512)
    frames, cap = [0, 1, 2, 3], 1024
    got = run_device(problem, Tables(problem), frames, M.CREATE, M.LAST_FRAME, cap)
    sel = got["depth_selected"].view(np.float32).reshape(4, cap)
    masked = np.full((4, cap), -1.0, np.float32)   # the mask, made on the host from the reading's selection
    for f in frames:
        fr = problem["frames"][f]
        visited = M.selection_literal(fr["depth"][:fr["n"]], M.TH_DEPTH)
        masked[f, visited] = fr["depth"][visited]
    assert sel.tobytes() == masked.tobytes() and (masked > 0).sum() > 400
    poses = np.zeros(4, _lib.TRACK_POSE_DTYPE)
    for f in frames:
        cam = problem["frames"][f]["cam"]
        Rwc = cam["Rwc"].reshape(3, 3)
        poses[f]["Rcw"], poses[f]["tcw"] = Rwc.T.reshape(9), -(Rwc.T @ cam["Ow"])
    poses["fx"] = poses["fy"] = 718.856; poses["cx"], poses["cy"], poses["mbf"] = 607.19, 185.22, 386.1448
    poses["max_x"], poses["max_y"], poses["th"], poses["forward"] = 1241, 376, 15, 0
    poses["scale_factors"][:, :8] = M.scale_factors()
    args = lambda d: (_dev(_stack(problem, frames, "keys_un")), _dev(_stack(problem, frames, "desc")), _dev(_scalars(problem, frames, "n", np.int32)),
                      d, _dev(_stack(problem, frames, "cam")), 0, _dev(poses), 0)
    out = []
    s = torch.cuda.Stream()
    for d in (torch.from_numpy(sel.copy()).cuda(), _dev(masked)):
        q, nq = torch.zeros((4, cap, 68), dtype=torch.uint8).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        matcher.track_queries_stereo_batch(*args(d), q, nq, s)
        s.synchronize()
        out.append((q.cpu().numpy(), nq.cpu().numpy()))
    assert out[0][0].tobytes() == out[1][0].tobytes() and np.array_equal(out[0][1], out[1][1])
    valid = out[0][0].reshape(-1).view(_lib.QUERY_DTYPE)["valid"].reshape(4, cap)
    assert valid.sum() > 100 and not valid[masked <= 0].any()


def test_the_chain_local_map_search_pose_keyframe_on_one_stream():
    """vote -> local map -> SearchLocalPoints -> PoseOptimization -> the keyframe call, enqueued on one stream with no host read in between
    (ref_kf is read where orbfe_local_map_batch_device left it, in its header array), against the same steps run one by one with
    a host read between them, and against the reading fed with what the one-by-one run left"""
    from refactored_orb_slam2_amd import local_map, optimizer, synth
    from refactored_orb_slam2_amd.matcher import Matcher, make_frustum
    from tests import np_localmap
    from tests.test_localmap_gpu import Resident
    from tests.test_matcher_gpu import _two_frames
    w, h, F = 640, 480, 8
    _, _, k1, d1, sf = _two_frames(w, h, 1000)
    scene, frames = np_localmap.make_local_map(21, n_kf=40, n_points=1500, n_keys=200, n_frames=F)
    conn_cap, kf_cap, p_cap = 64, 64, 1600
    R = Resident({"scene": scene, "frames": frames, "conn_cap": conn_cap, "kf_cap": kf_cap, "p_cap": p_cap, "tamper": None})
    frs, cams, Tcw = [], np.zeros(F, _lib.UNPROJECT_CAM_DTYPE), np.zeros((F, 12), np.float32)
    fx, cx, cy = 718.856, w / 2 + 3.2, h / 2 - 1.7
    for i in range(F):
        R_, t_ = synth.camera_pose(40 + i)
        R_, t_ = np.asarray(R_, np.float32).reshape(3, 3), np.asarray(t_, np.float32).reshape(3)
        frs.append(make_frustum(R_, t_, fx, fx, cx, cy, 386.1448, (0, w, 0, h), 1.2, 8))
        cams[i]["Rwc"], cams[i]["Ow"] = R_.T.reshape(9), -(R_.T @ t_)
        Tcw[i] = np.concatenate([R_, t_[:, None]], axis=1).reshape(12)
    cams["cx"], cams["cy"], cams["invfx"], cams["invfy"] = cx, cy, np.float32(1) / np.float32(fx), np.float32(1) / np.float32(fx)
    n_points = len(scene["points"])
    records = np.zeros(n_points, _lib.MAP_POINT_DTYPE)
    records[:] = np.resize(synth.local_map(k1, d1, frs[0], 41, n_points), n_points)
    rng = np.random.default_rng(77)
    records["observed"] = (rng.random(n_points) < 0.8).astype(np.int32)
    cap, n = len(k1) + 5, len(k1)
    kps = np.zeros((F, cap), _lib.KP_DTYPE); desc = np.zeros((F, cap, 32), np.uint8)
    kps[:, :n] = k1; desc[:, :n] = d1
    depth = np.zeros((F, cap), np.float32)
    depth[:, :n] = (np.round(rng.uniform(1, 90, (F, n)) / 0.05) * 0.05) * (rng.random((F, n)) < 0.7)
    pose_cam = np.zeros(1, _lib.POSE_CAMERA_DTYPE)
    pose_cam["fx"] = pose_cam["fy"] = fx; pose_cam["cx"], pose_cam["cy"], pose_cam["mbf"], pose_cam["n_levels"] = cx, cy, 386.1448, 8
    pose_cam["inv_level_sigma2"][0, :8] = 1.0 / (M.scale_factors() ** 2)
    decision = np.stack([M.default_decision(frame_id=100 + f, accept_keyframes=f % 2, keyframes_in_queue=f % 4, sensor=1 + f % 2) for f in range(F)])
    point_obs = rng.integers(0, 6, n_points).astype(np.int32)
    scales = M.make_scales(th_depth=np.float32(20))   # few enough close points are tracked for the frame that tracks at all to need a keyframe
    pk = R.pack
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a).cuda()
    tables = {"obs": _dev(pk["obs"]), "recs": _dev(pk["recs"]), "point_bad": R.point_bad, "kf_order": _dev(pk["kf_order"]), "kf_bad": R.kf_bad,
              "graph": R.graph, "children": R.children, "table": R.table, "records": _dev(records)}
    d_kps, d_desc, d_depth, d_cams, d_dec, d_obs = dev(kps), dev(desc), dev(depth), dev(cams), dev(decision), dev(point_obs)
    d_slots, d_sub, d_frames, d_seen = _dev(R.T["frame_slots"]), _dev(R.T["subjects"]), _dev(R.T["frames"]), _dev(R.T["seen"])
    d_frs, d_pcam, d_Tcw = dev(np.concatenate(frs)), dev(pose_cam), dev(Tcw)
    t_n = torch.full((F,), n, dtype=torch.int32, device="cuda")
    z = lambda *shape, dtype=torch.uint8, fill=CANARY: torch.full(shape, fill, dtype=dtype, device="cuda")
    m = Matcher()
    s = torch.cuda.Stream()

    def run(one_by_one):
        B = {"vote_h": z(F, 32), "vote_e": z(F * conn_cap, 8), "lm_h": z(F, 32), "local_kf": z(F, kf_cap, dtype=torch.int32),
             "local_points": z(F, p_cap, dtype=torch.int32), "n_pts": z(F, dtype=torch.int32), "map_points": z(F, p_cap, 72),
             "track": z(F, p_cap, 24, fill=0), "blocked": z(F, cap, fill=0), "assigned": z(F, cap, dtype=torch.int32, fill=-1),
             "ntm": z(F, dtype=torch.int32, fill=0), "nm": z(F, dtype=torch.int32, fill=0), "result": z(F, 68), "outlier": z(F, cap),
             "headers": z(F, 64), "new_points": z(F, cap, 72), "new_index": z(F, cap * 4).view(torch.int32), "n_new": z(F * 4).view(torch.int32),
             "depth_selected": z(F, cap * 4).view(torch.float32)}
        torch.cuda.synchronize()
        wait = s.synchronize if one_by_one else (lambda: None)
        with torch.cuda.stream(s):
            local_map.track_local_map_device(m, s, tables, d_slots, d_sub, d_frames, d_seen, conn_cap, kf_cap, B["vote_h"], B["vote_e"], B["lm_h"],
                                             B["local_kf"], B["local_points"], B["n_pts"], B["map_points"], d_kps, d_desc, t_n, None, (0, w, 0, h),
                                             d_frs, 1.0, 0.8, B["track"], B["blocked"], B["assigned"], B["ntm"], B["nm"])
            wait()
            optimizer.pose_optimization_batch(d_kps, None, t_n, B["assigned"], B["map_points"], B["n_pts"], d_pcam, d_Tcw, B["result"], B["outlier"],
                                              stream=s)
            wait()
            if one_by_one:   # the host reads the reference keyframes and hands them over as a plain array
                ref = torch.from_numpy(B["lm_h"].cpu().numpy().reshape(-1).view(_lib.LM_HEADER_DTYPE)["ref_kf"].copy()).cuda()
                ref_kf, stride = ref, 4
            else:
                ref_kf, stride = B["lm_h"].data_ptr() + _lib.LM_HEADER_DTYPE.fields["ref_kf"][1], 32
            B["before"] = B["assigned"].clone() if one_by_one else None
            tracking.keyframe_insertion_device(
                scales, M.ALL, M.KEYFRAME, S=F, cap=cap, new_cap=cap, depth=d_depth, n=t_n, headers=B["headers"], keys_un=d_kps, desc=d_desc,
                cam=d_cams, assigned=B["assigned"], points=B["map_points"], n_points=B["n_pts"], p_cap=p_cap, outlier=B["outlier"], decision=d_dec,
                ref_kf=ref_kf, ref_kf_stride=stride, keyframes=R.table, n_kf=int(R.table.shape[0]), point_bad=R.point_bad, point_observations=d_obs,
                n_map_points=n_points, new_points=B["new_points"], new_index=B["new_index"], n_new=B["n_new"], depth_selected=B["depth_selected"],
                stream=s)
        s.synchronize()
        return B

    chain, steps = run(False), run(True)
    for k in ("lm_h", "map_points", "result", "outlier", "assigned", "headers", "new_points", "new_index", "n_new", "depth_selected"):
        assert chain[k].cpu().numpy().tobytes() == steps[k].cpu().numpy().tobytes(), k
    # the reading, fed with what the steps left in front of the last call
    lm_h = steps["lm_h"].cpu().numpy().reshape(-1).view(_lib.LM_HEADER_DTYPE)
    before, outl = steps["before"].cpu().numpy(), steps["outlier"].cpu().numpy()
    mp = steps["map_points"].cpu().numpy().reshape(F, p_cap * 72).view(_lib.MAP_POINT_DTYPE).reshape(F, p_cap)
    npts = steps["n_pts"].cpu().numpy()
    fr = [{"n": n, "keys_un": kps[f], "desc": desc[f], "depth": depth[f], "cam": cams[f], "assigned": before[f], "points": mp[f],
           "n_points": int(npts[f]), "outlier": outl[f], "decision": decision[f], "ref_kf": int(lm_h["ref_kf"][f]), "base": 0} for f in range(F)]
    problem = {"frames": fr, "cap": cap, "p_cap": p_cap, "scales": scales, "observed_offset": 36,
               "tables": {"slot_arrays": R.T["kf_slots"], "slots_state": R.T["slots_state"], "n_keys": R.T["n_keys"],
                          "point_bad": R.T["point_bad"], "point_observations": point_obs}}
    want = M.reading(problem, list(range(F)), M.ALL, M.KEYFRAME, cap)
    got = {k: steps[k].cpu().numpy() for k in KEYS}
    H = want["headers"]
    print("inliers", H["n_matches_inliers"], "ref", H["n_ref_matches"], "close", H["n_tracked_close"], H["n_non_tracked_close"], "need", H["need"],
          "created", H["n_created"])
    assert _same(got, want, "chain")
    assert (H["status"] == M.OK).all() and (H["n_matches_inliers"] > 0).any() and (H["n_ref_matches"] > 0).any()
    assert 0 < H["need"].sum() < F and H["n_created"].sum() > 50 and (lm_h["ref_kf"] >= 0).all()
    m.close()


def test_driver_close_points(tmp_path):
    """examples/stereo_kitti.py --trajectory --close-points on a synthetic sequence in the KITTI layout: every tracked assignment of a
    frame names a keypoint of the frame before that the temporal-point rule selects (the closed form on the driver's own dump), and
    some keypoint with depth is left out by it"""
    import os
    import subprocess
    import sys
    from refactored_orb_slam2_amd import synth
    from tests.test_pose_gpu import ROOT, _write_png_gray
    seq = tmp_path / "00"
    (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir()
    W, H, N = 1241, 376, 3
    pairs = synth.sequence(W, H, N, seq=20, stereo=True)
    with open(seq / "times.txt", "w") as f:
        for i, (L, R) in enumerate(pairs):
            _write_png_gray(seq / "image_0" / f"{i:06d}.png", L)
            _write_png_gray(seq / "image_1" / f"{i:06d}.png", R)
            f.write(f"{i * 0.1:e}\n")
    traj, dump = str(tmp_path / "traj.txt"), str(tmp_path / "dump.npz")
    th = 6.0   # the synthetic scene is close: a ThDepth that cuts it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "stereo_kitti.py"), str(seq), "--trajectory", traj, "--dump", dump,
                        "--close-points", "--th-depth", str(th), "--batch", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "trajectory saved: 3 poses" in r.stdout
    g = np.load(dump)
    th_depth = np.float32(386.1448) * np.float32(th) / np.float32(718.856)
    left_out = tracked = 0
    for i in range(1, N):
        d = g[f"depth_{i - 1}"]
        order, Mc, c, Lp = M.selection_closed_form(d, th_depth)
        selected = set(order[:Lp].tolist())
        a = g[f"assigned_{i}"]
        assert set(a[a >= 0].tolist()) <= selected, i
        left_out += Mc - Lp
        tracked += int((a >= 0).sum())
    assert left_out > 50 and tracked > 50
