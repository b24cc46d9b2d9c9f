"""GPU: orbfe_pose_optimization / orbfe_pose_optimization_batch_device (Optimizer::PoseOptimization on the device) against the
numpy reading of tests/np_pose.py -- never against itself or against csrc/pose_internal.h compiled for the host.

Criterion (derived, not tuned): every rotation entry within 2^-23, every translation entry within 2^-23 * max(1, |t|_inf) -- one
unit in the last place of a float at the scale of the block, both sides computing in double and rounding once; outlier flags,
n_initial, n_bad, n_inliers and rounds EQUAL; iterations reported only.  Every figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from refactored_orb_slam2_amd._lib import KP_DTYPE, LAST_POINT_DTYPE, MAP_POINT_DTYPE, POSE_RESULT_DTYPE
from tests import np_pose as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _keys(s):
    k = np.zeros(len(s["keys_xy"]), KP_DTYPE)
    k["x"], k["y"], k["octave"] = s["keys_xy"][:, 0], s["keys_xy"][:, 1], s["octave"]
    k["size"], k["angle"], k["class_id"] = 31.0, 12.5, -1
    return k


def _camera(s):
    c = s["cam"]
    return optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["inv_level_sigma2"])


def _records(s, dtype):
    r = np.zeros(len(s["points"]), dtype)
    r["pos"] = s["points"]
    r["desc"] = 0xA5
    return r


def _compare(name, res, outlier, ref):
    """prints the figures, then asserts the criterion; returns the number of pose entries that are not bit-equal"""
    T, Tr = np.asarray(res["Tcw"], np.float32), ref["Tcw"]
    d = np.abs(T.astype(np.float64) - Tr.astype(np.float64))
    tol = P.pose_tolerance(Tr)
    not_equal = int((T.view(np.uint32) != Tr.view(np.uint32)).sum())
    flags_differ = int((np.asarray(outlier) != ref["outlier"]).sum())
    print(f"pose parity {name}: max diff / tolerance {float((d / tol).max()):.3f}, entries not bit-equal {not_equal}/12, flags that "
          f"differ {flags_differ}, n_initial {int(res['n_initial'])}/{ref['n_initial']}, n_bad {int(res['n_bad'])}/{ref['n_bad']}, "
          f"rounds {int(res['rounds'])}/{ref['rounds']}, iterations {int(res['iterations'])} (reading {ref['iterations']})")
    assert flags_differ == 0, name
    assert (int(res["n_initial"]), int(res["n_bad"]), int(res["n_inliers"]), int(res["rounds"])) == \
        (ref["n_initial"], ref["n_bad"], ref["n_inliers"], ref["rounds"]), name
    assert np.all(d <= tol), (name, d / tol)
    return not_equal


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a).cuda()


class Batch:
    """Scenes stacked into one batch: ragged counts, `cap` padding rows filled with garbage"""

    def __init__(self, scenes, dtype=LAST_POINT_DTYPE, frame_shift=0, with_u_right=True, pad=13):
        import torch
        self.scenes, F = scenes, len(scenes)
        self.cap = max(len(s["keys_xy"]) for s in scenes) + pad
        self.p_cap = max(len(s["points"]) for s in scenes) + 3
        rng = np.random.default_rng(7)
        kps = rng.integers(0, 256, (F, self.cap, KP_DTYPE.itemsize), dtype=np.uint8).view(KP_DTYPE).reshape(F, self.cap)
        ur = np.full((F, self.cap), np.nan, np.float32)
        asg = rng.integers(-3, 50, (F, self.cap)).astype(np.int32)
        pts = rng.integers(0, 256, (F, self.p_cap, dtype.itemsize), dtype=np.uint8).view(dtype).reshape(F, self.p_cap)
        n, npts, T = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros((F, 12), np.float32)
        for f, s in enumerate(scenes):
            m = len(s["keys_xy"])
            kps[f, :m], asg[f, :m], n[f], T[f] = _keys(s), s["assigned"], m, s["Tcw_in"]
            ur[f, :m] = -1.0 if s["u_right"] is None else s["u_right"]
            dst = (f - frame_shift) % F      # frame f reads the records of frame (f - frame_shift) mod F
            pts[dst, : len(s["points"])] = _records(s, dtype)
            npts[dst] = len(s["points"])
        self.h_assigned = asg
        self.kps, self.ur, self.asg, self.pts = _dev(kps), (_dev(ur) if with_u_right else None), _dev(asg), _dev(pts)
        self.n, self.npts, self.T = _dev(n), _dev(npts), _dev(T)
        self.cam = _dev(_camera(scenes[0]))
        self.res = torch.zeros((F, POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        self.out = torch.full((F, self.cap), 0xEE, dtype=torch.uint8, device="cuda")
        self.frame_shift = frame_shift

    def run(self, flags=0):
        import torch
        st = torch.cuda.Stream()
        optimizer.pose_optimization_batch(self.kps, self.ur, self.n, self.asg, self.pts, self.npts, self.cam, self.T, self.res, self.out,
                                          frame_shift=self.frame_shift, flags=flags, stream=st)
        st.synchronize()
        res = self.res.cpu().numpy().view(POSE_RESULT_DTYPE).reshape(-1)
        return res, self.out.cpu().numpy()


@pytest.fixture(scope="module")
def refs():
    return {name: (P.case_scene(name), P.run_case(P.case_scene(name))) for name in P.CASES}


@pytest.mark.parametrize("name", list(P.CASES))
def test_host_form_against_the_reading(refs, name):
    s, ref = refs[name]
    res, outlier = optimizer.pose_optimization(_keys(s), s["u_right"], s["assigned"], _records(s, LAST_POINT_DTYPE), _camera(s), s["Tcw_in"])
    _compare(name, res, outlier, ref)
    if name == "edges_2":   # returns 0, the pose is the input pose bit for bit
        assert int(res["n_inliers"]) == 0 and int(res["rounds"]) == 0
        assert np.array_equal(np.asarray(res["Tcw"]).view(np.uint32), s["Tcw_in"].view(np.uint32))


def test_batch_form_against_the_reading(refs):
    """every case of one camera stacked into one batch; the 12-level case, whose camera differs, with copies in a batch of its own;
    the all-monocular cases once more with d_u_right == NULL"""
    names8 = [n for n in P.CASES if n != "levels_12"]
    for names, kw in ((names8, {}), (["levels_12", "levels_12"], {}), (["all_mono", "u_right_null"], dict(with_u_right=False))):
        b = Batch([refs[n][0] for n in names], **kw)
        res, out = b.run()
        for f, name in enumerate(names):
            m = len(refs[name][0]["keys_xy"])
            _compare(f"batch:{name}", res[f], out[f, :m], refs[name][1])
            assert np.all(out[f, m:] == 0xEE), "rows behind d_n[f] must not be written"
        assert np.array_equal(b.asg.cpu().numpy(), b.h_assigned), "assigned is written only with ORBFE_POSE_DISCARD"


def test_deterministic_at_any_position_and_batch_size(refs):
    names = [n for n in P.CASES if n != "levels_12"]
    scenes = [refs[n][0] for n in names]
    r1, o1 = Batch(scenes).run()
    b = Batch(scenes)
    r2, o2 = b.run()
    r2b, o2b = b.run()      # the same buffers a second time
    assert r1.tobytes() == r2.tobytes() == r2b.tobytes() and o1.tobytes() == o2.tobytes() == o2b.tobytes()
    rr, orr = Batch(scenes[::-1]).run()
    assert rr[::-1].tobytes() == r1.tobytes() and np.array_equal(orr[::-1], o1)
    # one case alone against the same case in the middle of 256 copies of the others
    k = names.index("standard")
    many = [scenes[i % len(scenes)] for i in range(256)]
    many[128] = scenes[k]
    rm, om = Batch(many).run()
    ra, oa = Batch([scenes[k]]).run()
    assert rm[128].tobytes() == ra[0].tobytes() == r1[k].tobytes()
    m = len(scenes[k]["keys_xy"])
    assert np.array_equal(om[128, :m], oa[0, :m]) and np.array_equal(oa[0, :m], o1[k, :m])
    for i in range(256):
        assert rm[i].tobytes() == r1[i % len(scenes)].tobytes() or i == 128


def test_frame_shift_and_record_strides(refs):
    names = ["standard", "edges_40", "outliers_40", "behind"]
    scenes = [refs[n][0] for n in names]
    base, obase = Batch(scenes).run()
    for kw in (dict(frame_shift=1), dict(dtype=MAP_POINT_DTYPE), dict(dtype=MAP_POINT_DTYPE, frame_shift=1), dict(frame_shift=3),
               dict(frame_shift=5)):
        r, o = Batch(scenes, **kw).run()
        for f, name in enumerate(names):
            _compare(f"{kw}:{name}", r[f], o[f, : len(scenes[f]["keys_xy"])], refs[name][1])
        assert r.tobytes() == base.tobytes() and o.tobytes() == obase.tobytes()


def test_bare_positions_and_out_of_range_rows(refs):
    """stride 12 (bare positions); a row whose assigned value is >= n_points or whose octave is outside the levels is no edge"""
    s = dict(refs["standard"][0])
    s["assigned"] = s["assigned"].copy(); s["octave"] = s["octave"].copy()
    rows = np.flatnonzero(s["assigned"] >= 0)
    s["assigned"][rows[3]] = len(s["points"])            # first index outside
    s["assigned"][rows[4]] = 2 ** 30
    s["octave"][rows[5]] = s["n_levels"]                 # first level outside
    s["octave"][rows[6]] = -1
    ref = P.run_case(s)
    assert ref["n_initial"] == refs["standard"][1]["n_initial"] - 4
    res, outlier = optimizer.pose_optimization(_keys(s), s["u_right"], s["assigned"], s["points"], _camera(s), s["Tcw_in"])
    _compare("bare positions, four rows out of range", res, outlier, ref)
    assert not outlier[rows[3:7]].any()


def test_discard_flag(refs):
    names = ["standard", "edges_12", "outliers_40"]
    scenes = [refs[n][0] for n in names]
    b0 = Batch(scenes)
    r0, o0 = b0.run()
    b1 = Batch(scenes)
    r1, o1 = b1.run(flags=_lib.POSE_DISCARD)
    assert r0.tobytes() == r1.tobytes()                  # the counts are those before the discard
    a1 = b1.asg.cpu().numpy()
    for f, s in enumerate(scenes):
        m = len(s["keys_xy"])
        bad = o0[f, :m] != 0
        assert bad.sum() == r0[f]["n_bad"] > 0
        assert np.all(a1[f, :m][bad] == -1) and np.array_equal(a1[f, :m][~bad], s["assigned"][~bad])   # Tracking.cc:815-826
        assert not o1[f, :m].any()
        assert np.array_equal(a1[f, m:], b1.h_assigned[f, m:]) and np.all(o1[f, m:] == 0xEE)          # rows behind n untouched
    assert np.array_equal(b0.asg.cpu().numpy(), b0.h_assigned)


def test_validation_with_a_device():
    """the limits at their boundary where the accepted side needs a device (the refused side: tests/test_pose_cpu.py)"""
    s = P.make_scene(5, n_edges=20)
    b = Batch([s], pad=_lib.POSE_MAX_ROWS - len(s["keys_xy"]))
    assert b.cap == _lib.POSE_MAX_ROWS
    res, out = b.run()
    _compare("cap 9500", res[0], out[0, : len(s["keys_xy"])], P.run_case(s))
    for levels in (1, 16):
        s = P.make_scene(6, n_edges=50, n_levels=levels, scale_factor=1.05)
        res, outlier = optimizer.pose_optimization(_keys(s), s["u_right"], s["assigned"], s["points"], _camera(s), s["Tcw_in"])
        _compare(f"{levels} levels", res, outlier, P.run_case(s))
    # n = 0 and n_points = 0 are accepted
    s = P.make_scene(8, n_edges=0)
    res, outlier = optimizer.pose_optimization(_keys(s)[:0], None, s["assigned"][:0], s["points"][:0], _camera(s), s["Tcw_in"])
    assert int(res["n_initial"]) == 0 and int(res["rounds"]) == 0 and np.array_equal(np.asarray(res["Tcw"]), s["Tcw_in"])


# ---- the chain: extraction -> stereo matching -> UnprojectStereo -> track queries -> projection search -> pose optimisation ------
KITTI_CAM = dict(bf=386.1448, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)


def _track_records(W, H, sf):
    from refactored_orb_slam2_amd._lib import TRACK_POSE_DTYPE, UNPROJECT_CAM_DTYPE
    c = KITTI_CAM
    cam = np.zeros(1, UNPROJECT_CAM_DTYPE); pose = np.zeros(1, TRACK_POSE_DTYPE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    cam["Rwc"] = eye; cam["cx"] = c["cx"]; cam["cy"] = c["cy"]
    cam["invfx"] = np.float32(1) / np.float32(c["fx"]); cam["invfy"] = np.float32(1) / np.float32(c["fy"])
    pose["Rcw"] = eye; pose["fx"] = c["fx"]; pose["fy"] = c["fy"]; pose["cx"] = c["cx"]; pose["cy"] = c["cy"]; pose["mbf"] = c["bf"]
    pose["max_x"] = W; pose["max_y"] = H; pose["th"] = 7.0; pose["scale_factors"][0, :len(sf)] = sf
    return cam, pose


def _oracle_frames(pairs, NF, W, H):
    """what the oracle computes for the steps in front of the optimisation, frame by frame: (keypoints, mvuRight, depth, descriptors)"""
    from tests import oracle_lib as ol
    oL, oR = ol.OracleExtractor(NF), ol.OracleExtractor(NF)
    sf, isf = oL.scale_factors, oL.inv_scale_factors
    out = []
    for (L, R) in pairs:
        kL, dL = oL(L); kR, dR = oR(R)
        _, ur, depth = ol.compute_stereo_matches(kL, dL, kR, dR, [oL.level_pixels(l) for l in range(8)], [oR.level_pixels(l) for l in range(8)],
                                                 sf, isf, KITTI_CAM["bf"], KITTI_CAM["bf"] / KITTI_CAM["fx"])
        out.append((kL, ur, depth, dL))
    return out, sf, oL.inv_sigma2


def _reading_of_frame(kL, ur, assigned, points, inv_sigma2):
    cam = dict(fx=KITTI_CAM["fx"], fy=KITTI_CAM["fy"], cx=KITTI_CAM["cx"], cy=KITTI_CAM["cy"], mbf=KITTI_CAM["bf"], inv_level_sigma2=inv_sigma2)
    return P.optimize_pose(np.stack([kL["x"], kL["y"]], 1), kL["octave"], ur, assigned, points["pos"], cam,
                           np.eye(4, dtype=np.float32)[:3].reshape(12))


def test_chain_on_the_device_end_to_end():
    """orbfe_extract_batch_device x 2 -> orbfe_stereo_match_device -> orbfe_unproject_stereo_device -> orbfe_track_queries_device
    (frame_shift 1) -> orbfe_proj_match_batch_device -> orbfe_pose_optimization_batch_device on one stream with no host copy in
    between; the reading, fed what the oracle computes for the steps in front, must agree frame by frame.  The synthetic sequence is
    not a rigid motion, so there is no truth here -- only parity."""
    import torch
    from refactored_orb_slam2_amd import ORBextractor, synth
    from refactored_orb_slam2_amd.matcher import Matcher, track_queries_batch, unproject_stereo_batch
    from tests import oracle_lib as ol
    W, H, NF, F = 1241, 376, 2000, 4
    pairs = synth.sequence(W, H, F, seq=20, stereo=True)
    frames, sf, inv_sigma2 = _oracle_frames(pairs, NF, W, H)
    cam, pose = _track_records(W, H, sf)
    dev = torch.device("cuda", 0)
    exL, exR, mt = ORBextractor(NF, device=0), ORBextractor(NF, device=0), Matcher(0)
    np.testing.assert_array_equal(exL.GetInverseScaleSigmaSquares(), inv_sigma2)
    cap = exL.max_keypoints(W, H)
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)
    kl, dl, nl, kr, dr, nr = z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32), z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32)
    ur, depth, nst = z(F, cap, dt=torch.float32), z(F, cap, dt=torch.float32), z(F, dt=torch.int32)
    pts, q, nq = z(F, cap, 60), z(F, cap, 68), z(F, dt=torch.int32)
    blocked, assigned, ntr = z(F, cap), z(F, cap, dt=torch.int32), z(F, dt=torch.int32)
    t_cams = _dev(np.repeat(cam, F)); t_poses = _dev(np.repeat(pose, F))
    t_pcam = _dev(optimizer.pose_camera(KITTI_CAM["fx"], KITTI_CAM["fy"], KITTI_CAM["cx"], KITTI_CAM["cy"], KITTI_CAM["bf"], inv_sigma2))
    t_eye = _dev(np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (F, 1)))
    res, out = z(F, POSE_RESULT_DTYPE.itemsize), z(F, cap)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        dL = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev); dR = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
        exL.extract_batch_device(dL, kl, dl, nl, stream=st)
        exR.extract_batch_device(dR, kr, dr, nr, stream=st)
        mt.stereo_match(exL, exR, kl, dl, nl, kr, dr, nr, KITTI_CAM["bf"], KITTI_CAM["bf"] / KITTI_CAM["fx"], ur, depth, nst, stream=st)
        unproject_stereo_batch(kl, dl, nl, depth, t_cams, 1, pts, st)
        track_queries_batch(t_poses, pts, nl, 1, q, nq, st)
        assigned.fill_(-1)
        mt.proj_match_batch(kl, dl, nl, ur, (0.0, float(W), 0.0, float(H)), q, nq, 1, 0.9, True, blocked, assigned, ntr, stream=st)
        optimizer.pose_optimization_batch(kl, ur, nl, assigned, pts, nl, t_pcam, t_eye, res, out, frame_shift=1, stream=st)
    st.synchronize()
    r = res.cpu().numpy().view(POSE_RESULT_DTYPE).reshape(-1)
    o = out.cpu().numpy()
    for f in range(F):
        kL, urf, dep, dLf = frames[f]
        pk, _, pdep, pd = frames[(f - 1) % F]
        prev = ol.unproject_stereo(cam, pk, pd, pdep)
        nm, asg, _ = ol.OracleFrame(kL, dLf, sf, 0, W, 0, H, urf).search_by_projection_frame(ol.track_queries(pose, prev), True)
        ref = _reading_of_frame(kL, urf, asg, prev, inv_sigma2)
        assert ref["n_initial"] == nm and int(nl[f]) == len(kL)
        m = _margin(ref)
        print(f"chain frame {f}: {nm} matches, margin {m:.3g}")
        assert m >= 1e-4, "this frame is not a parity case: an edge sits on the chi2 bound"
        _compare(f"chain frame {f}", r[f], o[f, : len(kL)], ref)
        assert ref["n_initial"] > 300
    for h in (exL, exR, mt):
        h.close()


def _margin(r):
    return min((float(np.abs(t["chi2"].astype(np.float64) / t["bound"].astype(np.float64) - 1).min()) for t in r["trace"]), default=1.0)


def _write_png_gray(path, img):
    import struct, zlib
    h, w = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) +
                chunk(b"IEND", b""))


def test_driver_trajectory(tmp_path):
    """examples/stereo_kitti.py --trajectory on a synthetic sequence in the KITTI layout: one line of 12 finite numbers per frame,
    identical for batch sizes that cut the sequence at different chunk edges, and equal to composing the reading's relative poses --
    the reading fed the driver's own dump with the points unprojected by the oracle; the tolerance applies to each relative pose and
    the composition is repeated here in double.  --trajectory with --shard is refused."""
    from refactored_orb_slam2_amd import synth
    from tests import oracle_lib as ol
    seq = tmp_path / "00"
    (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir()
    W, H, N = 1241, 376, 5
    pairs = synth.sequence(W, H, N, seq=20, stereo=True)
    with open(seq / "times.txt", "w") as f:
        for i, (L, R) in enumerate(pairs):
            _write_png_gray(seq / "image_0" / f"{i:06d}.png", L)
            _write_png_gray(seq / "image_1" / f"{i:06d}.png", R)
            f.write(f"{i * 0.1:e}\n")
    drv = os.path.join(ROOT, "examples", "stereo_kitti.py")
    texts = []
    for extra in ([], ["--batch", "4"], ["--batch", "2"]):
        traj, dump = str(tmp_path / "traj.txt"), str(tmp_path / "dump.npz")
        r = subprocess.run([sys.executable, drv, str(seq), "--trajectory", traj, "--dump", dump] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "trajectory saved: 5 poses" in r.stdout
        texts.append(open(traj).read())
    assert texts[0] == texts[1] == texts[2]
    lines = texts[0].splitlines()
    got = np.array([[float(v) for v in l.split()] for l in lines])
    assert got.shape == (N, 12) and np.isfinite(got).all()
    assert np.array_equal(got[0], np.eye(4)[:3].reshape(12))
    # the reading on the driver's own dump
    g = np.load(dump)
    oL = ol.OracleExtractor(2000)
    sf, inv_sigma2 = oL.scale_factors, oL.inv_sigma2
    cam, _ = _track_records(W, H, sf)
    Twc = np.eye(4)
    for i in range(N):
        if i > 0:
            prev = ol.unproject_stereo(cam, g[f"kp_{i - 1}"], g[f"desc_{i - 1}"], g[f"depth_{i - 1}"])
            ref = _reading_of_frame(g[f"kp_{i}"], g[f"ur_{i}"], g[f"assigned_{i}"], prev, inv_sigma2)
            assert _margin(ref) >= 1e-4
            _compare(f"driver frame {i}", g[f"pose_{i}"], g[f"outlier_{i}"], ref)
            assert ref["n_inliers"] >= 10
            Tff = np.eye(4)
            Tff[:3] = np.asarray(g[f"pose_{i}"]["Tcw"], np.float64).reshape(3, 4)      # the driver's relative pose, within the tolerance
            inv = np.eye(4)
            inv[:3, :3] = Tff[:3, :3].T
            inv[:3, 3] = -Tff[:3, :3].T @ Tff[:3, 3]
            Twc = Twc @ inv
        want = [float(f"{v:.9f}") for v in Twc[:3].reshape(12)]
        assert np.array_equal(got[i], want), i
    r = subprocess.run([sys.executable, drv, str(seq), "--trajectory", str(tmp_path / "t.txt"), "--shard"], capture_output=True, text=True)
    assert r.returncode != 0 and "--trajectory" in r.stderr and not os.path.exists(tmp_path / "t.txt")


def test_frame_larger_than_the_lds_cache():
    """the kernel keeps the edges of the first 2 048 rows in LDS and re-reads the rows behind them from global memory: a frame of
    ~4 600 rows with 3 000 edges takes both paths"""
    s = P.make_scene(77, n_edges=3000)
    assert len(s["keys_xy"]) > 4096 and (s["assigned"][2048:] >= 0).sum() > 1000
    ref = P.run_case(s)
    assert _margin(ref) >= 1e-4
    res, outlier = optimizer.pose_optimization(_keys(s), s["u_right"], s["assigned"], _records(s, LAST_POINT_DTYPE), _camera(s), s["Tcw_in"])
    _compare("4 600 rows", res, outlier, ref)
    b = Batch([P.case_scene("edges_40"), s, P.case_scene("standard")])
    r, o = b.run()
    _compare("4 600 rows in a batch", r[1], o[1, : len(s["keys_xy"])], ref)
    assert r[1].tobytes() == np.asarray(res).tobytes()
