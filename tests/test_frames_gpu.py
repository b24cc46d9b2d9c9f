"""GPU: orbfe_undistort_frames_device (UndistortKeyPoints + ComputeStereoFromRGBD for a batch of frames) against the numpy second
reading byte for byte, its edge cases, and the whole RGB-D motion-model step with undistorted keypoints and bounds -- the batched
device API and examples/rgbd_tum.py -- against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from refactored_orb_slam2_amd import ORBextractor, camera, synth
from refactored_orb_slam2_amd._lib import KP_DTYPE
from tests import np_frames as nf
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

W, H = 640, 480
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _depth_raw(f, w=W, h=H, holes=True):
    """A smooth 16-bit depth map (TUM-like raw units: 0.6 .. 3.4 m at 5000 per metre) with zero-depth holes."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 2.0 + 0.8 * np.sin(xx / 83.0 + 0.4 * f) * np.cos(yy / 61.0) + 0.6 * xx / w
    raw = np.rint(z * 5000).astype(np.uint16)
    if holes:
        rng = np.random.default_rng(100 + f)
        for _ in range(12):
            cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(8, 40)
            raw[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = 0
        raw[:, :3] = 0
    return raw


@pytest.fixture(scope="module")
def frames():
    """8 extracted synthetic 640 x 480 frames with different counts, plus a ninth of hand-made rows"""
    ex = ORBextractor(1000)
    res = ex.extract_batch(synth.sequence(W, H, 8, seq=31))
    ex.close()
    out = [(k[: len(k) - 53 * i], d[: len(k) - 53 * i]) for i, (k, d) in enumerate(res)]
    hand = np.zeros(24, KP_DTYPE)
    hand["x"] = [0, 0.999, 5.999, 6.0, -0.5, -0.999, -1.0, W - 0.001, W, W + 3, 319.5, 100.25, 17.999, 600, 3.5, 638.9999,
                 0, W - 1, 320, 320, 1e9, -1e9, 2.999, 41.999]
    hand["y"] = [0, 0.999, 7.999, 8.0, 10, 10, 10, 20, 20, 20, 240, -0.3, 479.999, H, H - 0.0001, 479.5, H - 1, 0, -1.0, -0.9999,
                 5, 5, 2.999, 41.999]
    hand["size"] = 31.0
    hand["angle"] = np.linspace(0, 359, 24); hand["response"] = np.arange(24) * 1.5
    hand["octave"] = np.arange(24) % 8; hand["class_id"] = -1
    out.append((hand, np.zeros((24, 32), np.uint8)))
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a)).cuda()


def _pack(frames, cap=None):
    cap = cap or max(len(k) for k, _ in frames) + 5
    kps = np.zeros((len(frames), cap), KP_DTYPE)
    n = np.zeros(len(frames), np.int32)
    for i, (k, _) in enumerate(frames):
        kps[i, : len(k)] = k; n[i] = len(k)
    return kps, n, cap


def _run(kps, n, cal, fmt, maps=None, width=None, in_place=False, n_frames=None):
    """one call; outputs (kps_un, u_right, depth, n_depth) as numpy, rows behind n pre-filled with sentinels"""
    import torch
    F, cap = kps.shape
    t_k = _dev(kps); t_n = _dev(n)
    t_ku = t_k if in_place else torch.full((F, cap, 28), 0x5A, dtype=torch.uint8, device="cuda")
    t_ur = torch.full((F, cap), 77.25, dtype=torch.float32, device="cuda")
    t_dp = torch.full((F, cap), -33.5, dtype=torch.float32, device="cuda")
    t_nd = torch.full((F,), -9, dtype=torch.int32, device="cuda")
    t_map = None if maps is None else (maps if isinstance(maps, torch.Tensor) else _dev(maps))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        if n_frames is None:
            camera.undistort_frames_batch(t_k, t_n, cal, fmt, t_map, t_ku, t_ur, t_dp, t_nd, s, width=width)
        else:   # the C ABI itself: an empty torch slice has no data pointer
            from refactored_orb_slam2_amd import _lib
            es = t_map.element_size()
            _lib.check(_lib.lib().orbfe_undistort_frames_device(n_frames, _lib.ptr(t_k), _lib.ptr(t_n), cap, C.byref(cal), fmt, _lib.ptr(t_map),
                                                                t_map.shape[2], t_map.shape[1], t_map.stride(1) * es, t_map.stride(0) * es,
                                                                _lib.ptr(t_ku), _lib.ptr(t_ur), _lib.ptr(t_dp), _lib.ptr(t_nd),
                                                                _lib.stream_handle(s)), "orbfe_undistort_frames_device")
    s.synchronize()
    return (t_ku.cpu().numpy().reshape(F, cap * 28).view(KP_DTYPE), t_ur.cpu().numpy(), t_dp.cpu().numpy(), t_nd.cpu().numpy())


def _expect(kps, n, cal, maps_f32):
    """restatement per frame: (kps_un, u_right, depth, n_depth) over the valid rows"""
    out = []
    for f in range(len(n)):
        k = kps[f, : n[f]]
        ku = nf.keys_un(cal, k)
        if maps_f32 is None:
            out.append((ku, np.full(len(k), -1, np.float32), np.full(len(k), -1, np.float32), 0))
        else:
            ur, dp, cnt = nf.rgbd_stereo(cal, k, ku, maps_f32[f])
            out.append((ku, ur, dp, cnt))
    return out


def _check(got, exp, n, cap):
    ku, ur, dp, nd = got
    for f, (eku, eur, edp, ecnt) in enumerate(exp):
        m = n[f]
        assert ku[f, :m].tobytes() == eku.tobytes(), f"keypoints of frame {f}"
        assert ur[f, :m].tobytes() == eur.tobytes(), f"u_right of frame {f}"
        assert dp[f, :m].tobytes() == edp.tobytes(), f"depth of frame {f}"
        assert int(nd[f]) == ecnt, f
        # u_right / depth rows at and behind n[f] keep their sentinels (the keypoint rows: checked by the callers)
        assert (ur[f, m:] == np.float32(77.25)).all() and (dp[f, m:] == np.float32(-33.5)).all()


@pytest.mark.parametrize("name", sorted(nf.CAMERAS))
def test_device_equals_the_restatement(frames, name):
    cal, _ = nf.camera(name)
    kps, n, cap = _pack(frames)
    raw = np.stack([_depth_raw(f) for f in range(len(n))])
    got = _run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16))
    exp = _expect(kps, n, cal, np.stack([nf.depth_map(cal, r) for r in raw]))
    _check(got, exp, n, cap)
    for f in range(len(n)):   # rows behind the count keep their sentinel bytes
        assert (got[0][f, n[f]:].view(np.uint8) == 0x5A).all()
    assert sum(e[3] for e in exp) > 3000   # most keypoints have depth; the holes and the hand-made rows do not
    # the monocular form: keys_un only, u_right / depth -1, count 0
    got = _run(kps, n, cal, camera.DEPTH_NONE)
    _check(got, _expect(kps, n, cal, None), n, cap)
    if name != "strong":
        assert not np.array_equal(got[0][0, :n[0]]["x"], kps[0, :n[0]]["x"])


def test_depth_edge_cases(frames):
    import torch
    kps, n, cap = _pack(frames)
    F = len(n)
    raw = np.stack([_depth_raw(f) for f in range(F)])
    # 16-bit input with the two TUM factors
    for dmf in (5000.0, 5208.0):
        cal = camera.calibration(517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0, dmf)
        _check(_run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16)), _expect(kps, n, cal, np.stack([nf.depth_map(cal, r) for r in raw])), n, cap)
    # a factor inside (1 - 1e-5, 1 + 1e-5): the float map is NOT scaled, the 16-bit one is; outside it both are
    fmap = (raw.astype(np.float32) * np.float32(0.000201)).astype(np.float32)
    for dmf in (1.0 / (1 + 4e-6), 1.0 / (1 - 9e-6), 1.0 / (1 + 3e-5), 1.0):
        cal = camera.calibration(500, 500, 320, 240, 0.1, -0.2, 0, 0, 0, 40.0, dmf)
        fac = np.float32(cal.depth_factor)
        assert (abs(float(fac - np.float32(1))) > 1e-5) == (dmf == 1.0 / (1 + 3e-5))
        got = _run(kps, n, cal, camera.DEPTH_F32, fmap)
        _check(got, _expect(kps, n, cal, np.stack([nf.depth_map(cal, m) for m in fmap])), n, cap)
        if fac != 1 and abs(float(fac - np.float32(1))) <= 1e-5:   # not scaled: mvDepth is the float map's own sample
            k0 = kps[0, :n[0]]
            assert got[2][0, :n[0]].tobytes() == nf.rgbd_stereo(cal, k0, nf.keys_un(cal, k0), fmap[0])[1].tobytes()
        _check(_run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16)), _expect(kps, n, cal, np.stack([nf.depth_map(cal, r) for r in raw])), n, cap)
    # truncation at x = k + 0.999, octaves >= 1, keypoints outside the map: a map whose every sample is distinct
    cal, _ = nf.camera("tum1_rgbd")
    ramp = (np.arange(H * W, dtype=np.int64).reshape(H, W) % 60000 + 1).astype(np.uint16)
    ramps = np.stack([ramp] * F)
    got = _run(kps, n, cal, camera.DEPTH_U16, ramps.view(np.int16))
    _check(got, _expect(kps, n, cal, np.stack([nf.depth_map(cal, r) for r in ramps])), n, cap)
    hand = kps[F - 1, : n[F - 1]]
    dep = got[2][F - 1, : n[F - 1]]
    inside = (hand["x"] > -1) & (hand["x"] < W) & (hand["y"] > -1) & (hand["y"] < H)
    assert (dep[~inside] == -1).all() and (dep[inside] > 0).all() and (~inside).sum() >= 6
    i = int(np.nonzero(hand["x"] == np.float32(5.999))[0][0])   # (5.999, 7.999) reads sample (7, 5)
    assert dep[i] == np.float32(ramp[7, 5]) * np.float32(cal.depth_factor)
    assert (hand["octave"][inside] >= 1).any()
    # pitched maps: extra columns and extra rows per image, filled with garbage that must not be read
    big = np.full((F, H + 5, W + 37), 0x7777, np.uint16)
    big[:, :H, :W] = raw
    t_big = _dev(big.view(np.int16))[:, :H, :]
    exp = _expect(kps, n, cal, np.stack([nf.depth_map(cal, r) for r in raw]))
    _check(_run(kps, n, cal, camera.DEPTH_U16, t_big, width=W), exp, n, cap)
    bigf = np.full((F, H + 2, W + 9), 123.0, np.float32)
    bigf[:, :H, :W] = fmap
    calf = camera.calibration(cal.fx, cal.fy, cal.cx, cal.cy, cal.k1, cal.k2, cal.p1, cal.p2, cal.k3, cal.mbf, 1000.0)
    _check(_run(kps, n, calf, camera.DEPTH_F32, _dev(bigf)[:, :H, :], width=W), _expect(kps, n, calf, np.stack([nf.depth_map(calf, m) for m in fmap])), n, cap)
    # in place: d_kps_un == d_kps
    ku, ur, dp, nd = _run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16), in_place=True)
    for f, (eku, eur, edp, ecnt) in enumerate(exp):
        assert ku[f, : n[f]].tobytes() == eku.tobytes() and ur[f, : n[f]].tobytes() == eur.tobytes() and int(nd[f]) == ecnt
        assert ku[f, n[f]:].tobytes() == kps[f, n[f]:].tobytes()
    # n_frames = 0: nothing is written
    ku, ur, dp, nd = _run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16), n_frames=0)
    assert (ku.view(np.uint8) == 0x5A).all() and (ur == np.float32(77.25)).all() and (nd == -9).all()
    # k1 = 0 (the TUM3 camera): mvKeysUn = mvKeys
    cal3, _ = nf.camera("tum3")
    ku, ur, dp, nd = _run(kps, n, cal3, camera.DEPTH_U16, raw.view(np.int16))
    for f in range(F):
        assert ku[f, : n[f]].tobytes() == kps[f, : n[f]].tobytes()
    _check((ku, ur, dp, nd), _expect(kps, n, cal3, np.stack([nf.depth_map(cal3, r) for r in raw])), n, cap)
    # the largest map accepted: 4095 x 4095 (one frame)
    m1 = np.zeros((1, 4095, 4095), np.uint16); m1[0, 4094, 4094] = 4321; m1[0, 0, 0] = 7
    k1 = np.zeros((1, 4), KP_DTYPE); k1[0]["x"] = [4094.5, 0.2, 4095.0, 2000]; k1[0]["y"] = [4094.9, 0.7, 10, 4095.5]
    ku, ur, dp, nd = _run(k1, np.array([4], np.int32), cal3, camera.DEPTH_U16, m1.view(np.int16))
    assert dp[0].tolist() == [np.float32(4321) * np.float32(cal3.depth_factor), np.float32(7) * np.float32(cal3.depth_factor), -1, -1]
    assert int(nd[0]) == 2


def test_batch_equals_frame_by_frame_and_repeats(frames):
    kps, n, cap = _pack(frames)
    raw = np.stack([_depth_raw(f) for f in range(len(n))])
    cal, _ = nf.camera("tum2_rgbd")
    a = _run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16))
    b = _run(kps, n, cal, camera.DEPTH_U16, raw.view(np.int16))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for f in range(len(n)):
        one = _run(kps[f:f + 1], n[f:f + 1], cal, camera.DEPTH_U16, raw[f:f + 1].view(np.int16))
        for x, y in zip(a, one):
            assert x[f:f + 1].tobytes() == y.tobytes(), f


# ------------------------------------------------------------------------------------------------ the RGB-D motion-model step
def _oracle_sequence(images, raws, cal, nfeat=1000):
    """oracle extraction -> restatement -> ol.unproject_stereo -> ol.track_queries -> OracleFrame(keys_un, ..., bounds, u_right)
    .search_by_projection_frame, frame by frame (frame 0 has no predecessor)"""
    from refactored_orb_slam2_amd._lib import TRACK_POSE_DTYPE, UNPROJECT_CAM_DTYPE
    oe = ol.OracleExtractor(nfeat)
    sf = oe.scale_factors
    h, w = images[0].shape
    bounds = nf.image_bounds(cal, w, h)
    cam = np.zeros(1, UNPROJECT_CAM_DTYPE); pose = np.zeros(1, TRACK_POSE_DTYPE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    cam["Rwc"] = eye; cam["cx"] = cal.cx; cam["cy"] = cal.cy
    cam["invfx"] = np.float32(1) / np.float32(cal.fx); cam["invfy"] = np.float32(1) / np.float32(cal.fy)
    pose["Rcw"] = eye; pose["fx"] = cal.fx; pose["fy"] = cal.fy; pose["cx"] = cal.cx; pose["cy"] = cal.cy; pose["mbf"] = cal.mbf
    pose["min_x"], pose["max_x"], pose["min_y"], pose["max_y"] = bounds
    pose["th"] = 15.0; pose["scale_factors"][0, :len(sf)] = sf
    exp, prev = [], None
    for img, raw in zip(images, raws):
        k, d = oe(img)
        ku = nf.keys_un(cal, k)
        ur, dep, _ = nf.rgbd_stereo(cal, k, ku, nf.depth_map(cal, raw))
        nm, assigned = 0, np.full(len(k), -1, np.int32)
        if prev is not None:
            nm, assigned, _ = ol.OracleFrame(ku, d, sf, *bounds, ur).search_by_projection_frame(ol.track_queries(pose, prev), True)
        exp.append(dict(kp=k, kpu=ku, desc=d, ur=ur, depth=dep, assigned=assigned, ntrack=nm))
        prev = ol.unproject_stereo(cam, ku, d, dep)
    return exp, bounds, cam, pose, sf


N_SEQ = 6
# floor of tracked matches per frame: half of the smallest count of frames 1-5 in the first run (TUM1: 642 .. 724, steep: 400 .. 477)
TRACK_FLOOR = {"tum1_rgbd": 320, "steep": 200}


@pytest.mark.parametrize("name", ["tum1_rgbd", "steep"])
def test_rgbd_motion_model_step_equals_the_oracle(name):
    import torch
    from refactored_orb_slam2_amd.matcher import Matcher, track_queries_stereo_batch
    images = synth.sequence(W, H, N_SEQ, seq=41)
    raws = [_depth_raw(f) for f in range(N_SEQ)]
    cal, _ = nf.camera(name)
    exp, bounds, cam, pose, sf = _oracle_sequence(images, raws, cal)
    # GPU: extract -> undistort / depth -> queries from the previous frame -> SearchByProjection(cur, last), one batch
    ex = ORBextractor(1000); mt = Matcher()
    cap = ex.max_keypoints(W, H)
    F = N_SEQ
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device="cuda")
    kps, desc, n = z(F, cap, 28), z(F, cap, 32), z(F, dt=torch.int32)
    kpu, ur, dep, nd = z(F, cap, 28), z(F, cap, dt=torch.float32), z(F, cap, dt=torch.float32), z(F, dt=torch.int32)
    q, nq = z(F, cap, 68), z(F, dt=torch.int32)
    blocked, assigned, ntr = z(F, cap), torch.full((F, cap), -1, dtype=torch.int32, device="cuda"), z(F, dt=torch.int32)
    cams = _dev(np.repeat(cam, F)); poses = _dev(np.repeat(pose, F))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_img = torch.from_numpy(np.stack(images)).cuda()
        d_map = torch.from_numpy(np.stack(raws).view(np.int16)).cuda()
        ex.extract_batch_device(d_img, kps, desc, n, stream=s)
        camera.undistort_frames_batch(kps, n, cal, camera.DEPTH_U16, d_map, kpu, ur, dep, nd, s)
        track_queries_stereo_batch(kpu, desc, n, dep, cams, 1, poses, 1, q, nq, s)
        mt.proj_match_batch(kpu, desc, n, ur, bounds, q, nq, 1, 0.9, True, blocked, assigned, ntr, stream=s)
    s.synchronize()
    outside = 0
    for f, e in enumerate(exp):
        m = int(n[f])
        assert m == len(e["kp"])
        assert kps[f, :m].cpu().numpy().reshape(-1).view(KP_DTYPE).tobytes() == e["kp"].tobytes()
        assert desc[f, :m].cpu().numpy().tobytes() == e["desc"].tobytes()
        g_ku = kpu[f, :m].cpu().numpy().reshape(-1).view(KP_DTYPE)
        assert g_ku.tobytes() == e["kpu"].tobytes()
        assert ur[f, :m].cpu().numpy().tobytes() == e["ur"].tobytes() and dep[f, :m].cpu().numpy().tobytes() == e["depth"].tobytes()
        assert int(nd[f]) == int((e["depth"] > 0).sum())
        outside += int(((g_ku["x"] < bounds[0]) | (g_ku["x"] >= bounds[1]) | (g_ku["y"] < bounds[2]) | (g_ku["y"] >= bounds[3])).sum())
        if f == 0:
            continue   # frame 0 was searched with the batch's tail (index mod F); the oracle frame 0 has no predecessor
        assert int(ntr[f]) == e["ntrack"], f
        np.testing.assert_array_equal(assigned[f, :m].cpu().numpy(), e["assigned"])
        assert e["ntrack"] >= TRACK_FLOOR[name], (f, e["ntrack"])
    assert bounds != (0, W, 0, H) and not np.array_equal(exp[1]["kpu"]["x"], exp[1]["kp"]["x"])
    if name == "steep":   # undistorted keypoints outside the bounds (TUM1's never are: see tests/np_frames.py), hundreds per frame
        assert outside >= N_SEQ * 100, outside
    ex.close(); mt.close()


def test_monocular_search_for_initialization_on_undistorted_frames():
    """SearchForInitialization between two undistorted frames (DEPTH_NONE) with the undistorted bounds == the oracle"""
    import torch
    from refactored_orb_slam2_amd.matcher import FrameView, ORBmatcher
    cal, _ = nf.camera("tum1_mono")
    ex = ORBextractor(2000)
    (k0, d0), (k1, d1) = ex.extract_batch(synth.sequence(W, H, 2, seq=15))
    sf = ex.GetScaleFactors()
    ex.close()
    kps, n, cap = _pack([(k0, d0), (k1, d1)])
    ku = _run(kps, n, cal, camera.DEPTH_NONE)[0]
    u0, u1 = ku[0, : n[0]].copy(), ku[1, : n[1]].copy()
    assert u0.tobytes() == nf.keys_un(cal, k0).tobytes() and u1.tobytes() == nf.keys_un(cal, k1).tobytes()
    b = camera.image_bounds(cal, W, H)
    prev = np.stack([u0["x"], u0["y"]], axis=1).astype(np.float32)
    nm, m12, p2 = ORBmatcher(0.9, True).SearchForInitialization(FrameView(u0, d0, *b), FrameView(u1, d1, *b), prev, 100)
    onm, om12, op2 = ol.search_for_initialization(u0, d0, ol.OracleFrame(u1, d1, sf, *b), prev, 100, np.float32(0.9), True)
    assert nm == onm and nm > 100
    np.testing.assert_array_equal(m12, om12)
    np.testing.assert_array_equal(p2, op2)


# ------------------------------------------------------------------------------------------------ examples/rgbd_tum.py
def _settings(path, vals):
    fx, fy, cx, cy, k1, k2, p1, p2, k3, bf, dmf = vals
    path.write_text(f"%YAML:1.0\n\nCamera.fx: {fx}\nCamera.fy: {fy}\nCamera.cx: {cx}\nCamera.cy: {cy}\n\nCamera.k1: {k1}\nCamera.k2: {k2}\n"
                    f"Camera.p1: {p1}\nCamera.p2: {p2}\n" + (f"Camera.k3: {k3}\n" if k3 else "") +
                    f"\nCamera.width: {W}\nCamera.height: {H}\nCamera.fps: 30.0\nCamera.bf: {bf}\nCamera.RGB: 1\nThDepth: 40.0\n"
                    f"DepthMapFactor: {dmf}\n\nORBextractor.nFeatures: 1000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\n"
                    "ORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n")


def test_rgbd_tum_driver_on_a_synthetic_tum_layout(tmp_path):
    """examples/rgbd_tum.py on a TUM RGB-D layout written here: RGB colour PNGs (Camera.RGB: 1), 16-bit depth PNGs, an association
    file and a settings file with the TUM1 values; per-frame mode and batches of 4 and 2 (the carry crosses chunk edges over 5
    frames): every frame's dump == the oracle.  Then a TUM3-style file (k1 = 0): mvKeysUn = mvKeys, bounds = the image."""
    from PIL import Image
    N = 5
    seq = tmp_path / "seq"
    (seq / "rgb").mkdir(parents=True); (seq / "depth").mkdir()
    greys = synth.sequence(W, H, N, seq=43)
    rng = np.random.default_rng(5)
    images, raws = [], []
    with open(tmp_path / "assoc.txt", "w") as fa:
        for i, g in enumerate(greys):
            rgb = np.stack([np.clip(g.astype(np.int16) + rng.integers(-6, 7, g.shape), 0, 255).astype(np.uint8), g,
                            np.clip(g.astype(np.int16) + rng.integers(-6, 7, g.shape), 0, 255).astype(np.uint8)], axis=-1)
            Image.fromarray(rgb).save(seq / "rgb" / f"{i}.png")
            raw = _depth_raw(i)
            Image.fromarray(raw).save(seq / "depth" / f"{i}.png")
            t = 1305031102.175304 + i / 30
            fa.write(f"{t:.6f} rgb/{i}.png {t + 0.002:.6f} depth/{i}.png\n")
            # Camera.RGB 1: RGB2GRAY on imread's BGR data -- the 0.299 weight meets the file's blue channel
            images.append(((rgb[..., 2].astype(np.int64) * 4899 + rgb[..., 1].astype(np.int64) * 9617 + rgb[..., 0].astype(np.int64) * 1868
                            + 8192) >> 14).astype(np.uint8))
            raws.append(raw)
    drv = os.path.join(ROOT, "examples", "rgbd_tum.py")
    for name, vals in (("TUM1.yaml", nf.CAMERAS["tum1_rgbd"][0]), ("TUM3.yaml", nf.TUM3[0])):
        _settings(tmp_path / name, vals)
        cal = camera.read_settings(str(tmp_path / name))["calibration"]
        exp, bounds, *_ = _oracle_sequence(images, raws, cal)
        for extra in ([], ["--batch", "4"], ["--batch", "2"]) if name == "TUM1.yaml" else (["--batch", "4"],):
            dump = str(tmp_path / "dump.npz")
            r = subprocess.run([sys.executable, drv, str(tmp_path / name), str(seq), str(tmp_path / "assoc.txt"), "--dump", dump] + extra,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "median tracking time" in r.stdout and "Images in the sequence: 5" in r.stdout and "depth points/frame" in r.stdout
            g = np.load(dump)
            assert g["bounds"].tobytes() == np.array(bounds, np.float32).tobytes()
            for i, e in enumerate(exp):
                for key in ("kp", "kpu", "desc", "ur", "depth", "assigned"):
                    assert g[f"{key}_{i}"].tobytes() == e[key].tobytes(), (name, extra, i, key)
                assert int(g[f"ntrack_{i}"]) == e["ntrack"], (name, extra, i)
            assert min(e["ntrack"] for e in exp[1:]) > 100
        if name == "TUM3.yaml":
            assert tuple(float(b) for b in g["bounds"]) == (0.0, float(W), 0.0, float(H))
            for i in range(N):
                assert g[f"kpu_{i}"].tobytes() == g[f"kp_{i}"].tobytes()
        else:
            assert any(not np.array_equal(g[f"kpu_{i}"], g[f"kp_{i}"]) for i in range(N))
