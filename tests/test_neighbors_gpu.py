"""The resident fuse batch on the device: rows of one batched search against K single orbfe_kf_search calls (byte for byte) and against
the numpy reading, the partial search, the device forms, mapping.search_in_neighbors on the census scenes, refused inputs."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, mapping
from refactored_orb_slam2_amd.matcher import FrameView, FuseBatch, ORBmatcher
from tests import np_neighbors as N
from tests import np_restatement as nr

pytestmark = pytest.mark.gpu

W, H = 640, 480
K_ALL, N_ALL = 33, 257
KS, NS = (1, 2, 5, 33), (0, 1, 63, 64, 65, 257)
MODES = {"fuse": (_lib.KF_FUSE, 3.0), "fuse_sim3": (_lib.KF_FUSE_SIM3, 4.0)}
SKIPPED = np.array([(-1, 256, -1, 0, 0, 0)], _lib.KF_RESULT_DTYPE)[0]


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)


def _camera(k, th):
    R = _rot_y(0.015 * ((k % 7) - 3)).astype(np.float32)
    t = np.array([0.05 * ((k % 5) - 2), 0.03 * ((k % 3) - 1), 0.02 * (k % 4)], np.float32)
    cam = np.zeros(1, _lib.KF_CAMERA_DTYPE)
    cam["R"][0], cam["t"][0] = R.reshape(9), t
    cam["Ow"][0] = -(R.T.astype(np.float64) @ t.astype(np.float64))
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"] = 517.3, 516.5, 318.6, 255.3, 40.0
    cam["min_x"], cam["max_x"], cam["min_y"], cam["max_y"] = 0, W, 0, H
    cam["log_scale_factor"] = np.float32(np.log(1.2))
    cam["n_levels"] = N.N_LEVELS
    cam["th"] = th
    cam["scale_factors"][0, :N.N_LEVELS] = N.SCALE_FACTORS
    return cam


def _flip(rng, desc, n):
    d = desc.copy()
    for b in rng.choice(256, n, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


@pytest.fixture(scope="module")
def world():
    """257 candidate points (a few skipped, behind the cameras or outside the images) and 33 targets with a pose, a 1 / sigma2 table and
    keypoints of their own: 0 keypoints (target 1), 1 (target 2), about 300 otherwise -- noisy projections of the points, with
    descriptors 0 .. 60 bits away, and keypoints of no point.  Odd targets are stereo (a part of their keypoints has a right
    coordinate).  Target 4 is target 3 with a four times tighter 1 / sigma2 table."""
    rng = np.random.default_rng(2024)
    pts = np.zeros(N_ALL, _lib.KF_POINT_DTYPE)
    pos = np.stack([rng.uniform(-3.5, 3.5, N_ALL), rng.uniform(-2.5, 2.5, N_ALL), rng.uniform(4, 10, N_ALL)], 1).astype(np.float32)
    pos[5, 2] = -3.0; pos[77, 0] = 40.0
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1))
    pts["pos"] = pos
    pts["normal"] = (pos / dist[:, None]).astype(np.float32)
    pts["normal"][9] = -pts["normal"][9]                                  # fails the viewing-angle gate
    pts["max_distance"] = (dist * rng.uniform(1.0, 1.9, N_ALL)).astype(np.float32)
    pts["min_distance"] = (dist * rng.uniform(0.3, 0.9, N_ALL)).astype(np.float32)
    pts["min_distance"][11] = np.float32(dist[11] * 2)                    # fails the distance range
    pts["desc"] = rng.integers(0, 256, (N_ALL, 32), dtype=np.uint8)
    pts["skip"][[3, 64, 200]] = 1
    targets = []
    for k in range(K_ALL):
        cam = _camera(k, 3.0)
        R = cam["R"][0].reshape(3, 3).astype(np.float64); t = cam["t"][0].astype(np.float64)
        pc = pos.astype(np.float64) @ R.T + t
        u = 517.3 * pc[:, 0] / pc[:, 2] + 318.6; v = 516.5 * pc[:, 1] / pc[:, 2] + 255.3
        keys, desc, ur = [], [], []
        stereo = k % 2 == 1
        want = 0 if k == 1 else (1 if k == 2 else 300)
        for i in rng.permutation(N_ALL):
            if len(keys) >= want or pc[i, 2] <= 0:
                continue
            d3 = np.sqrt(((pos[i] - cam["Ow"][0]).astype(np.float64) ** 2).sum())
            lvl = int(np.clip(np.ceil(np.log(pts["max_distance"][i] / d3) / np.log(1.2)), 0, N.N_LEVELS - 1))
            x, y = u[i] + rng.normal(0, 1.1), v[i] + rng.normal(0, 1.1)
            if not (2 < x < W - 2 and 2 < y < H - 2):
                continue
            for _ in range(int(rng.integers(1, 3))):                       # one or two keypoints near a projection
                keys.append((x + rng.normal(0, 0.6), y + rng.normal(0, 0.6), 31.0, 0.0, 20.0, max(0, lvl - int(rng.integers(0, 3))), -1))
                desc.append(_flip(rng, pts["desc"][i], int(rng.integers(0, 61))))
                ur.append(np.float32(keys[-1][0] - 40.0 / pc[i, 2] + rng.normal(0, 0.8)) if stereo and rng.random() < 0.6 else np.float32(-1))
        while len(keys) < want:
            keys.append((rng.uniform(5, W - 5), rng.uniform(5, H - 5), 31.0, 0.0, 20.0, int(rng.integers(0, 4)), -1))
            desc.append(rng.integers(0, 256, 32, dtype=np.uint8)); ur.append(np.float32(-1))
        keys, desc, ur = keys[:want], desc[:want], ur[:want]
        inv = (N.INV_LEVEL_SIGMA2 * np.float32(1.0 + 0.1 * (k % 3))).astype(np.float32)
        targets.append(dict(keys=np.array(keys, _lib.KP_DTYPE) if keys else np.zeros(0, _lib.KP_DTYPE),
                            desc=np.array(desc, np.uint8).reshape(-1, 32), u_right=np.array(ur, np.float32) if stereo else None, inv=inv, k_cam=k))
    targets[4] = dict(targets[3], inv=(targets[3]["inv"] * np.float32(4)).astype(np.float32))
    return dict(points=pts, targets=targets)


def _views(world, K):
    return [FrameView(t["keys"], t["desc"], 0, W, 0, H, t["u_right"]) for t in world["targets"][:K]]


def _cams(world, K, th):
    return np.concatenate([_camera(t["k_cam"], th) for t in world["targets"][:K]])


def _batch(world, K, mode):
    m, th = MODES[mode]
    return FuseBatch(_views(world, K), _cams(world, K, th), [t["inv"] for t in world["targets"][:K]] if m == _lib.KF_FUSE else None, m)


@pytest.fixture(scope="module")
def single_rows(world):
    """K single orbfe_kf_search calls, as the drop-in makes them: the rows every batched form must equal byte for byte"""
    out = {}
    matcher = ORBmatcher(0.8, True)
    for mode, (m, th) in MODES.items():
        rows = np.zeros((K_ALL, N_ALL), _lib.KF_RESULT_DTYPE)
        for k, v in enumerate(_views(world, K_ALL)):
            t = world["targets"][k]
            _, rows[k], _ = matcher.KeyFrameSearch(v, _camera(t["k_cam"], th), world["points"], m, inv_level_sigma2=t["inv"] if m == _lib.KF_FUSE else None)
        out[mode] = rows
    return out


@pytest.fixture(scope="module")
def numpy_rows(world):
    out = {}
    P = list(world["points"])
    for mode, (m, th) in MODES.items():
        rows = []
        for k, t in enumerate(world["targets"]):
            F = nr.RefFrame(t["keys"], t["desc"], 0, W, 0, H, t["u_right"])
            cam = N._cam_dict(_camera(t["k_cam"], th))
            rows.append(nr.ref_fuse(F, t["inv"], cam, P) if m == _lib.KF_FUSE else nr.ref_fuse_sim3(F, cam, P))
        out[mode] = np.array(rows, np.int64)          # (K, N, 2): best_idx, best_dist
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K", KS)
def test_batch_rows_equal_single_calls_and_the_numpy_reading(world, single_rows, numpy_rows, mode, K):
    b = _batch(world, K, mode)
    try:
        for n in NS:
            rows = b.search(world["points"][:n])
            assert rows.shape == (K, n)
            assert rows.tobytes() == np.ascontiguousarray(single_rows[mode][:K, :n]).tobytes(), (K, n)
            np.testing.assert_array_equal(rows["best_idx"], numpy_rows[mode][:K, :n, 0])
            np.testing.assert_array_equal(rows["best_dist"], numpy_rows[mode][:K, :n, 1])
    finally:
        b.close()
    if K == K_ALL:
        r = single_rows[mode]
        print(f"{mode}: {(r['best_idx'] >= 0).sum()} of {r.size} rows with a candidate, {(r['level'] >= 0).sum()} pass the prologue")
        assert (r["best_idx"] >= 0).sum() > 2000 and (r["best_dist"][r["best_idx"] >= 0] <= 50).sum() > 1000
        assert (r[1]["best_idx"] == -1).all() and (r[1]["level"] >= 0).sum() > 100     # the empty target: prologue only
        stereo_hit = [k for k in range(1, K_ALL, 2) if (r[k]["best_idx"] >= 0).any()]
        assert len(stereo_hit) >= 10
        if mode == "fuse":   # targets 3 and 4 differ in the 1 / sigma2 table alone, and it decides rows
            differ = (r[3]["best_idx"] != r[4]["best_idx"]).sum()
            print(f"rows decided by the target's own 1 / sigma2 table: {differ}")
            assert differ >= 1 and (r[3]["level"] == r[4]["level"]).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_targets_with_image_bounds_of_their_own(world, mode):
    """every target carries its own bounds (several cameras): a row still is the single call's, bounds and grid geometry of target k"""
    m, th = MODES[mode]
    bounds = [(0, W, 0, H), (-8, W + 12, -5, H + 10), (0, W, 0, H), (-31, W + 3, -17, H + 29), (4, W - 4, 6, H - 2)]
    T = world["targets"][:5]
    views, cams = [], []
    for t, bd in zip(T, bounds):
        views.append(FrameView(t["keys"], t["desc"], *bd, u_right=t["u_right"]))
        c = _camera(t["k_cam"], th)
        c["min_x"], c["max_x"], c["min_y"], c["max_y"] = bd
        cams.append(c)
    invs = [t["inv"] for t in T]
    b = FuseBatch(views, np.concatenate(cams), invs if m == _lib.KF_FUSE else None, m)
    try:
        rows = b.search(world["points"])
    finally:
        b.close()
    matcher = ORBmatcher(0.8, True)
    differ = 0
    for k in range(5):
        _, single, _ = matcher.KeyFrameSearch(views[k], cams[k], world["points"], m, inv_level_sigma2=invs[k] if m == _lib.KF_FUSE else None)
        assert rows[k].tobytes() == single.tobytes(), k
        _, same_bounds, _ = matcher.KeyFrameSearch(_views(world, 5)[k], _camera(T[k]["k_cam"], th), world["points"], m,
                                                   inv_level_sigma2=invs[k] if m == _lib.KF_FUSE else None)
        differ += int(single.tobytes() != same_bounds.tobytes())
    assert (rows["best_idx"] >= 0).sum() > 400
    print(f"{mode}: targets whose rows depend on their own bounds: {differ}")


def _window_scene(counts=(0, 1, 16, 17, 64, 65)):
    """one target whose windows hold exactly `counts` octave-eligible keypoints (and keypoints of another octave behind them): the
    chunk edges of the enumeration.  Two keypoints tie at the minimum distance -- the last two in enumeration order, on either side of
    the chunk edge where the count is odd -- and the first must win."""
    b = N.Builder(5, K=1, stereo_target=-1)
    expect = []
    for n in counts:
        s = b.site()
        p = b.point(s, N.D()); b.keypoint(b.current, s, N.D(), p)
        first = None
        for j in range(n):
            tie = n >= 2 and j >= n - 2
            idx = b.keypoint(0, s, N.D(range(5)) if tie else N.D(range(20 + j % 7)), dx=0.25 * (j % 3), dy=0.25 * (j % 2))
            if tie and first is None:
                first = idx
        for j in range(n // 5):
            b.keypoint(0, s, N.D(), octave=5)              # nearer, but not of the predicted level: behind the eligible ones in the cell
        if n == 1:
            first = idx
        expect.append((-1, 256) if n == 0 else (first, 5 if n >= 2 else 20))
    return b.m, expect


@pytest.mark.parametrize("mode", list(MODES))
def test_hand_placed_windows(mode):
    m, expect = _window_scene()
    mo, th = MODES[mode]
    t = m.target(0, th)
    view = FrameView(t["keys"], t["desc"], 0, W, 0, H, t["u_right"])
    ids = m.point_matches(1)
    rec = np.zeros(len(ids), _lib.KF_POINT_DTYPE)
    for j, p in enumerate(ids):
        m.fill_point(p, rec[j])
    b = FuseBatch([view], t["camera"], [t["inv_level_sigma2"]] if mo == _lib.KF_FUSE else None, mo)
    try:
        rows = b.search(rec)[0]
    finally:
        b.close()
    _, single, _ = ORBmatcher(0.8, True).KeyFrameSearch(view, t["camera"], rec, mo, inv_level_sigma2=t["inv_level_sigma2"] if mo == _lib.KF_FUSE else None)
    assert rows.tobytes() == single.tobytes()
    assert [(int(r["best_idx"]), int(r["best_dist"])) for r in rows] == expect
    cam = N._cam_dict(t["camera"])
    want = nr.ref_fuse(m.kfs[0].frame(), t["inv_level_sigma2"], cam, list(rec)) if mo == _lib.KF_FUSE else nr.ref_fuse_sim3(m.kfs[0].frame(), cam, list(rec))
    assert [tuple(int(x) for x in w) for w in want] == expect


def _changed(world, idx, seed=3):
    rng = np.random.default_rng(seed)
    pts = world["points"][:65].copy()
    for i in idx:
        pts["desc"][i] = _flip(rng, pts["desc"][i], 12)
        pts["skip"][i] = 0
    return pts


@pytest.mark.parametrize("first_target", [0, 4, 5])
def test_partial_search(world, first_target):
    """the rows of the index list equal a full search after the same record change; every other byte of `results` keeps the sentinel"""
    K, n = 5, 65
    idx = np.array([0, 3, 17, 64], np.int32)
    pts = _changed(world, idx)
    b, full = _batch(world, K, "fuse"), _batch(world, K, "fuse")
    try:
        want = full.search(pts)
        b.search(world["points"][:n])
        got = np.frombuffer(bytes([0xAB]) * (K * n * 24), _lib.KF_RESULT_DTYPE).reshape(K, n).copy()
        b.search(pts[idx], idx, first_target, results=got)
        sel = np.zeros((K, n), bool); sel[first_target:, idx] = True
        assert got[sel].tobytes() == want[sel].tobytes()
        assert (got[~sel].view(np.uint8) == 0xAB).all()
        assert sel.sum() == (K - first_target) * len(idx)
        # the table is updated whatever first_target is: a full-width partial search over every target now equals the full search
        allp = np.arange(n, dtype=np.int32)
        again = b.search(pts, allp, 0)
        assert again.tobytes() == want.tobytes()
        # an empty index list writes nothing
        got2 = got.copy()
        b.search(pts[:0], np.zeros(0, np.int32), 0, results=got2)
        assert got2.tobytes() == got.tobytes()
        # the mask: a masked row is a skipped point's row, the others are untouched by it
        mask = np.zeros((K, n), np.uint8); mask[0, :] = 1; mask[3, 10:20] = 1; mask[:, 40] = 1
        masked = b.search(pts, skip=mask)
        assert masked[mask != 0].tobytes() == SKIPPED.tobytes() * int((mask != 0).sum())
        assert masked[mask == 0].tobytes() == want[mask == 0].tobytes()
        assert (want[mask != 0]["best_idx"] >= 0).sum() > 10     # the mask did hide candidates
    finally:
        b.close(); full.close()


def test_device_forms_equal_the_host_form(world):
    """orbfe_fuse_batch_create_device on borrowed arrays strided by a capacity and orbfe_fuse_batch_search_device, full and partial"""
    torch = pytest.importorskip("torch")
    K, n, cap = 5, 65, 320
    dev = torch.device("cuda")
    T = world["targets"][:K]
    kps = np.zeros((K, cap), _lib.KP_DTYPE); desc = np.zeros((K, cap, 32), np.uint8); ur = np.full((K, cap), -1, np.float32)
    cnt = np.zeros(K, np.int32)
    for k, t in enumerate(T):
        c = len(t["keys"]); cnt[k] = c
        kps[k, :c], desc[k, :c] = t["keys"], t["desc"]
        if t["u_right"] is not None:
            ur[k, :c] = t["u_right"]
    inv = np.zeros((K, 16), np.float32)
    for k, t in enumerate(T):
        inv[k, :N.N_LEVELS] = t["inv"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    stream = torch.cuda.Stream()
    held = [up(kps), up(desc), up(ur), up(cnt), up(_cams(world, K, 3.0)), up(inv)]
    b = FuseBatch.from_device(held[0].view(K, cap, 28), held[1].view(K, cap, 32), held[2], held[3], (0, W, 0, H), held[4], held[5],
                              _lib.KF_FUSE, stream)
    host = _batch(world, K, "fuse")
    try:
        want = host.search(world["points"][:n])
        d_pts = up(world["points"][:n]); d_res = torch.full((K * n * 24,), 0xAB, dtype=torch.uint8, device=dev)
        b.search_device(d_pts, n, None, 0, None, d_res, stream)
        stream.synchronize()
        assert d_res.cpu().numpy().tobytes() == want.tobytes()
        hits = (want["level"][2:] >= 0).sum(0)                 # three points that pass the prologue of the targets searched again
        idx = np.sort(np.argsort(-hits, kind="stable")[:3]).astype(np.int32)
        pts = _changed(world, idx)
        want2 = host.search(pts[idx], idx, 2, results=want.copy())
        k_m = 2 + int(np.argmax(want["level"][2:, idx[1]] >= 0))
        assert want2[k_m, idx[1]]["level"] >= 0
        mask = np.zeros((K, n), np.uint8); mask[k_m, idx[1]] = 1
        want3 = host.search(pts[idx], idx, 2, skip=mask, results=want.copy())
        d_idx, d_rec = up(idx), up(pts[idx])
        b.search_device(d_rec, n, d_idx.view(torch.int32), 2, None, d_res, stream)
        stream.synchronize()
        assert d_res.cpu().numpy().tobytes() == want2.tobytes()
        b.search_device(d_rec, n, d_idx.view(torch.int32), 2, up(mask), d_res, stream)
        stream.synchronize()
        assert d_res.cpu().numpy().tobytes() == want3.tobytes() and want3.tobytes() != want2.tobytes()
    finally:
        b.close(); host.close()


@pytest.mark.parametrize("i", range(len(N.SCENE_SEEDS)))
def test_search_in_neighbors_on_the_device(i):
    """the protocol on the device == the sequential yardstick on the census scenes: log, final state, and the numbers of full and
    repair searches the numpy backend makes"""
    s = N.scenes()[i]
    c = N.clone(s)
    want_log, want_fused, notes = N.sequential(c["map"], c["current"], c["targets"])
    assert N.census(notes) == set(N.TAGS)
    n = N.clone(s)
    ref = mapping.search_in_neighbors(n["map"], n["current"], n["targets"], search=lambda m, t, th: N.NumpySearch(m, t, th))
    d = N.clone(s)
    got = mapping.search_in_neighbors(d["map"], d["current"], d["targets"])
    assert got["log"] == want_log and got["n_fused"] == want_fused
    assert d["map"].state() == c["map"].state()
    assert (got["n_full"], got["n_repair"]) == (ref["n_full"], ref["n_repair"]) == (2, 3)


def test_a_refused_input_leaves_the_handle_usable(world):
    """each limit of the search at its last accepted and first refused value, between good calls.  K x n_points within int32 is refused
    before anything is read or allocated (a run of its last accepted value would be two thousand million rows: the stand-alone program
    of tests/cpp_neighbors checks that function at both values)."""
    K, n = 5, 65
    b = _batch(world, K, "fuse")
    L = _lib.lib()
    try:
        pts = world["points"][:n]
        want = b.search(pts)
        res = want.copy()

        def call(points=pts, n_points=n, idx=None, first_target=0, results=res):
            return L.orbfe_fuse_batch_search(b._h, _lib.ptr(points), n_points, _lib.ptr(idx), 0 if idx is None else len(idx), first_target,
                                             None, _lib.ptr(results))
        i32 = lambda *v: np.array(v, np.int32)   # noqa: E731
        for kw in (dict(first_target=-1), dict(first_target=K + 1), dict(n_points=-1), dict(idx=i32(n)), dict(idx=i32(-1)), dict(idx=i32(4, 4)),
                   dict(idx=i32(5, 4)), dict(idx=i32(1), n_points=n - 1), dict(n_points=(2 ** 31 - 1) // K + 1), dict(points=None),
                   dict(results=None)):
            assert call(**kw) == _lib.ERR_INVALID, kw
            assert b"fuse search" in L.orbfe_last_error(), kw
            assert res.tobytes() == want.tobytes()
        assert call(idx=i32(n - 1), points=pts[n - 1:]) == _lib.OK and call(idx=i32(0), points=pts[:1], first_target=K) == _lib.OK
        assert call(idx=i32(3, 4), points=pts[3:5], first_target=K - 1) == _lib.OK
        assert res.tobytes() == want.tobytes()
        assert b.search(pts).tobytes() == want.tobytes()
        assert b.search(pts[:0]).shape == (K, 0)          # an empty table launches nothing
        assert b.search(pts).tobytes() == want.tobytes()
    finally:
        b.close()
