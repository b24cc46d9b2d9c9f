"""GPU tests at the hard limits of include/orbfe.h: every limit at its largest accepted value (whole path byte-equal to the oracle,
the extreme value asserted to occur in the data) and at its first refused value (ORBFE_ERR_INVALID with a message, refused on the
host before any kernel runs, and the handle still works on the next valid call).

The kernels lean on these limits through packed fields: 12-bit keypoint coordinates, 16-bit keypoint indices next to distances, the
octave in 4 bits, 2 x 8192 + 1 stereo row-bucket ints and 9 bytes per keypoint of the ordered resolver in LDS."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import ORBextractor, _lib, synth
from refactored_orb_slam2_amd.matcher import FrameView, Matcher, ORBmatcher, make_frustum, make_queries
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

TALL_H = 4095
STEREO_LEVELS = 16
CAND_CAP = 1 << 22      # debug_candidates buffer: a 4095 x 4095 noise image has ~1.7 M level-0 candidates


def _refused(fn, *args, match):
    """fn(*args) raises ORBFE_ERR_INVALID whose message names the limit"""
    with pytest.raises(_lib.OrbfeError, match=match) as ei:
        fn(*args)
    assert ei.value.code == _lib.ERR_INVALID


def _extract_raw(ex, img, cap=64):
    """orbfe_extract on its own (ORBextractor.__call__ asks orbfe_extractor_max_keypoints first): a small output buffer, so a
    call that were not refused would end in a capacity error, never out of bounds"""
    h, w = img.shape
    kps = np.zeros(cap, _lib.KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int(0)
    _lib.check(_lib.lib().orbfe_extract(ex._h, _lib.ptr(img), w, h, img.strides[0], _lib.ptr(kps), _lib.ptr(desc), cap, C.byref(n)),
               "orbfe_extract")


def _compare_stages(ex, orc, kps, desc, okps, odesc, nlevels):
    """every stage view of the last extraction of `ex` / `orc`: pyramid, blur, FAST candidates, octree keypoints, then the keypoints
    and descriptors"""
    for l in range(nlevels):
        assert ex.level_size(l) == orc.level_size(l)
        np.testing.assert_array_equal(ex.debug_pyramid(0, l), orc.level_pixels(l), err_msg=f"pyramid level {l}")
        ob = orc.level_blurred(l)
        if ob is not None:
            np.testing.assert_array_equal(ex.debug_blurred(0, l), ob, err_msg=f"blur level {l}")
        x, y, s = ex.debug_candidates(0, l, CAND_CAP)
        ox, oy, os_ = orc.level_candidates(l)
        assert len(ox) < CAND_CAP
        np.testing.assert_array_equal(np.stack([x, y, s]), np.stack([ox, oy, os_]), err_msg=f"candidates level {l}")
        kx, ky, ks = ex.debug_level_keypoints(0, l, 1 << 15)
        ok = orc.level_keypoints(l)
        np.testing.assert_array_equal(np.stack([kx, ky, ks]), np.stack([ok["x"], ok["y"], ok["response"]]).astype(np.int32),
                                      err_msg=f"octree keypoints level {l}")
    np.testing.assert_array_equal(kps, okps)
    np.testing.assert_array_equal(desc, odesc)


def _n_ini(level_sizes):
    """nIni of every level with FAST cells (extractor.cpp: roundf(width / height) on the border-trimmed level, float arithmetic)"""
    out = []
    for lw, lh in level_sizes:
        width, height = np.float32(lw - 32), np.float32(lh - 32)
        if int(width / np.float32(30)) < 1 or int(height / np.float32(30)) < 1:
            continue
        q = float(width / height)
        out.append(int(q) + (1 if q - int(q) >= 0.5 else 0))
    return out


def _node_table(nf, sf=1.2, nlevels=8, n_ini=1):
    """max_nodes of the octree node table (extractor.cpp): round-64 of the largest max(N + 3, 4 nIni) + 1 over the levels"""
    m = max(max(n + 3, 4 * n_ini) + 1 for n in ol.OracleExtractor(nf, sf, nlevels).features_per_level)
    return (m + 63) & ~63


def _octree_lds(M):
    """LDS bytes of octree_select_kernel for a node table of M nodes (extractor.cpp / orbfe_octree_lds_bytes): 56 bytes per node,
    keys in what is left of a 40 KiB budget (at least 512), fixed tables"""
    fixed = 56 * M + 64 * 4 + 256 * 8 + 256
    keys = (40 * 1024 - fixed) // 8 if fixed + 8 * 512 <= 40 * 1024 else 512
    return fixed + 8 * keys


# the node table's real bound: the octree kernel's LDS (160 KiB per workgroup), far below the 8 192 entries it is declared for
NODE_MAX = max(M for M in range(64, 8193, 64) if _octree_lds(M) <= 160 * 1024)


def _largest_nf_of_full_node_table():
    nf = 9000
    while _node_table(nf) <= NODE_MAX:
        nf += 64
    while _node_table(nf) > NODE_MAX:
        nf -= 1
    return nf


def _stereo_scale_factor(nlevels=STEREO_LEVELS):
    """the largest float32 scale factor whose float32 scale[nlevels - 1] (float * double products, ORBextractor.cc:417) passes the
    row-bucket check 2 scale + 2 <= 28 of orbfe_stereo_match*, and the next float32 up"""
    def top(sf):
        s = np.float32(1)
        for _ in range(nlevels - 1):
            s = np.float32(np.float64(s) * np.float64(sf))
        return s
    sf = np.float32(13.0 ** (1.0 / (nlevels - 1)))
    while top(sf) > np.float32(13):
        sf = np.nextafter(sf, np.float32(0))
    while top(np.nextafter(sf, np.float32(2))) <= np.float32(13):
        sf = np.nextafter(sf, np.float32(2))
    return sf, np.nextafter(sf, np.float32(2))


# ------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def big():
    """one 4095 x 4095 image (noise over a synthetic frame) with nFeatures at the largest value whose octree node table fits in LDS:
    max_nodes == NODE_MAX"""
    nf = _largest_nf_of_full_node_table()
    rng = np.random.default_rng(12)
    img = np.tile(synth.frame(1365, 1365, seq=9, f=0), (3, 3))[:4095, :4095].copy()
    img[:, 1500:] = rng.integers(0, 256, (4095, 2595), dtype=np.uint8)
    ex, orc = ORBextractor(nf), ol.OracleExtractor(nf)
    k, d = ex(img)
    ok, od = orc(img)
    yield dict(nf=nf, img=img, ex=ex, orc=orc, k=k, d=d, ok=ok, od=od)
    ex.close()


@pytest.fixture(scope="module")
def tall():
    """a stereo pair of 4095 rows (512 row buckets) at 16 levels with the largest scale factor the stereo search takes (n_keys =
    8192), at the narrowest width every level accepts (nIni >= 1): the smallest accepted aspect ratio of a 4095-row image"""
    sf, sf_next = _stereo_scale_factor()
    exL, exR = ORBextractor(3000, float(sf), STEREO_LEVELS), ORBextractor(3000, float(sf), STEREO_LEVELS)
    ok = lambda w: min(_n_ini([exL.level_size(l, w, TALL_H) for l in range(STEREO_LEVELS)])) >= 1
    w = 2048
    while not ok(w):
        w += 1
    assert not ok(w - 1)
    L, R = synth.stereo_pair(w, TALL_H, seq=21, f=0)
    kL, dL = exL(L); kR, dR = exR(R)
    oL, oR = ol.OracleExtractor(3000, float(sf), STEREO_LEVELS), ol.OracleExtractor(3000, float(sf), STEREO_LEVELS)
    okL, odL = oL(L); okR, odR = oR(R)
    yield dict(sf=sf, sf_next=sf_next, w=w, L=L, R=R, exL=exL, exR=exR, kL=kL, dL=dL, kR=kR, dR=dR, oL=oL, oR=oR, okL=okL,
               odL=odL, okR=okR, odR=odR)
    exL.close(); exR.close()


@pytest.fixture(scope="module")
def lv16():
    """a full-HD frame at 16 levels, scale factor 1.08: level 15 (605 x 340) still has FAST cells"""
    img = np.tile(synth.frame(960, 540, seq=7, f=1), (2, 2))
    ex, orc = ORBextractor(4000, 1.08, 16), ol.OracleExtractor(4000, 1.08, 16)
    k, d = ex(img)
    ok, od = orc(img)
    yield dict(img=img, ex=ex, orc=orc, k=k, d=d, ok=ok, od=od, sf=ex.GetScaleFactors(), inv_s2=ex.GetInverseScaleSigmaSquares())
    ex.close()


# ------------------------------------------------------------------------------------------------------------- 1. image size
@pytest.mark.parametrize("w,h", [(4095, 300)], ids=["w4095"])
def test_widest_image_sets_bit_11_of_x(w, h):
    img = synth.frame(w, h, seq=7, f=1)
    ex, orc = ORBextractor(3000), ol.OracleExtractor(3000)
    k, d = ex(img)
    ok, od = orc(img)
    _compare_stages(ex, orc, k, d, ok, od, 8)
    assert (orc.level_keypoints(0)["x"] >= 2048).sum() > 100 and (k["x"] >= 4000).any()
    ex.close()


@pytest.mark.parametrize("h", [TALL_H], ids=["h4095-nIni1-16levels"])
def test_tallest_image_sets_bit_11_of_y(tall, h):
    t = tall
    assert t["L"].shape == (h, t["w"])
    _compare_stages(t["exL"], t["oL"], t["kL"], t["dL"], t["okL"], t["odL"], STEREO_LEVELS)
    np.testing.assert_array_equal(t["kR"], t["okR"]); np.testing.assert_array_equal(t["dR"], t["odR"])
    assert (t["oL"].level_keypoints(0)["y"] >= 2048).sum() > 100


@pytest.mark.parametrize("size", [4095], ids=[f"4095x4095-max_nodes{NODE_MAX}"])
def test_largest_image_with_a_full_node_table(big, size):
    b = big
    assert NODE_MAX == 2752 and b["img"].shape == (size, size) and _node_table(b["nf"]) == NODE_MAX
    n0 = b["orc"].features_per_level[0]
    assert n0 + 4 > NODE_MAX - 64                             # the level-0 lists fill the last 64-node block
    assert len(b["orc"].level_candidates(0)[0]) > 10 * n0 and len(b["orc"].level_keypoints(0)) >= n0
    _compare_stages(b["ex"], b["orc"], b["k"], b["d"], b["ok"], b["od"], 8)
    assert (b["k"]["x"] >= 2048).any() and (b["k"]["y"] >= 2048).any()


def test_refused_image_sizes_and_node_table(big, tall):
    ex = ORBextractor(1000)
    for w, h in ((4096, 300), (2048, 4096)):
        _refused(_extract_raw, ex, np.zeros((h, w), np.uint8), match="unsupported image size")
    img = synth.frame(640, 480, seq=3, f=0)
    k, d = ex(img)                                        # the handle still works
    ok, od = ol.OracleExtractor(1000)(img)
    np.testing.assert_array_equal(k, ok); np.testing.assert_array_equal(d, od)
    # the narrowest 4095-row image whose levels all have nIni >= 1 is accepted (test_tallest_image_...), one pixel less is not
    t = tall
    ex16 = ORBextractor(3000, float(t["sf"]), STEREO_LEVELS)
    _refused(_extract_raw, ex16, np.ascontiguousarray(t["L"][:, : t["w"] - 1]), match="nIni=0")
    k16, d16 = ex16(t["L"])
    np.testing.assert_array_equal(k16, t["okL"]); np.testing.assert_array_equal(d16, t["odL"])
    ex16.close()
    # nFeatures one above the node table's limit
    assert _node_table(big["nf"] + 1) > NODE_MAX
    ex2 = ORBextractor(big["nf"] + 1)
    _refused(_extract_raw, ex2, big["img"], match="octree LDS")
    ex2.close()
    k, d = ex(img)
    np.testing.assert_array_equal(k, ok); np.testing.assert_array_equal(d, od)
    ex.close()


# ------------------------------------------------------------------------------------------------------------- 2. 16 levels
@pytest.mark.parametrize("nlevels", [16], ids=["levels16-octave15"])
def test_sixteen_level_extraction(lv16, nlevels):
    v = lv16
    _compare_stages(v["ex"], v["orc"], v["k"], v["d"], v["ok"], v["od"], nlevels)
    assert (v["k"]["octave"] == 15).sum() > 20


def _self_queries(k, d, sf, th, seed):
    rng = np.random.default_rng(seed)
    q = make_queries(len(k))
    q["u"] = k["x"] + rng.normal(0, 0.7, len(k)).astype(np.float32)
    q["v"] = k["y"] + rng.normal(0, 0.7, len(k)).astype(np.float32)
    q["u_r"] = q["u"] - np.float32(20.0)
    q["radius"] = np.float32(th) * sf[k["octave"]]
    q["min_level"] = k["octave"] - 1
    q["max_level"] = k["octave"] + 1
    q["valid"] = (rng.random(len(k)) < 0.95).astype(np.int32)
    q["blocks"] = (rng.random(len(k)) < 0.5).astype(np.int32)
    q["angle"] = k["angle"]
    q["desc"] = d
    return q


@pytest.mark.parametrize("nlevels", [16], ids=["octave15"])
def test_sixteen_level_searches(lv16, nlevels):
    """SearchByProjectionFrame, proj_match_batch mode 1 and KeyFrameSearch (Fuse, 16 inv_level_sigma2 entries) on keypoints of
    octaves 0..15: the octave travels in the 4-bit field of the projection resolver"""
    import torch
    v = lv16
    k, d, sf = v["k"], v["d"], v["sf"]
    h, w = v["img"].shape
    top = k["octave"] == nlevels - 1
    q = _self_queries(k, d, sf, 7.0, 3)
    fv, of = FrameView(k, d, 0, w, 0, h), ol.OracleFrame(k, d, sf, 0, w, 0, h)
    nm, assigned, blocked = ORBmatcher(0.9, True).SearchByProjectionFrame(fv, q)
    onm, oassigned, oblocked = of.search_by_projection_frame(q, True)
    assert nm == onm
    np.testing.assert_array_equal(assigned, oassigned); np.testing.assert_array_equal(blocked, oblocked)
    assert (assigned[top] >= 0).sum() > 10
    # the device batch entry point, mode 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a).cuda()
    n = len(k)
    t_k, t_d, t_n, t_q = dev(k[None]), dev(d[None]), dev(np.array([n], np.int32)), dev(q[None])
    t_nq = dev(np.array([n], np.int32))
    t_blocked = torch.zeros((1, n), dtype=torch.uint8, device="cuda")
    t_assigned = torch.full((1, n), -1, dtype=torch.int32, device="cuda"); t_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    m = Matcher()
    m.proj_match_batch(t_k, t_d, t_n, None, (0.0, float(w), 0.0, float(h)), t_q, t_nq, 1, 0.9, True, t_blocked, t_assigned, t_nm, stream=s)
    s.synchronize()
    assert int(t_nm[0]) == onm
    np.testing.assert_array_equal(t_assigned[0].cpu().numpy(), oassigned)
    np.testing.assert_array_equal(t_blocked[0].cpu().numpy(), oblocked)
    m.close()
    # Fuse through orbfe_kf_search: points predicted at every level, inv_level_sigma2 with 16 entries
    R, t = synth.camera_pose(77)
    fr = make_frustum(R, t, 1000.0, 1000.0, 960.0, 540.0, 50.0, (0, w, 0, h), 1.08, nlevels)
    np.testing.assert_array_equal(fr["scale_factors"][0, :nlevels], sf)
    mp = synth.local_map(k, d, fr, 78, n_extra=300)
    cam = np.zeros(1, _lib.KF_CAMERA_DTYPE)
    for f in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y", "log_scale_factor", "n_levels"):
        cam[f] = fr[f]
    cam["R"] = fr["Rcw"]; cam["t"] = fr["tcw"]; cam["Ow"] = fr["Ow"]; cam["scale_factors"] = fr["scale_factors"]; cam["th"] = 3.0
    pts = np.zeros(len(mp), _lib.KF_POINT_DTYPE)
    for f in ("pos", "normal", "min_distance", "max_distance", "skip", "desc"):
        pts[f] = mp[f]
    pts["angle"] = np.random.default_rng(79).uniform(0, 360, len(pts)).astype(np.float32)
    assert len(v["inv_s2"]) == 16
    nk, res, _ = ORBmatcher(0.8, True).KeyFrameSearch(fv, cam, pts, _lib.KF_FUSE, inv_level_sigma2=v["inv_s2"])
    onk, ores, _ = ol.kf_search(of, cam, pts, 1, inv_level_sigma2=v["inv_s2"])
    for f in ("best_idx", "best_dist", "level", "u", "v", "u_r"):
        np.testing.assert_array_equal(res[f], ores[f], err_msg=f)
    assert nk == onk
    hit = res["best_idx"] >= 0
    assert (k["octave"][res["best_idx"][hit]] == 15).sum() > 10 and (res["level"] == 15).any()


# ------------------------------------------------------------------------------------------------------------- 3. stereo keys
@pytest.mark.parametrize("rows", [TALL_H], ids=["rows4095-levels16-keys8192"])
def test_stereo_at_the_key_limit(tall, rows):
    import torch
    from refactored_orb_slam2_amd.matcher import compute_stereo_matches
    t = tall
    sf, w = t["sf"], t["w"]
    assert ((rows + 7) // 8) * STEREO_LEVELS == 8192
    gsf = t["exL"].GetScaleFactors()
    assert gsf[-1] <= np.float32(13) and 2 * gsf[-1] + 2 <= 28
    mbf, mb = np.float32(386.1448), np.float32(386.1448 / 718.856)
    oL, oR = t["oL"], t["oR"]
    pL = [oL.level_pixels(l).copy() for l in range(STEREO_LEVELS)]; pR = [oR.level_pixels(l).copy() for l in range(STEREO_LEVELS)]
    on, our, odepth = ol.compute_stereo_matches(t["okL"], t["odL"], t["okR"], t["odR"], pL, pR, oL.scale_factors, oL.inv_scale_factors,
                                                float(mbf), float(mb))
    matched = our >= 0
    assert on > len(t["okL"]) // 4 and (t["okL"]["y"][matched] >= 2048).any() and (t["okL"]["octave"][matched] >= 13).any()
    # host entry point, on the pyramids of the fixture's extractors
    nm, ur, depth = compute_stereo_matches(t["exL"], t["exR"], t["kL"], t["dL"], t["kR"], t["dR"], mbf, mb)
    assert ur.tobytes() == our.tobytes() and depth.tobytes() == odepth.tobytes() and nm == on
    # device entry point
    exL, exR = ORBextractor(3000, float(sf), STEREO_LEVELS), ORBextractor(3000, float(sf), STEREO_LEVELS)
    cap = exL.max_keypoints(w, rows)
    mk = lambda: (torch.zeros((1, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((1, cap, 32), dtype=torch.uint8, device="cuda"),
                  torch.zeros(1, dtype=torch.int32, device="cuda"))
    kl, dl, nl = mk(); kr, dr, nr = mk()
    ur_d = torch.zeros((1, cap), dtype=torch.float32, device="cuda"); depth_d = torch.zeros((1, cap), dtype=torch.float32, device="cuda")
    nmatched = torch.zeros(1, dtype=torch.int32, device="cuda")
    Lt, Rt = torch.from_numpy(t["L"][None].copy()).cuda(), torch.from_numpy(t["R"][None].copy()).cuda()
    torch.cuda.synchronize()
    exL.extract_batch_device(Lt, kl, dl, nl); exR.extract_batch_device(Rt, kr, dr, nr)
    exL.sync(); exR.sync()
    m = Matcher()
    m.stereo_match(exL, exR, kl, dl, nl, kr, dr, nr, float(mbf), float(mb), ur_d, depth_d, nmatched)
    m.sync()
    n_l = int(nl[0])
    assert n_l == len(t["okL"])
    assert ur_d[0, :n_l].cpu().numpy().tobytes() == our.tobytes() and depth_d[0, :n_l].cpu().numpy().tobytes() == odepth.tobytes()
    assert int(nmatched[0]) == on
    m.close(); exL.close(); exR.close()


def test_stereo_refuses_the_next_scale_factor(tall):
    """one float32 step above the largest scale factor: scale[15] > 13, refused by both entry points before any kernel; the next
    valid call on the same (per-thread) matcher still equals the first"""
    from refactored_orb_slam2_amd.matcher import compute_stereo_matches
    t = tall
    sf_next = float(t["sf_next"])
    L, R = synth.stereo_pair(1241, 376, seq=14, f=3)
    exL, exR = ORBextractor(2000, sf_next, STEREO_LEVELS), ORBextractor(2000, sf_next, STEREO_LEVELS)
    assert exL.GetScaleFactors()[-1] > np.float32(13)
    kL, dL = exL(L); kR, dR = exR(R)
    mbf, mb = np.float32(386.1448), np.float32(386.1448 / 718.856)
    _refused(compute_stereo_matches, exL, exR, kL, dL, kR, dR, mbf, mb, match="too large for the row buckets")
    exL.close(); exR.close()
    nm1, ur1, d1 = compute_stereo_matches(t["exL"], t["exR"], t["kL"], t["dL"], t["kR"], t["dR"], mbf, mb)
    nm2, ur2, d2 = compute_stereo_matches(t["exL"], t["exR"], t["kL"], t["dL"], t["kR"], t["dR"], mbf, mb)
    assert nm1 == nm2 > 0 and ur1.tobytes() == ur2.tobytes() and d1.tobytes() == d2.tobytes()


# ------------------------------------------------------------------------------------------------------------- 4. 65 535 descriptors
def _bf_oracle(A, B, gA=None, gB=None):
    out = [ol.hamming_bf(A[i:i + 16], B, None if gA is None else gA[i:i + 16], gB) for i in range(0, len(A), 16)]
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


def _check_bf(out, ref):
    np.testing.assert_array_equal(out["best_idx"], ref[0]); np.testing.assert_array_equal(out["best_dist"], ref[1])
    np.testing.assert_array_equal(out["second_dist"], ref[2])


@pytest.mark.parametrize("nB", [65535], ids=["strideB65535"])
def test_brute_force_at_65535(nB):
    import torch
    rng = np.random.default_rng(65535)
    A = rng.integers(0, 256, (128, 32), dtype=np.uint8); B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
    A[0] = B[nB - 1]                                       # unique best at the last index
    B[nB - 2] = B[nB - 3] = A[1]                           # a tie at the top of the range: the lower index wins
    B[9] = B[nB - 4] = A[2]                                # a tie across the range
    gB = rng.integers(0, 40, nB).astype(np.int32); gA = rng.integers(0, 40, len(A)).astype(np.int32)
    gA[0] = gB[nB - 1]; gB[nB - 2] = gB[nB - 3] = gA[1]; gB[9] = gB[nB - 4] = gA[2]
    out = ORBmatcher.BruteForce(A, B)
    ref = _bf_oracle(A, B)
    _check_bf(out, ref)
    assert tuple(out[0]) == (nB - 1, 0, ref[2][0]) and tuple(out[1])[:2] == (nB - 3, 0) and tuple(out[2])[:2] == (9, 0)
    outg = ORBmatcher.BruteForce(A, B, gA, gB)
    refg = _bf_oracle(A, B, gA, gB)
    _check_bf(outg, refg)
    assert outg[0]["best_idx"] == nB - 1 and outg[1]["best_idx"] == nB - 3
    # strideB = 65536 is refused (B holds 65536 rows, so nothing would be out of bounds even if it were not)
    L = _lib.lib()
    dA = torch.from_numpy(A).cuda(); dB = torch.from_numpy(np.concatenate([B, B[:1]])).cuda()
    nA_t = torch.tensor([len(A)], dtype=torch.int32, device="cuda"); nB_t = torch.tensor([nB + 1], dtype=torch.int32, device="cuda")
    res = torch.zeros((len(A), 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _refused(lambda: _lib.check(L.orbfe_hamming_bf_device(_lib.ptr(dA), _lib.ptr(nA_t), len(A), len(A), _lib.ptr(dB), _lib.ptr(nB_t), nB + 1,
                                                          None, None, None, 1, _lib.ptr(res), C.c_void_p(None)), "orbfe_hamming_bf_device"),
             match="strideB must be < 65536")
    _check_bf(ORBmatcher.BruteForce(A, B), ref)


@pytest.mark.parametrize("nB", [8192, 8193], ids=["sorted8192", "scan8193"])
def test_grouped_brute_force_at_the_sort_limit(nB):
    """grouped brute force with B at HBF_MAX_SORT (in-LDS sort by group) and one above (plain scan with the group test); one group
    holds most of B.  B[8192] belongs to a group no row of A asks for, so both sizes give the same answer."""
    rng = np.random.default_rng(8192)
    A = rng.integers(0, 256, (256, 32), dtype=np.uint8); B = rng.integers(0, 256, (8193, 32), dtype=np.uint8)
    gB = np.where(rng.random(8193) < 0.9, 5, rng.integers(0, 30, 8193)).astype(np.int32); gB[8192] = 999
    gA = np.where(rng.random(256) < 0.8, 5, rng.integers(0, 30, 256)).astype(np.int32)
    A[:20] = B[rng.integers(0, 8192, 20)]
    B[8191] = B[100]; gB[8191] = gB[100]; A[20] = B[100]; gA[20] = gB[100]
    outs = {n: ORBmatcher.BruteForce(A, B[:n], gA, gB[:n]) for n in (8192, 8193)}
    ref = _bf_oracle(A, B[:nB], gA, gB[:nB])
    _check_bf(outs[nB], ref)
    assert outs[8192].tobytes() == outs[8193].tobytes() and outs[nB][20]["best_idx"] == 100


@pytest.mark.parametrize("n", [65535], ids=["keypoints65535"])
def test_proj_best_on_the_largest_frame(n):
    """orbfe_proj_best on a 65 535-keypoint frame (queries on the top indices), and a 65 536-keypoint frame refused on the host"""
    rng = np.random.default_rng(n)
    w, h = 1241, 376
    k = np.zeros(n + 1, ol.KP_DTYPE)
    k["x"] = rng.uniform(0, w, n + 1).astype(np.float32); k["y"] = rng.uniform(0, h, n + 1).astype(np.float32)
    k["octave"] = rng.integers(0, 8, n + 1); k["angle"] = rng.uniform(0, 360, n + 1).astype(np.float32); k["size"] = 31
    d = rng.integers(0, 256, (n + 1, 32), dtype=np.uint8)
    sf = np.array([np.float32(1.2) ** i for i in range(8)], np.float32)
    fv, of = FrameView(k[:n], d[:n], 0, w, 0, h), ol.OracleFrame(k[:n], d[:n], sf, 0, w, 0, h)
    nq = 256
    src = np.concatenate([np.arange(n - 128, n), rng.integers(0, n, nq - 128)])
    q = make_queries(nq)
    q["u"] = k["x"][src]; q["v"] = k["y"][src]; q["u_r"] = q["u"]; q["radius"] = np.float32(6.0)
    q["min_level"] = k["octave"][src] - 1; q["max_level"] = k["octave"][src]   # Fuse's nPredictedLevel-1 .. nPredictedLevel
    q["desc"] = d[src]; q["desc"][1::2, :4] ^= 0x11          # half exact, half a few bits off
    bi, bd = ORBmatcher().ProjBest(fv, q)
    obi, obd = of.proj_best(q)
    np.testing.assert_array_equal(bi, obi); np.testing.assert_array_equal(bd, obd)
    assert (bi == n - 1).any() and (bi >= 65280).sum() > 64
    m = ORBmatcher()
    _refused(m.ProjBest, FrameView(k, d, 0, w, 0, h), q, match="at most 65535")
    _refused(m.ProjCandidates, FrameView(k, d, 0, w, 0, h), q, match="at most 65535")
    bi2, bd2 = m.ProjBest(fv, q)
    np.testing.assert_array_equal(bi2, obi); np.testing.assert_array_equal(bd2, obd)


@pytest.mark.parametrize("nB", [60000], ids=["node60000"])
def test_search_by_bow_node_of_60000(nB):
    rng = np.random.default_rng(60000)
    nA = 48
    dB = rng.integers(0, 256, (nB + 1, 32), dtype=np.uint8); aB = rng.uniform(0, 360, nB + 1).astype(np.float32)
    src = np.concatenate([[nB - 1, nB - 2], rng.integers(0, nB, nA - 2)])
    dA = dB[src].copy(); dA[3::3, :2] ^= 0x03              # exact and near copies, the last frame feature included
    aA = (aB[src] + rng.normal(0, 2, nA)).astype(np.float32) % np.float32(360)
    vA = (rng.random(nA) < 0.9).astype(np.uint8); vA[:2] = 1
    gA = {11: list(range(nA // 2)), 12: list(range(nA // 2, nA))}
    gB = {11: list(range(nB))}
    m = ORBmatcher(0.7, True)
    nm, mB = m.SearchByBoW(dA, aA, vA, gA, dB[:nB], aB[:nB], gB)
    onm, omB = ol.search_by_bow(dA, aA, vA, gA, dB[:nB], aB[:nB], gB, nnratio=0.7)
    assert nm == onm and nm > 10
    np.testing.assert_array_equal(mB, omB)
    assert mB[nB - 1] == 0
    _refused(m.SearchByBoW, dA, aA, vA, gA, dB, aB, {11: list(range(nB + 1))}, match="at most 60000")
    nm2, mB2 = m.SearchByBoW(dA, aA, vA, gA, dB[:nB], aB[:nB], gB)
    assert nm2 == onm and np.array_equal(mB2, omB)


# ------------------------------------------------------------------------------------------------------------- 5. ordered resolvers at 9 500
def _subsample(k, d, n, seed):
    idx = np.sort(np.random.default_rng(seed).choice(len(k), n, replace=False))
    return k[idx].copy(), d[idx].copy()


@pytest.mark.parametrize("n", [9500], ids=["cap9500"])
def test_ordered_resolvers_at_9500(big, n):
    import torch
    b = big
    sf = b["ex"].GetScaleFactors()
    frames = [_subsample(b["k"], b["d"], n, s) for s in (1, 2)]
    w = h = 4095
    # host pointers: SearchByProjectionFrame with n = 9500, and 9501 refused
    k, d = frames[0]
    q = _self_queries(k, d, sf, 15.0, 5)
    rng = np.random.default_rng(6)
    blocked0 = (rng.random(n) < 0.05).astype(np.uint8)
    fv, of = FrameView(k, d, 0, w, 0, h), ol.OracleFrame(k, d, sf, 0, w, 0, h)
    mt = ORBmatcher(0.9, True)
    nm, assigned, blocked = mt.SearchByProjectionFrame(fv, q, blocked0)
    onm, oassigned, oblocked = of.search_by_projection_frame(q, True, blocked0)
    assert nm == onm and nm > n // 2
    np.testing.assert_array_equal(assigned, oassigned); np.testing.assert_array_equal(blocked, oblocked)
    assert (assigned[n - 64:] >= 0).any()
    k1, d1 = _subsample(b["k"], b["d"], n + 1, 3)
    _refused(mt.SearchByProjectionFrame, FrameView(k1, d1, 0, w, 0, h), _self_queries(k1, d1, sf, 15.0, 5), match="cap <= 9500")
    # device batch: cap = 9500, every row filled; cap 9501 refused on the same handle first
    F = len(frames)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a).cuda()
    qs = [_self_queries(kk, dd, sf, 15.0, 10 + i) for i, (kk, dd) in enumerate(frames)]
    m = Matcher()
    s = torch.cuda.Stream()
    big_k = np.zeros((F, n + 1), ol.KP_DTYPE); big_d = np.zeros((F, n + 1, 32), np.uint8)
    for i, (kk, dd) in enumerate(frames):
        big_k[i, :n] = kk; big_d[i, :n] = dd
    t_n = dev(np.full(F, n, np.int32))
    t_q = dev(np.stack(qs)); t_nq = dev(np.full(F, n, np.int32))
    t_blocked = torch.zeros((F, n + 1), dtype=torch.uint8, device="cuda")
    t_assigned = torch.full((F, n + 1), -1, dtype=torch.int32, device="cuda"); t_nm = torch.zeros(F, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _refused(m.proj_match_batch, dev(big_k), dev(big_d), t_n, None, (0.0, 4095.0, 0.0, 4095.0), t_q, t_nq, 1, 0.9, True, t_blocked,
             t_assigned, t_nm, s, match="cap <= 9500")
    t_k, t_d = dev(big_k[:, :n]), dev(big_d[:, :n])
    t_blocked = torch.zeros((F, n), dtype=torch.uint8, device="cuda")
    t_assigned = torch.full((F, n), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.proj_match_batch(t_k, t_d, t_n, None, (0.0, 4095.0, 0.0, 4095.0), t_q, t_nq, 1, 0.9, True, t_blocked, t_assigned, t_nm, stream=s)
    s.synchronize()
    for i, (kk, dd) in enumerate(frames):
        onm, oassigned, oblocked = ol.OracleFrame(kk, dd, sf, 0, w, 0, h).search_by_projection_frame(qs[i], True)
        assert int(t_nm[i]) == onm and onm > n // 2
        np.testing.assert_array_equal(t_assigned[i].cpu().numpy(), oassigned)
        np.testing.assert_array_equal(t_blocked[i].cpu().numpy(), oblocked)
    m.close()


# ------------------------------------------------------------------------------------------------------------- 6. initialisation tables in LDS
def test_search_for_initialization_at_the_lds_limit():
    """SearchForInitialization keeps vMatchedDistance and vnMatches21 of the second frame in LDS, 8 bytes per keypoint and 60 KiB at
    the most: 7680 keypoints equal the oracle (the last index matched, so both tables are written at their last entry), 7681 are
    refused on the host before any kernel, and the handle goes on working"""
    n2 = 7680
    rng = np.random.default_rng(n2)
    w, h, n1 = 1241, 376, 600
    k = np.zeros(n2 + 1, ol.KP_DTYPE)
    k["x"] = rng.uniform(0, w, n2 + 1).astype(np.float32); k["y"] = rng.uniform(0, h, n2 + 1).astype(np.float32)
    k["octave"] = rng.integers(0, 3, n2 + 1); k["angle"] = rng.uniform(0, 360, n2 + 1).astype(np.float32); k["size"] = 31
    k["octave"][n2 - 1] = 0
    d = rng.integers(0, 256, (n2 + 1, 32), dtype=np.uint8)
    sf = np.array([np.float32(1.2) ** i for i in range(8)], np.float32)
    # first frame: copies of level-0 keypoints of the second, the last index among them and a third of them twice (the nearer copy
    # comes later and steals), moved by a few pixels and with a few bits turned
    lvl0 = np.flatnonzero(k["octave"][:n2] == 0)
    src = np.concatenate([[n2 - 1], rng.choice(lvl0, n1 - 201, replace=False)])
    src = np.concatenate([src, src[:200]])
    k1 = k[src].copy()
    k1["angle"] = (k1["angle"] + rng.normal(0, 3, n1)).astype(np.float32) % np.float32(360)
    k1["octave"][rng.random(n1) < 0.1] = 1
    d1 = d[src].copy()
    d1[:n1 - 200, :3] ^= 0x15
    d1[n1 - 200:, :1] ^= 0x01
    prev = np.stack([k1["x"] + rng.uniform(-4, 4, n1).astype(np.float32), k1["y"] + rng.uniform(-4, 4, n1).astype(np.float32)], 1)
    prev = prev.astype(np.float32)
    m = ORBmatcher(0.9, True)
    f1 = FrameView(k1, d1, 0, w, 0, h)
    nm, m12, p2 = m.SearchForInitialization(f1, FrameView(k[:n2], d[:n2], 0, w, 0, h), prev, 10)
    onm, om12, op2 = ol.search_for_initialization(k1, d1, ol.OracleFrame(k[:n2], d[:n2], sf, 0, w, 0, h), prev, 10, np.float32(0.9), True)
    assert nm == onm and nm > 200
    np.testing.assert_array_equal(m12, om12)
    assert p2.tobytes() == op2.tobytes()
    assert (m12 == n2 - 1).any() and (m12[:200] == -1).sum() > 100       # the last table entry is used; matches were stolen
    _refused(m.SearchForInitialization, f1, FrameView(k, d, 0, w, 0, h), prev, 10, match="exceeds the LDS-resident tables")
    nm2, m12b, p2b = m.SearchForInitialization(f1, FrameView(k[:n2], d[:n2], 0, w, 0, h), prev, 10)
    assert nm2 == onm and np.array_equal(m12b, om12) and p2b.tobytes() == op2.tobytes()


# ------------------------------------------------------------------------------------------------------------- 7. carry frame
def test_carry_frame_feeds_frame_zero_and_refuses_shift_2():
    """orbfe_track_queries_stereo_device: a carry that differs from the batch's tail changes frame 0's queries (they come from the
    carry, as the oracle computes them); frame_shift 2 without a carry wraps mod F; frame_shift 2 with a carry is refused (the
    carry holds one frame)"""
    import torch
    from refactored_orb_slam2_amd.matcher import track_queries_stereo_batch
    from refactored_orb_slam2_amd._lib import QUERY_DTYPE
    w, h, F = 752, 480, 3
    ex = ORBextractor(1200)
    seq = synth.sequence(w, h, F + 1, seq=31)
    ext = [ex(img) for img in seq]                          # frames 0..F-1 of the batch, then the carry frame
    sf = ex.GetScaleFactors()
    ex.close()
    cap = max(len(k) for k, _ in ext) + 3
    rng = np.random.default_rng(8)
    G = F + 1
    kps = np.zeros((G, cap), ol.KP_DTYPE); desc = np.zeros((G, cap, 32), np.uint8); n = np.zeros(G, np.int32)
    depth = np.full((G, cap), -1, np.float32)
    cams = np.zeros(G, ol.UNPROJECT_CAM_DTYPE); poses = np.zeros(F, ol.TRACK_POSE_DTYPE)
    for i, (k, d) in enumerate(ext):
        kps[i, :len(k)] = k; desc[i, :len(k)] = d; n[i] = len(k)
        z = rng.uniform(2, 60, len(k)).astype(np.float32); z[rng.random(len(k)) < 0.25] = -1
        depth[i, :len(k)] = z
        R, t = synth.camera_pose(300 + i)
        cams["Rwc"][i] = R.T.reshape(9); cams["Ow"][i] = -(R.T @ t)
        cams["cx"][i] = 370.0; cams["cy"][i] = 236.5; cams["invfx"][i] = np.float32(1) / np.float32(458.654)
        cams["invfy"][i] = np.float32(1) / np.float32(457.296)
    for j in range(F):
        R2, t2 = synth.camera_pose(300 + (j - 1) % G)
        poses["Rcw"][j] = R2.reshape(9); poses["tcw"][j] = t2 + np.array([0.05, -0.02, 0.0], np.float32)
        poses["fx"][j] = 458.654; poses["fy"][j] = 457.296; poses["cx"][j] = 367.215; poses["cy"][j] = 248.375; poses["mbf"][j] = 47.9
        poses["min_x"][j] = 0; poses["max_x"][j] = w; poses["min_y"][j] = 0; poses["max_y"][j] = h
        poses["th"][j] = 15.0; poses["scale_factors"][j, :len(sf)] = sf
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a).cuda()
    t_kps, t_desc, t_n, t_depth, t_cams, t_poses = dev(kps), dev(desc), dev(n), dev(depth), dev(cams), dev(poses)
    carry = (t_kps[F].clone(), t_desc[F].clone(), t_n[F:].clone(), t_depth[F].clone(), t_cams[F].clone())
    b = lambda t: t[:F].contiguous()
    t_q = torch.zeros((F, cap, 68), dtype=torch.uint8, device="cuda"); t_nq = torch.zeros(F, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def run(shift, c):
        t_q.fill_(0xAB); t_nq.fill_(-5)
        with torch.cuda.stream(s):
            track_queries_stereo_batch(b(t_kps), b(t_desc), b(t_n), b(t_depth), b(t_cams), 1, t_poses, shift, t_q, t_nq, s, carry=c)
        s.synchronize()
        return t_q.cpu().numpy().reshape(F, cap * 68).view(QUERY_DTYPE).reshape(F, cap), t_nq.cpu().numpy()

    def oracle(j, src):
        k, d = ext[src]
        return ol.track_queries(poses[j:j + 1], ol.unproject_stereo(cams[src:src + 1], k, d, depth[src]))

    assert not np.array_equal(kps[F], kps[F - 1])
    _refused(run, 2, carry, match="frame_shift")
    for shift, c in ((1, carry), (1, None), (2, None)):
        gq, gnq = run(shift, c)
        for j in range(F):
            src = j - shift if j >= shift else (F if c is not None else (j - shift) % F)
            oq = oracle(j, src)
            assert gnq[j] == len(oq)
            assert gq[j, :len(oq)].tobytes() == oq.tobytes(), (shift, c is not None, j)
            if j == 0 and c is not None:
                assert oq["valid"].sum() > 100 and oq.tobytes() != oracle(0, F - 1).tobytes()
