"""stereo_bucket_kernel / stereo_match_kernel / stereo_median_kernel on the directed scenes of tests/np_stereo.py, through both entry
points.  The extractors only put the pyramids of the builder's image pair into HBM; keypoints and descriptors are the hand-placed
ones.  Expected values: oo_compute_stereo_matches on OracleExtractor planes of the same images; every comparison is on bytes.
tests/test_stereo_cpu.py holds the census of what these scenes reach."""
import ctypes as C
import functools

import numpy as np
import pytest

from refactored_orb_slam2_amd import ORBextractor, _lib
from refactored_orb_slam2_amd.matcher import Matcher, compute_stereo_matches
from tests import np_stereo as ns
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
NF = 200
N_BATCH = 11            # one XCD-remapped group of 8 pairs and a tail of 3


@functools.lru_cache(maxsize=None)
def planes(w, h, seed):
    L, R, scenes, b = ns.build_scenes(w, h, seed)
    oL, oR = ol.OracleExtractor(NF, ns.SCALE, ns.N_LEVELS), ol.OracleExtractor(NF, ns.SCALE, ns.N_LEVELS)
    oL(L); oR(R)
    return ([oL.level_pixels(l).copy() for l in range(ns.N_LEVELS)], [oR.level_pixels(l).copy() for l in range(ns.N_LEVELS)])


def oracle(w, h, seed, kL, dL, kR, dR, maxd):
    """(count, mvuRight, mvDepth) of the oracle for these keypoints on the image pair of `seed`"""
    b = ns.build_scenes(w, h, seed)[3]
    pL, pR = planes(w, h, seed)
    return ol.compute_stereo_matches(kL, dL, kR, dR, pL, pR, b.sf, b.isf, float(maxd[0]), float(maxd[1]))


def level0_tiled(ex):
    t = C.c_int(-1)
    _lib.check(_lib.lib().orbfe_device_pyramid_layout(ex._h, 0, C.byref(t)), "orbfe_device_pyramid_layout")
    return t.value


def combined(w, h, seed=0, first=1):
    """the keypoints of all scenes of one image pair in one set, the scenes from `first` on in front"""
    scenes = ns.build_scenes(w, h, seed)[2]
    parts = [sc.arrays() for sc in scenes[first:] + scenes[:first]]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


# ---- the host entry point ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_pair(w, h):
    """two extractors whose last call was the one-image extraction of the builder's pair: (exL, exR, level 0 tiled?)"""
    L, R, _, _ = ns.build_scenes(w, h, 0)
    exL, exR = ORBextractor(NF, ns.SCALE, ns.N_LEVELS), ORBextractor(NF, ns.SCALE, ns.N_LEVELS)
    exL(L); exR(R)
    assert level0_tiled(exL) == level0_tiled(exR)
    return exL, exR, level0_tiled(exL)


def check_host(w, h, kL, dL, kR, dR, maxd, what):
    exL, exR, _ = host_pair(w, h)
    nm, ur, depth = compute_stereo_matches(exL, exR, kL, dL, kR, dR, maxd[0], maxd[1])
    on, our, odepth = oracle(w, h, 0, kL, dL, kR, dR, maxd)
    assert ur.tobytes() == our.tobytes(), (what, np.flatnonzero(ur.view(np.uint32) != our.view(np.uint32))[:8], ur, our)
    assert depth.tobytes() == odepth.tobytes(), (what, np.flatnonzero(depth.view(np.uint32) != odepth.view(np.uint32))[:8])
    assert nm == on == int((our >= 0).sum()), (what, nm, on)
    return ur, depth


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_host_every_scene(geom):
    """every directed scene as built, one call after the other on the thread's matcher: each call follows one with other keypoints and
    mostly another maxD, so stale sad / bucket / staging contents would show"""
    for sc in ns.build_scenes(*geom)[2]:
        check_host(*geom, *sc.arrays(), (sc.mbf, sc.mb), sc.name)


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_host_unequal_counts(geom):
    """cap = max(n_l, n_r): the slot clamp min(iL, cap - 1) and the idle rows of the short side"""
    kL, dL, kR, dR = combined(*geom)
    by_name = {sc.name: sc for sc in ns.build_scenes(*geom)[2]}
    k2, d2 = by_name["median_two"].arrays()[2:]
    ur, _ = check_host(*geom, kL, dL, k2, d2, ns.KITTI, "n_l >> n_r")
    assert len(kL) > 50 * len(k2) and (ur >= 0).sum() == 2
    e = by_name["edges_l0"].arrays()
    ur, _ = check_host(*geom, e[0][:3], e[1][:3], kR, dR, ns.WIDE, "n_r >> n_l")
    assert len(kR) > 50 * 3 and (ur >= 0).sum() >= 1


@pytest.mark.parametrize("n_l", [1, 15, 16, 17])
@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_host_counts_around_one_workgroup(geom, n_l):
    """sixteen left keypoints per workgroup: one short of it, exactly it, one more, and a single one"""
    kL, dL, kR, dR = combined(*geom)
    ur, _ = check_host(*geom, kL[:n_l], dL[:n_l], kR, dR, ns.WIDE, n_l)
    assert (ur >= 0).sum() >= (n_l + 3) // 4


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_host_reversed_left_keypoints(geom):
    """the left keypoints in reversed order: the same results, permuted"""
    kL, dL, kR, dR = combined(*geom)
    ur, depth = check_host(*geom, kL, dL, kR, dR, ns.KITTI, "forward")
    rur, rdepth = check_host(*geom, kL[::-1].copy(), dL[::-1].copy(), kR, dR, ns.KITTI, "reversed")
    assert rur[::-1].tobytes() == ur.tobytes() and rdepth[::-1].tobytes() == depth.tobytes() and (ur >= 0).sum() > 40


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_host_second_call_equals_the_scene_alone(geom):
    """a long-run scene at maxD = 800, then the disparity scene at maxD = 30 on the same matcher, then the first again: each equals the
    oracle's result for that scene alone"""
    by_name = {sc.name: sc for sc in ns.build_scenes(*geom)[2]}
    a, b = by_name["long_run"], by_name["disparity"]
    ua, _ = check_host(*geom, *a.arrays(), (a.mbf, a.mb), a.name)
    ub, _ = check_host(*geom, *b.arrays(), (b.mbf, b.mb), b.name)
    ua2, _ = check_host(*geom, *a.arrays(), (a.mbf, a.mb), a.name)
    assert ua.tobytes() == ua2.tobytes() and (ua >= 0).sum() == 3 and (ub >= 0).sum() == 17


# ---- the device entry point ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_batch(w, h):
    """two extractors whose last call was a device batch of N_BATCH pairs (pair p: the images of seed p % 3), and a matcher"""
    import torch
    imgs = [ns.build_scenes(w, h, p % 3)[:2] for p in range(N_BATCH)]
    exL, exR = ORBextractor(NF, ns.SCALE, ns.N_LEVELS), ORBextractor(NF, ns.SCALE, ns.N_LEVELS)
    cap = exL.max_keypoints(w, h)
    dev = "cuda"
    L = torch.from_numpy(np.stack([p[0] for p in imgs])).to(dev)
    R = torch.from_numpy(np.stack([p[1] for p in imgs])).to(dev)
    t = dict(cap=cap, images=(L, R))
    for side in "lr":
        t["k" + side] = torch.zeros((N_BATCH, cap, 28), dtype=torch.uint8, device=dev)
        t["d" + side] = torch.zeros((N_BATCH, cap, 32), dtype=torch.uint8, device=dev)
        t["n" + side] = torch.zeros(N_BATCH, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # torch's default stream does not order against the handles' own streams
    exL.extract_batch_device(L, t["kl"], t["dl"], t["nl"])
    exR.extract_batch_device(R, t["kr"], t["dr"], t["nr"])
    exL.sync(); exR.sync()
    assert level0_tiled(exL) == level0_tiled(exR)
    return exL, exR, Matcher(), t, level0_tiled(exL)


def run_batch(w, h, sets, maxd):
    """sets[p] = (kL, dL, kR, dR) of pair p: overwrite the extractors' keypoints with them, match, compare with the oracle"""
    import torch
    exL, exR, m, t, _ = device_batch(w, h)
    cap = t["cap"]
    host = {k: np.zeros(tuple(t[k].shape), np.uint8 if k[0] != "n" else np.int32) for k in ("kl", "dl", "nl", "kr", "dr", "nr")}
    for p, (kL, dL, kR, dR) in enumerate(sets):
        assert len(kL) <= cap and len(kR) <= cap
        host["kl"][p, :len(kL)] = kL.view(np.uint8).reshape(-1, 28); host["dl"][p, :len(kL)] = dL; host["nl"][p] = len(kL)
        host["kr"][p, :len(kR)] = kR.view(np.uint8).reshape(-1, 28); host["dr"][p, :len(kR)] = dR; host["nr"][p] = len(kR)
    for k, v in host.items():
        t[k].copy_(torch.from_numpy(v))
    ur = torch.full((N_BATCH, cap), 7.0, dtype=torch.float32, device="cuda")
    depth = torch.full((N_BATCH, cap), 7.0, dtype=torch.float32, device="cuda")
    nm = torch.full((N_BATCH,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.stereo_match(exL, exR, t["kl"], t["dl"], t["nl"], t["kr"], t["dr"], t["nr"], float(maxd[0]), float(maxd[1]), ur, depth, nm)
    m.sync()
    ur, depth, nm = ur.cpu().numpy(), depth.cpu().numpy(), nm.cpu().numpy()
    total = 0
    for p, (kL, dL, kR, dR) in enumerate(sets):
        on, our, odepth = oracle(w, h, p % 3, kL, dL, kR, dR, maxd)
        n = len(kL)
        assert ur[p, :n].tobytes() == our.tobytes(), (p, np.flatnonzero(ur[p, :n].view(np.uint32) != our.view(np.uint32))[:8])
        assert depth[p, :n].tobytes() == odepth.tobytes(), p
        assert np.all(ur[p, n:] == -1) and np.all(depth[p, n:] == -1), p     # slots beyond n_l and below cap: no match
        assert nm[p] == on, (p, nm[p], on)
        total += on
    return total


def batch_sets(w, h, shift):
    """a different scene for every pair (pair p: scene 1 + (p + shift) % 11 on the images of seed p % 3); pair 2 is filled up to
    n_l == cap, pair 9 has no left keypoints, pair 10 no right ones"""
    cap = device_batch(w, h)[3]["cap"]
    sets = []
    for p in range(N_BATCH):
        scenes = ns.build_scenes(w, h, p % 3)[2]
        kL, dL, kR, dR = scenes[1 + (p + shift) % 11].arrays()
        if p == 2:
            aL, bL, aR, bR = combined(w, h, p % 3, 1 + (p + shift) % 11)
            kL, dL, kR, dR = np.tile(aL, 2)[:cap], np.tile(bL, (2, 1))[:cap], aR[:cap - 5], bR[:cap - 5]
        if p == 9:
            kL, dL = kL[:0], dL[:0]
        if p == 10:
            kR, dR = kR[:0], dR[:0]
        sets.append((kL, dL, kR, dR))
    assert len(sets[2][0]) == cap
    return sets


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_device_batch_of_eleven_pairs(geom):
    """eleven pairs, a scene each, then the same matcher again with the scenes moved on by five pairs and maxD = 30 instead of 800"""
    assert run_batch(*geom, batch_sets(*geom, 0), ns.WIDE) > 60
    assert run_batch(*geom, batch_sets(*geom, 5), ns.NARROW) > 30
    assert run_batch(*geom, batch_sets(*geom, 0), ns.KITTI) > 60


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_both_level0_layouts_are_covered(geom):
    """the SAD windows of the tests above were cut from a tiled level 0 and from a row-major one: today the one-image call leaves
    level 0 in 16 x 8 tiles and a batch of more than eight images row-major.  If the tiling policy changes, this says which layout
    lost its coverage."""
    host, batch = host_pair(*geom)[2], device_batch(*geom)[4]
    by_name = {sc.name: sc for sc in ns.build_scenes(*geom)[2]}
    e = by_name["edges_l0"]
    check_host(*geom, *e.arrays(), (e.mbf, e.mb), e.name)
    assert run_batch(*geom, batch_sets(*geom, 0), ns.WIDE) > 60
    assert 1 in (host, batch), "no stereo test reads a TILED level 0 any more"
    assert 0 in (host, batch), "no stereo test reads a ROW-MAJOR level 0 any more"
