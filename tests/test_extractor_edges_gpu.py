"""The directed extractor scenes of tests/np_extractor.py on the device, stage by stage against the C oracle: every comparison is
exact, every expected value comes from the oracle (tests/test_extractor_edges_cpu.py holds the oracle to the numpy reading and the
scenes to their census).  One image per call (one FAST cell per wave), batches of more than eight images (runs of cells, DMA host
path), the device-resident batch with padded source rows and sentinel-filled outputs; everything twice on one handle."""
import numpy as np
import pytest

from refactored_orb_slam2_amd import ORBextractor
from refactored_orb_slam2_amd._lib import KP_DTYPE
from tests import np_extractor as ne
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

BATCH_PARAMS = ((300, 20, 7), (300, 1, 1))     # every image of a geometry under one parameter set: the usual thresholds, and (1, 1)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def oracle():
    """oracle(geometry, scene index, (nfeatures, ini, min)) -> dict(kps, desc, levels=[dict(size, pixels, blurred, cand, keys)]), computed
    once and left unchanged"""
    cache = {}

    def get(geom, i, params):
        key = (geom, i, params)
        if key not in cache:
            nf, ini, mn = params
            orc = ol.OracleExtractor(nf, ne.SCALE, ne.N_LEVELS, ini, mn)
            k, d = orc(ne.build_scenes(geom)[1][i].image)
            levels = []
            for l in range(ne.N_LEVELS):
                lk = orc.level_keypoints(l)
                levels.append(dict(size=orc.level_size(l), pixels=orc.level_pixels(l), blurred=orc.level_blurred(l),
                                   cand=np.stack(orc.level_candidates(l)),
                                   keys=np.stack([lk["x"], lk["y"], lk["response"]]).astype(np.int32)))
            for a in [k, d] + [v for L in levels for v in L.values() if isinstance(v, np.ndarray)]:
                a.setflags(write=False)
            cache[key] = dict(kps=k, desc=d, levels=levels)
        return cache[key]

    return get


def _explain(scene, params, level, kind, got, want):
    """the first differing FAST cell by (level, row, column) with its census record, or the quadtree call's record"""
    pattern = np.ctypeslib.as_array(ol.lib().oo_pattern(), (1024,)).copy()
    rd = ne.read(scene.image, *params, pattern, census_only=True)
    if kind == "candidates":
        cell, rec = ne.first_differing_cell(rd, level, got, want)
        return f"first differing cell (level, row, column) = {cell}: {rec}"
    return f"quadtree call of level {level}: {rd['levels'][level]['tree']}"


def _check_lists(ex, slot, scene, params, want, tag):
    """debug_candidates and debug_level_keypoints of image `slot`: x, y, score and order, per level"""
    for l, L in enumerate(want["levels"]):
        for kind, got, exp in (("candidates", np.stack(ex.debug_candidates(slot, l)), L["cand"]),
                               ("level keypoints", np.stack(ex.debug_level_keypoints(slot, l)), L["keys"])):
            if got.shape != exp.shape or not np.array_equal(got, exp):
                pytest.fail(f"{tag} {params}: {kind} of level {l} differ ({got.shape[1]} against {exp.shape[1]}); "
                            + _explain(scene, params, l, kind, got, exp))


def _check_outputs(k, d, want, tag):
    assert len(k) == len(want["kps"]), tag
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        np.testing.assert_array_equal(k[f], want["kps"][f], err_msg=f"{tag}: keypoint field {f}")
    np.testing.assert_array_equal(k["angle"].view(np.uint32), want["kps"]["angle"].view(np.uint32), err_msg=f"{tag}: angle bits")
    np.testing.assert_array_equal(d, want["desc"], err_msg=f"{tag}: descriptor bytes")


@pytest.mark.parametrize("geom", list(ne.GEOMETRIES))
def test_every_scene_one_image_per_call(geom, oracle):
    """ORBextractor.__call__ (n_images = 1: one FAST cell per wave) at the scene's own parameters: pyramid and blurred planes,
    candidate lists and quadtree selections with their order, keypoint records with the angle bit for bit, descriptor bytes; twice
    on the same handle (one handle per parameter set, used for all its scenes in turn)."""
    _, scenes = ne.build_scenes(geom)
    handles = {}
    try:
        for i, sc in enumerate(scenes):
            if sc.params not in handles:
                handles[sc.params] = ORBextractor(sc.nfeatures, ne.SCALE, ne.N_LEVELS, sc.ini, sc.mn)
            ex = handles[sc.params]
            want = oracle(geom, i, sc.params)
            tag = f"{geom}/{sc.name}"
            k, d = ex(sc.image)
            for l, L in enumerate(want["levels"]):
                assert ex.level_size(l) == L["size"]
                np.testing.assert_array_equal(ex.debug_pyramid(0, l), L["pixels"], err_msg=f"{tag}: pyramid level {l}")
                if L["blurred"] is not None:
                    np.testing.assert_array_equal(ex.debug_blurred(0, l), L["blurred"], err_msg=f"{tag}: blurred level {l}")
            _check_lists(ex, 0, sc, sc.params, want, tag)
            _check_outputs(k, d, want, tag)
            k2, d2 = ex(sc.image)
            assert k.tobytes() == k2.tobytes() and d.tobytes() == d2.tobytes(), f"{tag}: the second run differs from the first"
            _check_lists(ex, 0, sc, sc.params, want, tag + " (second run)")
    finally:
        for ex in handles.values():
            ex.close()


def _batch_order(n):
    """every scene once, neighbours in the batch far apart in the scene list, so that the images differ from slot to slot"""
    half = (n + 1) // 2
    return [j for pair in zip(range(half), list(range(half, n)) + [None]) for j in pair if j is not None]


@pytest.mark.parametrize("params", BATCH_PARAMS, ids=lambda p: "th%d_%d" % p[1:])
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("geom", list(ne.GEOMETRIES))
def test_all_scenes_of_a_geometry_in_one_batch(geom, form, params, oracle):
    """more than eight images: the launch in which one wave walks a run of up to four cells and restages its LDS slice from cell
    to cell (host form: DMA copies; device form: source rows padded, outputs filled with a sentinel that must survive behind
    n[i]).  Per image: candidate lists, quadtree selections, keypoints and descriptors against the oracle at the batch's
    parameters; the whole batch twice on the same handle, byte for byte."""
    import torch
    g, scenes = ne.build_scenes(geom)
    order = _batch_order(len(scenes))
    assert len(order) >= 9 and sorted(order) == list(range(len(scenes)))
    imgs = [scenes[j].image for j in order]
    ex = ORBextractor(params[0], ne.SCALE, ne.N_LEVELS, params[1], params[2])
    try:
        runs = []
        for rep in range(2):
            if form == "host":
                res = ex.extract_batch(imgs)
            else:
                pad = np.full((len(imgs), g.h, g.w + 29), 0x5A, np.uint8)
                pad[:, :, :g.w] = np.stack(imgs)
                dimg = torch.from_numpy(pad).cuda()[:, :, :g.w]
                cap = ex.max_keypoints(g.w, g.h)
                kps = torch.full((len(imgs), cap, 28), SENTINEL, dtype=torch.uint8, device="cuda")
                desc = torch.full((len(imgs), cap, 32), SENTINEL, dtype=torch.uint8, device="cuda")
                n = torch.full((len(imgs),), -1, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ex.extract_batch_device(dimg, kps, desc, n)
                ex.sync(); ex.device_status()
                hk, hd, hn = kps.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()
                res = []
                for i in range(len(imgs)):
                    c = int(hn[i])
                    assert 0 <= c <= cap
                    assert (hk[i, c:] == SENTINEL).all() and (hd[i, c:] == SENTINEL).all(), f"slot {i}: bytes behind n[i] = {c} were written"
                    res.append((hk[i, :c].copy().view(KP_DTYPE).reshape(-1), hd[i, :c].copy()))
            for slot, j in enumerate(order):
                tag = f"{geom}/{scenes[j].name} ({form} batch, slot {slot}, run {rep})"
                want = oracle(geom, j, params)
                _check_lists(ex, slot, scenes[j], params, want, tag)
                _check_outputs(res[slot][0], res[slot][1], want, tag)
            runs.append(b"".join(k.tobytes() + d.tobytes() for k, d in res))
        assert runs[0] == runs[1]
    finally:
        ex.close()


@pytest.mark.parametrize("geom", list(ne.GEOMETRIES))
def test_recycle_heavy_then_flat_then_again(geom, oracle):
    """one handle, never closed between: the image whose cells recycle their lists, a flat image (zero keypoints), the first image
    again (equal to its first result); then the same three in alternation in one batch of nine"""
    g, scenes = ne.build_scenes(geom)
    i = [s.name for s in scenes].index("dense")
    heavy, flat = scenes[i].image, np.full((g.h, g.w), 77, np.uint8)
    want = oracle(geom, i, scenes[i].params)
    ex = ORBextractor(scenes[i].nfeatures, ne.SCALE, ne.N_LEVELS, scenes[i].ini, scenes[i].mn)
    try:
        k1, d1 = ex(heavy)
        _check_outputs(k1, d1, want, f"{geom}: first")
        k0, d0 = ex(flat)
        assert len(k0) == 0 and d0.shape == (0, 32)
        assert all(len(ex.debug_candidates(0, l)[0]) == 0 for l in range(ne.N_LEVELS))
        k3, d3 = ex(heavy)
        assert k1.tobytes() == k3.tobytes() and d1.tobytes() == d3.tobytes()
        _check_lists(ex, 0, scenes[i], scenes[i].params, want, f"{geom}: third")
        for slot, (k, d) in enumerate(ex.extract_batch([heavy, flat, heavy, flat, flat, heavy, heavy, flat, heavy])):
            if slot in (1, 3, 4, 7):
                assert len(k) == 0, slot
            else:
                _check_outputs(k, d, want, f"{geom}: batch slot {slot}")
                _check_lists(ex, slot, scenes[i], scenes[i].params, want, f"{geom}: batch slot {slot}")
    finally:
        ex.close()
