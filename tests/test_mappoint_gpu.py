"""GPU suite of the map-point refresh (mappoint_kernels.hip behind orbfe_refresh_map_points and orbfe_refresh_map_points_batch_device)
against the literal reading of tests/np_mappoint.py.  Everything is compared byte for byte: best, desc, n_live, status and the five
floats as bit patterns.  The shapes are the smallest at which the kernels can go wrong: one observation, the wave's 64 and the
workgroup's 256 and 1 024 from both sides, with the number of LIVE observations varied around the same boundaries; a distance of
256; identical descriptors; keyframes that are all bad; empty points; each flag alone over a canary pattern; refused points between
good ones; canaries around the output array; a point alone, in a batch and at another position; two runs; the host form; and, for
two observations, the bytes orbfe_triangulate_matches writes for the same pair."""
import numpy as np
import pytest
import torch

from refactored_orb_slam2_amd import _lib, map_point, mapping
from tests import np_mapping
from tests import np_mappoint as M
from tests.test_mappoint_cpu import _all_bad, _identical, refusal_scene

pytestmark = pytest.mark.gpu
BOTH = M.DESCRIPTOR | M.NORMAL_DEPTH
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 66, 255, 256, 257, 1023, 1024)
GUARD = 3   # canary records on either side of the output array


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()


class Resident:
    """a scene in device memory: every keyframe's descriptor block, the table with their device addresses, the packed points"""

    def __init__(self, scene, stride=12):
        self.scene = scene
        table, obs, recs, positions, _ = map_point.pack_map_points(scene["keyframes"], scene["points"])
        blocks = [np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32) for kf in scene["keyframes"]]
        offs = np.cumsum([0] + [b.size for b in blocks])
        self.desc = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks] + [np.zeros(32, np.uint8)])).cuda()
        table["desc"] = self.desc.data_ptr() + offs[:-1]
        rec = np.zeros((len(recs), stride), np.uint8)
        rec[:, :12] = positions.view(np.uint8).reshape(len(recs), 12)
        rec[:, 12:] = 0x5A
        self.stride, self.P = stride, len(recs)
        self.table, self.obs, self.recs, self.pos = _dev(table), _dev(obs), _dev(recs), torch.from_numpy(rec).cuda()
        self.obs_np, self.recs_np = obs, recs

    def run(self, flags=BOTH, prior=None, subset=None):
        """the records of the points `subset` (default: all, in order) after one call; the guard records on both sides must survive"""
        idx = list(range(self.P)) if subset is None else list(subset)
        recs = _dev(self.recs_np[idx]) if subset is not None else self.recs
        pos = self.pos[idx].contiguous() if subset is not None else self.pos
        n = len(idx)
        buf = np.full((n + 2 * GUARD, 64), 0xC3, np.uint8)
        if prior is not None:
            buf[GUARD:GUARD + n] = prior.view(np.uint8).reshape(n, 64)
        out = torch.from_numpy(buf).cuda()
        map_point.refresh_map_points_device(self.table, self.obs, recs, pos, self.stride, self.scene["scale_factors"], flags, out[GUARD:])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:GUARD] == 0xC3).all() and (got[GUARD + n:] == 0xC3).all(), "a record outside the output array was written"
        return got[GUARD:GUARD + n].copy().view(_lib.MP_UPDATE_DTYPE).reshape(n)


def _canary(n):
    return np.full((n, 64), 0xC3, np.uint8).view(_lib.MP_UPDATE_DTYPE).reshape(n)


def _same(got, want):
    if got.tobytes() == want.tobytes():
        return True
    for i in range(len(got)):
        if got[i].tobytes() != want[i].tobytes():
            print("point", i, "\n got ", got[i], "\n want", want[i])
            break
    return False


@pytest.fixture(scope="module")
def ragged():
    """three points of every small size and two of every large one, shuffled, empty points between them"""
    sizes = [n for n in SIZES for _ in range(3 if n < 255 else 2)] + [0, 0, 0]
    sizes = [sizes[i] for i in np.random.default_rng(1).permutation(len(sizes))]
    scene = M.make_scene(101, sizes)
    return Resident(scene, stride=44), M.run(scene, BOTH, prior=_canary(len(sizes)))


def test_ragged_batch_equals_the_literal_reading(ragged):
    R, want = ragged
    got = R.run(BOTH, prior=_canary(R.P))
    assert _same(got, want)
    assert {int(x) for x in R.recs_np["n_obs"]} == set(SIZES) | {0}
    assert (got["status"] == M.UNCHANGED).sum() == 3 and (got["best"] > 0).sum() >= 15


def test_two_runs_and_the_host_form_give_the_same_bytes(ragged):
    R, want = ragged
    assert R.run(BOTH, prior=_canary(R.P)).tobytes() == want.tobytes()
    s = R.scene
    host = map_point.refresh_map_points(s["keyframes"], s["points"], s["scale_factors"])
    assert _same(host, M.run(s, BOTH))


def test_a_point_alone_in_a_batch_and_at_another_position(ragged):
    R, want = ragged
    pick = [int(np.flatnonzero(R.recs_np["n_obs"] == n)[0]) for n in (1, 5, 64, 65, 257, 1024)]
    for p in pick:
        assert R.run(BOTH, prior=_canary(1), subset=[p]).tobytes() == want[[p]].tobytes(), p
    order = pick[::-1] + pick
    assert R.run(BOTH, prior=_canary(len(order)), subset=order).tobytes() == want[order].tobytes()


@pytest.mark.parametrize("flags", [M.DESCRIPTOR, M.NORMAL_DEPTH])
def test_each_flag_alone_leaves_the_other_half_untouched(ragged, flags):
    R, _ = ragged
    subset = [int(np.flatnonzero(R.recs_np["n_obs"] == n)[0]) for n in (0, 1, 4, 64, 66, 256)]
    scene = dict(R.scene, points=[R.scene["points"][p] for p in subset])
    prior = _canary(len(subset))
    want = M.run(scene, flags, prior=prior)
    assert _same(R.run(flags, prior=prior, subset=subset), want)
    table, obs, recs, positions, keep = map_point.pack_map_points(scene["keyframes"], scene["points"])
    host = map_point.refresh_map_points_batch(table, obs, recs, positions, scene["scale_factors"], flags, updates=prior.copy())
    assert _same(host, want)


def _with_live(seed, n_obs, n_live):
    """one point of n_obs observations of which exactly n_live are of keyframes that are not bad, the bad ones spread over the list"""
    s = M.make_scene(seed, [n_obs], bad_frac=0.0)
    obs = s["points"][0]["obs"]
    for j in np.random.default_rng(seed).permutation(n_obs)[: n_obs - n_live]:
        s["keyframes"][obs[j][0]]["bad"] = True
    return s


@pytest.mark.parametrize("n_obs,lives", [(64, (0, 1, 2, 63, 64)), (65, (0, 1, 63, 64, 65)), (66, (2, 64, 65, 66)), (130, (63, 64, 65, 129)),
                                         (300, (255, 256, 257)), (1024, (1, 64, 65, 1023))])
def test_live_counts_around_every_class_boundary(n_obs, lives):
    for k, n_live in enumerate(lives):
        s = _with_live(1000 * n_obs + k, n_obs, n_live)
        want = M.run(s, BOTH)
        assert want[0]["n_live"] == n_live and (want[0]["best"] >= 0) == (n_live > 0)
        assert _same(Resident(s).run(BOTH), want), (n_obs, n_live)


def test_a_distance_of_256_identical_descriptors_and_all_bad_keyframes():
    s = M.nine_bit_scene()
    got = Resident(s).run(BOTH)
    assert got[0]["best"] == 2 and _same(got, M.run(s, BOTH))
    s = _identical(M.make_scene(6, [2, 9, 64, 90, 300]))
    got = Resident(s).run(BOTH)
    assert (got["best"] == [next(j for j, (kf, _) in enumerate(p["obs"]) if not s["keyframes"][kf]["bad"]) for p in s["points"]]).all()
    assert _same(got, M.run(s, BOTH))
    s = _all_bad(M.make_scene(5, [1, 6, 64, 70, 400]))
    got = Resident(s).run(BOTH, prior=_canary(5))
    assert (got["best"] == -1).all() and (got["n_live"] == 0).all() and not got["desc"].any() and (got["status"] == M.UPDATED).all()
    assert (got["max_distance"] > 0).all() and _same(got, M.run(s, BOTH, prior=_canary(5)))


def test_refused_points_between_good_ones():
    s, broken = refusal_scene()
    R = Resident(s)
    prior = _canary(R.P)
    got, want = R.run(BOTH, prior=prior), M.run(s, BOTH, prior=prior)
    assert _same(got, want)
    assert sorted(np.flatnonzero(got["status"] == M.REFUSED).tolist()) == broken and len(broken) == 16
    good = [p for p in range(R.P) if p not in broken]
    assert R.run(BOTH, prior=_canary(len(good)), subset=good).tobytes() == got[good].tobytes()   # the neighbours' bytes as without them
    # what only the device form can be handed: counts and offsets out of range
    recs = R.recs_np.copy()
    edits = {0: ("n_obs", _lib.MP_MAX_OBS + 1), 2: ("n_obs", -1), 4: ("obs_offset", -1), 6: ("obs_offset", len(R.obs_np) - 2),
             18: ("n_obs", 2 ** 31 - 1), 20: ("obs_offset", 2 ** 31 - 1)}
    for p, (field, val) in edits.items():
        recs[p][field] = val
    R.recs_np, R.recs = recs, _dev(recs)
    again = R.run(BOTH, prior=prior)
    for p in range(R.P):
        if p in edits:
            assert again[p]["status"] == M.REFUSED and again[p]["best"] == -1 and not again[p]["desc"].any() and again[p]["max_distance"] == 0
        else:
            assert again[p].tobytes() == got[p].tobytes(), p


def test_two_observations_give_the_bytes_of_the_triangulation():
    """orbfe_triangulate_matches writes normal / min_distance / max_distance of a new point from its two observations, pKF1 the
    reference keyframe: the refresh of the same point with the list {pKF1, pKF2} and ref = 0 must give the same bytes."""
    t = np_mapping.case_scene("mixed", n=400)
    pts, _ = mapping.triangulate_matches(*np_mapping.scene_args(t))
    rows = np.flatnonzero(pts["code"] == np_mapping.OK)
    assert len(rows) >= 100
    n_levels = int(t["view1"]["n_levels"][0])
    kfs = [dict(desc=np.zeros((1, 32), np.uint8), bad=False, Ow=t["view1"]["Ow"][0]), dict(desc=np.zeros((1, 32), np.uint8), bad=False, Ow=t["view2"]["Ow"][0])]
    points = [dict(obs=[(0, 0), (1, 0)], pos=pts["pos"][i], ref=0, ref_octave=int(t["keys1"]["octave"][i])) for i in rows]
    scene = dict(keyframes=kfs, points=points, scale_factors=t["view1"]["scale_factors"][0][:n_levels])
    got = Resident(scene).run(M.NORMAL_DEPTH)
    for f in ("normal", "min_distance", "max_distance"):
        assert got[f].tobytes() == np.ascontiguousarray(pts[f][rows]).tobytes(), f
    assert _same(got, M.run(scene, M.NORMAL_DEPTH, prior=_canary(len(rows))))
