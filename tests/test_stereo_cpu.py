"""Frame::ComputeStereoMatches on directed input, CPU side: the C oracle against the instrumented reading on every scene of
tests/np_stereo.py, every hand-placed keypoint at the exit it was placed for, and the census -- the proof that the directed input
reaches what the extractor's own keypoints do not (window guards, piece clamp, long candidate runs, Hamming and SAD ties, the
disparity gate with its 0.01 clamp, small and tied median populations).  tests/test_stereo_gpu.py runs the same scenes on the device."""
import functools
import os

import numpy as np
import pytest

from refactored_orb_slam2_amd import synth
from tests import np_restatement as nr
from tests import np_stereo as ns
from tests import oracle_lib as ol


@functools.lru_cache(maxsize=None)
def planes(w, h, seed=0):
    """the oracle's pyramids of the builder's image pair"""
    L, R, scenes, b = ns.build_scenes(w, h, seed)
    oL, oR = ol.OracleExtractor(200, ns.SCALE, ns.N_LEVELS), ol.OracleExtractor(200, ns.SCALE, ns.N_LEVELS)
    oL(L); oR(R)
    pL = [oL.level_pixels(l).copy() for l in range(ns.N_LEVELS)]; pR = [oR.level_pixels(l).copy() for l in range(ns.N_LEVELS)]
    assert [p.shape[::-1] for p in pL] == b.sizes and [p.shape[::-1] for p in pR] == b.sizes
    np.testing.assert_array_equal(oL.scale_factors, b.sf); np.testing.assert_array_equal(oL.inv_scale_factors, b.isf)
    return pL, pR


@functools.lru_cache(maxsize=None)
def walked(w, h):
    """[(scene, mvuRight, mvDepth, exits, facts)] of the reading, once per geometry"""
    _, _, scenes, b = ns.build_scenes(w, h)
    pL, pR = planes(w, h)
    return [(sc,) + ns.stereo_exits(*sc.arrays(), pL, pR, b.sf, b.isf, sc.mbf, sc.mb) for sc in scenes]


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_oracle_equals_reading_on_directed_scenes(geom):
    _, _, scenes, b = ns.build_scenes(*geom)
    pL, pR = planes(*geom)
    for sc, ur, depth, exits, facts in walked(*geom):
        kL, dL, kR, dR = sc.arrays()
        n, our, odepth = ol.compute_stereo_matches(kL, dL, kR, dR, pL, pR, b.sf, b.isf, float(sc.mbf), float(sc.mb))
        assert our.tobytes() == ur.tobytes() and odepth.tobytes() == depth.tobytes(), sc.name
        assert n == int((ur >= 0).sum()), sc.name
        assert np.array_equal(ur >= 0, np.isin(exits, (ns.SX_MATCHED, ns.SX_CLAMPED))), sc.name


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_every_keypoint_takes_the_exit_it_was_placed_for(geom):
    for sc, ur, depth, exits, facts in walked(*geom):
        kL = sc.arrays()[0]
        assert np.all((kL["x"] >= 0) & (kL["x"] < geom[0]) & (kL["y"] >= 0) & (kL["y"] < geom[1])), sc.name   # the input domain
        for i, want in enumerate(sc.expect):
            if want is not None:
                assert exits[i] == want, (sc.name, i, kL[i], ns.EXIT_NAMES[want], ns.EXIT_NAMES.get(int(exits[i]), int(exits[i])))
        pk = facts["per_keypoint"]
        for i in sc.tags.get("touch", []):
            assert pk["touches"][i], (sc.name, i)
        for i in sc.tags.get("tie", []):       # two candidates at distance 0 with different x; the lower index is the partner
            assert pk["hamming_ties"][i] == 1 and pk["hamming_ties_dx"][i] and pk["best_dist"][i] == 0, (sc.name, i)
        for i in sc.tags.get("sad_tie", []):   # shifts 1 and 2 tie at 0: the first wins, deltaR = d1 / (2 d1)
            assert pk["sad_ties"][i] == 1 and pk["sad"][i] == 0 and pk["best_inc"][i] == 1 and pk["delta"][i] == np.float32(0.5), (sc.name, i)
        for i in sc.tags.get("sad_tie_end", []):
            assert pk["sad_ties"][i] == 1 and pk["sad"][i] == 0 and pk["best_inc"][i] == -5, (sc.name, i)
        for i in sc.tags.get("clamp", []):     # disparity exactly 0: mvuRight = uL - 0.01, mvDepth = mbf / 0.01f
            assert pk["delta"][i] == 0 and ur[i] == np.float32(float(kL["x"][i]) - 0.01) and depth[i] == sc.mbf / np.float32(0.01), (sc.name, i)
        for i in sc.tags.get("min_u", []):
            assert pk["at_min_u"][i] == 1, (sc.name, i)
        for flips in (73, 74, 75, 76, 99):
            for i in sc.tags.get(f"flip{flips}", []):
                assert pk["best_dist"][i] == flips, (sc.name, i)
        if sc.name == "long_run":
            assert facts["longest_run"] == 150
        if sc.name in ns.MEDIAN_POPULATIONS:
            assert facts["median_in"] == sorted(ns.MEDIAN_POPULATIONS[sc.name]), sc.name


@pytest.mark.parametrize("geom", ns.GEOMETRIES)
def test_census(geom):
    """the conditions hold on the reading's own exit codes; none of them reads the kernel's output"""
    results = [(sc, exits, facts) for sc, _, _, exits, facts in walked(*geom)]
    print(geom, ns.exit_counts(results), "longest run", max(f["longest_run"] for _, _, f in results))
    assert ns.census(results) == []
    by_name = {sc.name: (ur, exits, facts) for sc, ur, _, exits, facts in walked(*geom)}
    # what the median rule does with the listed populations, as the reading has it
    assert by_name["median_one"][1].tolist() == [ns.SX_MATCHED]
    assert by_name["median_zeros"][1].tolist() == [ns.SX_MEDIAN] * 3 and np.all(by_name["median_zeros"][0] == -1)
    assert by_name["median_two"][1].tolist() == [ns.SX_MATCHED] * 2
    assert by_name["median_equal"][1].tolist() == [ns.SX_MATCHED] * 4
    assert by_name["median_bin_256"][2]["median"] == 256 and by_name["median_bin_512"][2]["median"] == 512
    ur, exits, facts = by_name["median_cut_100"]
    sad = facts["per_keypoint"]["sad"]
    assert facts["median"] == 100 and sorted(sad.tolist()) == [100, 100, 100, 100, 209, 210, 211]
    th = np.float32(1.5) * np.float32(1.4) * np.float32(100)          # 1.5f * 1.4f * median, as Frame.cc:636-637 forms it
    assert np.array_equal(exits == ns.SX_MEDIAN, sad.astype(np.float32) >= th) and (exits == ns.SX_MEDIAN).any() and (sad[exits == ns.SX_MATCHED] > 100).any()


def test_refactored_reading_gives_the_bytes_it_gave():
    """ref_compute_stereo_matches became a wrapper of stereo_walk: on the stereo input of tests/test_oracle_cpu.py it returns the bytes
    recorded from the function as it was before (tests/golden/stereo_reading_640x360.npz)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "stereo_reading_640x360.npz"))
    w, h, nf = 640, 360, 800
    L, R = synth.stereo_pair(w, h, seq=41, f=2)
    oL, oR = ol.OracleExtractor(nf), ol.OracleExtractor(nf)
    kL, dL = oL(L); kR, dR = oR(R)
    pL = [oL.level_pixels(l).copy() for l in range(8)]; pR = [oR.level_pixels(l).copy() for l in range(8)]
    sf, isf = oL.scale_factors, oL.inv_scale_factors
    for i, (mbf, mb) in enumerate(((np.float32(386.1448), np.float32(386.1448 / 718.856)), (np.float32(47.9), np.float32(0.11)))):
        ur, depth = nr.ref_compute_stereo_matches(kL, dL, kR, dR, pL, pR, sf, isf, mbf, mb)
        assert ur.dtype == np.float32 and depth.dtype == np.float32
        assert ur.tobytes() == g[f"ur_{i}"].tobytes() and depth.tobytes() == g[f"depth_{i}"].tobytes()
        eur, edepth, exits, facts = ns.stereo_exits(kL, dL, kR, dR, pL, pR, sf, isf, mbf, mb)
        assert eur.tobytes() == ur.tobytes() and edepth.tobytes() == depth.tobytes()
        assert np.array_equal(ur >= 0, np.isin(exits, (ns.SX_MATCHED, ns.SX_CLAMPED)))
