"""The directed extractor scenes of tests/np_extractor.py on the CPU: the census (every edge of EDGES is reached, every scene reaches
the edges it is named for, no directed cell in the "either" band of the recycle verdict), the C oracle against the numpy reading on
every scene, and the same census over the images the GPU suite already had."""
import numpy as np
import pytest

from refactored_orb_slam2_amd import synth
from tests import np_extractor as ne
from tests import np_restatement as nr
from tests import oracle_lib as ol


@pytest.fixture(scope="module")
def pattern():
    return np.ctypeslib.as_array(ol.lib().oo_pattern(), (1024,)).copy()


@pytest.fixture(scope="module")
def readings(pattern):
    """{geometry: (Geometry, scenes, [(scene name, reading)])}: read() itself asserts that the per-cell walk equals
    np_restatement.fast_candidates and the node-list walk np_restatement.distribute_octree"""
    out = {}
    for name in ne.GEOMETRIES:
        g, scenes = ne.build_scenes(name)
        out[name] = (g, scenes, [(s.name, ne.read(s.image, s.nfeatures, s.ini, s.mn, pattern)) for s in scenes])
    return out


def _union(censuses):
    return {e: sorted({(g,) + hit for g, c in censuses.items() for hit in c[e]}) for e in ne.EDGES}


def test_every_edge_is_reached_and_every_scene_reaches_its_own(readings):
    censuses = {name: ne.census(res) for name, (_, _, res) in readings.items()}
    for name, (g, scenes, _) in readings.items():
        for sc in scenes:
            for edge, where in sc.expect:
                assert (sc.name, where) in censuses[name][edge], f"{name}/{sc.name} does not reach {edge} at {where}"
    union = _union(censuses)
    print("\nedge: (geometry, scene, where) of the first scene that reaches it, and how many do")
    for e in ne.EDGES:
        print(f"  {e:40s} {len(union[e]):4d}  {union[e][0] if union[e] else '-'}")
    assert [e for e in ne.EDGES if not union[e]] == []
    assert not any(e in ne.EDGES for e in ne.UNREACHABLE)


def test_no_directed_cell_is_in_the_either_band(readings):
    for name, (_, scenes, res) in readings.items():
        assert ne.either_band(res, scenes) == [], name


def test_geometries_select_the_variants_and_hold_the_levels_they_are_for():
    want = {"wide": "span<=64,rows<=48", "tall": "span<=64,rows>48", "square": "span<=64,rows>48"}
    for name, (w, h) in ne.GEOMETRIES.items():
        assert w <= 430 and h <= 210
        assert ne.kernel_variant(w, h)[0] == want[name]
    inis = {name: [ne.n_ini(lw, lh) for lw, lh in ne.level_sizes(w, h) if nr.level_cells(lw, lh)[0]] for name, (w, h) in ne.GEOMETRIES.items()}
    assert max(inis["wide"]) >= 3 and set(inis["square"]) == {1} and ne.level_sizes(121, 121)[0] == (121, 121)
    g = ne.Geometry("wide")
    assert g.runs == [(0, 4), (4, 4), (8, 4)] and ne.cell_runs(7, 31) == [(0, 4), (4, 3)] and ne.cell_runs(5, 45) == [(0, 3), (3, 2)]
    # tested widths odd and even, first tested columns odd and even, a clipped last column and last row
    cells = g.cells.values()
    assert {c["tw"] % 2 for c in cells} == {0, 1} and {c["x0"] % 2 for c in cells} == {0, 1}
    assert min(c["tw"] for c in cells) < g.wcell and min(c["th"] for c in cells) < g.hcell


def test_no_level_width_reaches_the_96_byte_tile():
    """fast_cells_kernel<96, 7> is chosen when a cell's staged span (x0 & 15) + 1 + cols exceeds 64.  With cells of
    ceil(width / floor(width / 30)) columns it never does: two or more cell columns mean wCell <= 45, a cell of 51 columns is
    wCell = 45 with two columns, whose second cell is clipped to 44; one column means x0 = 16 and at most 59 columns.  Checked
    for every level width up to 4096; the census names the variant of every scene, and no geometry can be given for this one."""
    worst = 0
    for w in range(62, 4097):
        for (_, _, x0, _, x1, _) in nr.level_cells(w, 100)[0]:
            worst = max(worst, (x0 & 15) + 1 + (x1 - x0))
    assert worst <= 64


@pytest.mark.parametrize("name", list(ne.GEOMETRIES))
def test_oracle_matches_the_reading_on_every_scene(readings, name):
    """two independent readings -- literal C loops over cells and node lists, vectorised numpy with its parallel walks -- agree on
    the candidate lists per level, the selected keypoints per level in order, and the final keypoints and descriptors"""
    _, scenes, res = readings[name]
    for sc, (_, rd) in zip(scenes, res):
        orc = ol.OracleExtractor(sc.nfeatures, ne.SCALE, ne.N_LEVELS, sc.ini, sc.mn)
        ok, od = orc(sc.image)
        for l, L in enumerate(rd["levels"]):
            where = f"{name}/{sc.name} level {l}"
            assert orc.level_size(l) == L["size"], where
            np.testing.assert_array_equal(orc.level_pixels(l), L["pixels"], err_msg=where)
            np.testing.assert_array_equal(np.stack(orc.level_candidates(l)), np.stack(L["cand"]), err_msg=where + " candidates")
            k = orc.level_keypoints(l)
            np.testing.assert_array_equal(np.stack([k["x"], k["y"], k["response"]]).astype(np.int64), np.stack([L["kx"], L["ky"], L["ks"]]),
                                          err_msg=where + " selected keypoints")
            if L["blurred"] is not None:
                np.testing.assert_array_equal(orc.level_blurred(l), L["blurred"], err_msg=where + " blurred plane")
        assert len(ok) == len(rd["keypoints"]), f"{name}/{sc.name}"
        for j, field in enumerate(("x", "y", "size", "angle", "response", "octave")):
            np.testing.assert_array_equal(ok[field], np.array([kp[j] for kp in rd["keypoints"]], ok[field].dtype), err_msg=f"{name}/{sc.name} {field}")
        np.testing.assert_array_equal(od, rd["descriptors"], err_msg=f"{name}/{sc.name} descriptors")


def suite_images():
    """the images tests/test_extractor_gpu.py compares whole: synth.frame at its three GEOMS and one image of each kind of
    test_dense_texture_spills_keys_to_hbm, with their parameters"""
    out = [(f"synth.frame {w}x{h}", synth.frame(w, h, seq=3, f=1), nf) for w, h, nf in ((1241, 376, 2000), (640, 480, 1000), (752, 480, 1200))]
    rng = np.random.default_rng(0)
    h, w = 376, 1241
    out.append(("white_noise", rng.integers(0, 256, (h, w), dtype=np.uint8), 2000))
    img = np.full((h, w), 90, np.uint8)
    img[60:300, 700:1100] = rng.integers(0, 256, (240, 400), dtype=np.uint8)
    out.append(("noise_block", img, 2000))
    img = synth.frame(w, h, seq=3, f=0).copy()
    img[20:200, 30:330] = rng.integers(0, 256, (180, 300), dtype=np.uint8)
    img[150:370, 800:1230] = rng.integers(0, 256, (220, 430), dtype=np.uint8)
    out.append(("two_blocks", img, 2000))
    out.append(("noisy_frame", np.clip(synth.frame(w, h, seq=5, f=0).astype(np.int16) + rng.integers(-8, 9, (h, w)), 0, 255).astype(np.uint8), 2000))
    return out


def test_directed_scenes_reach_more_than_the_suites_images(readings, pattern):
    old = ne.census([(name, ne.read(img, nf, 20, 7, pattern, census_only=True)) for name, img, nf in suite_images()])
    new = _union({name: ne.census(res) for name, (_, _, res) in readings.items()})
    reached_old = {e for e in ne.EDGES if old[e]}
    reached_new = {e for e in ne.EDGES if new[e]}
    print("\nedges the suite's earlier images reach (counted on the CPU by the reading):")
    for e in ne.EDGES:
        print(f"  {e:40s} {'yes' if old[e] else 'no ':3s} {sorted({n for n, _ in old[e]})}")
    assert reached_old < reached_new
