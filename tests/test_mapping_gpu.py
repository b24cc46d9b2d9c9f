"""GPU suite of CreateNewMapPoints (mapping_kernels.hip behind orbfe_triangulate_matches, orbfe_triangulate_matches_batch_device and
orbfe_create_new_map_points) against the numpy yardstick of tests/np_mapping.py: codes, paths and matches equal R32 on every parity
pair; unprojected points, normals and distances within 4 float ulps; linear points no further from the truth (R64) than four times
what the float reading itself is; the shapes where indexing can go wrong; batch form == host form byte for byte; the whole neighbour
loop against a replay of the oracle's search, the reading and the mask update."""
import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, mapping
from tests import np_mapping as M
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in M.CASES:
        s = M.case_scene(name)
        out[name] = (s, M.run(s, "R64"), M.run(s, "R32"))
    return out


@pytest.fixture(scope="module")
def chain_small():
    return M.make_chain_scene(seed=43, n=130)


@pytest.mark.parametrize("name", list(M.CASES))
def test_host_form_against_the_reading(runs, name):
    """(On linear-path points normal / min_distance / max_distance inherit the difference between the two decompositions; the 4-ulp
    bound is asserted on them all the same.)"""
    s, r64, r32 = runs[name]
    got, n_new = mapping.triangulate_matches(*M.scene_args(s))
    assert n_new == int((got["code"] == M.OK).sum())
    M.check_against_yardstick(name, s, r64, r32, got)


def test_host_form_is_deterministic(runs):
    s = runs["mixed"][0]
    a, b = mapping.triangulate_matches(*M.scene_args(s))[0], mapping.triangulate_matches(*M.scene_args(s))[0]
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nA", [0, 1, 63, 64, 65])
def test_row_counts_around_a_wave(runs, nA):
    """The first nA rows of a case give the first nA records of the full run: a record depends on its own row only."""
    s = runs["mixed"][0]
    full = mapping.triangulate_matches(*M.scene_args(s))[0]
    v1, k1, ur1, z1, v2, k2, ur2, z2, mA = M.scene_args(s)
    got, n_new = mapping.triangulate_matches(v1, k1[:nA], ur1[:nA], z1[:nA], v2, k2, ur2, z2, mA[:nA])
    assert len(got) == nA and got.tobytes() == full[:nA].tobytes() and n_new == int((full[:nA]["code"] == M.OK).sum())


def test_no_matches_and_empty_neighbour(runs):
    s = runs["mixed"][0]
    v1, k1, ur1, z1, v2, k2, ur2, z2, mA = M.scene_args(s)
    blank = np.zeros(200, _lib.NEW_POINT_DTYPE)
    blank["idx2"], blank["code"] = -1, M.NO_MATCH
    got, n_new = mapping.triangulate_matches(v1, k1[:200], ur1[:200], z1[:200], v2, k2, ur2, z2, np.full(200, -1, np.int32))
    assert n_new == 0 and got.tobytes() == blank.tobytes()
    got, n_new = mapping.triangulate_matches(v1, k1[:200], ur1[:200], z1[:200], v2, k2[:0], ur2[:0], z2[:0], mA[:200])   # nB == 0
    assert n_new == 0 and got.tobytes() == blank.tobytes()
    got, _ = mapping.triangulate_matches(v1, k1[:200], ur1[:200], z1[:200], v2, k2[:50], ur2[:50], z2[:50], mA[:200])    # matches >= nB
    full = mapping.triangulate_matches(*M.scene_args(s))[0][:200]
    inside = (mA[:200] >= 0) & (mA[:200] < 50)
    assert got[inside].tobytes() == full[inside].tobytes() and got[~inside].tobytes() == blank[~inside].tobytes()
    bad = k1[:200].copy()
    bad["octave"][::3] = 8                                                # outside [0, n_levels): "no match", nothing is read
    got, _ = mapping.triangulate_matches(v1, bad, ur1[:200], z1[:200], v2, k2, ur2, z2, mA[:200])
    assert (got["code"][::3] == M.NO_MATCH).all() and (got["idx2"][::3] == -1).all()
    keep = np.ones(200, bool); keep[::3] = False
    assert got[keep].tobytes() == full[keep].tobytes()


def _batch(scene, order, nA_rows, capA, capB, nB_rows=None):
    """orbfe_triangulate_matches_batch_device for the neighbours `order` of a chain scene; returns (records [K][capA], n_new)"""
    import torch
    A, K = scene["A"], len(order)
    n = len(A["keys"])
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keys1 = np.zeros(capA, _lib.KP_DTYPE); keys1[:n] = A["keys"]
    ur1, z1 = np.full(capA, -1, np.float32), np.full(capA, -1, np.float32)
    ur1[:n], z1[:n] = A["u_right"], A["depth"]
    keys2, ur2, z2 = np.zeros((K, capB), _lib.KP_DTYPE), np.full((K, capB), -1, np.float32), np.full((K, capB), -1, np.float32)
    view2, mA = np.zeros(K, _lib.TRI_VIEW_DTYPE), np.full((K, capA), -1, np.int32)
    for j, k in enumerate(order):
        nb = scene["neighbors"][k]
        keys2[j, :n], ur2[j, :n], z2[j, :n], view2[j] = nb["keys"], nb["u_right"], nb["depth"], nb["view"][0]
        mA[j, :n] = M.true_matches(scene, k)
    out = torch.full((K, capA, 44), 0xAB, dtype=torch.uint8, device=dev)
    n_new = torch.full((K,), -5, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = [up(A["view"].view(np.uint8)), up(keys1.view(np.uint8).reshape(capA, 28)), up(ur1), up(z1), up(np.asarray(nA_rows, np.int32)),
             up(view2.view(np.uint8).reshape(K, 224)), up(keys2.view(np.uint8).reshape(K, capB, 28)), up(ur2), up(z2),
             up(np.full(K, n, np.int32) if nB_rows is None else np.asarray(nB_rows, np.int32)), up(mA)]
        mapping.triangulate_matches_batch(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], out, n_new, s)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(K, capA * 44), n_new.cpu().numpy()


@pytest.mark.parametrize("order,rows", [((0,), (130,)), ((0, 1, 2), (130, 77, 1)), ((2, 0, 1), (1, 130, 77)), ((1, 1, 0), (0, 65, 64))])
def test_batch_form_equals_host_form(chain_small, order, rows):
    """K = 1 and K = 3 with unequal row counts, capA > nA and capB > nB: pair k's rows are the host form's bytes for that neighbour
    whatever its position in the batch, rows at and behind d_nA[k] keep their sentinel bytes, and a second run is byte-identical."""
    sc = chain_small
    A = sc["A"]
    capA, capB = 160, 140
    got, n_new = _batch(sc, order, rows, capA, capB)
    again, n_again = _batch(sc, order, rows, capA, capB)
    assert got.tobytes() == again.tobytes() and np.array_equal(n_new, n_again)
    for j, k in enumerate(order):
        nb, r = sc["neighbors"][k], rows[j]
        want, nn = mapping.triangulate_matches(A["view"], A["keys"][:r], A["u_right"][:r], A["depth"][:r], nb["view"], nb["keys"],
                                               nb["u_right"], nb["depth"], M.true_matches(sc, k)[:r])
        assert got[j, :r * 44].tobytes() == want.tobytes()
        assert (got[j, r * 44:] == 0xAB).all()
        assert n_new[j] == nn
        if r > 60:
            assert nn > 0


def test_batch_form_with_unequal_neighbour_counts(chain_small):
    """d_nB[k] smaller than the rows that are there, zero, and beyond capB (clamped): a match at or behind d_nB[k] comes back as "no
    match", the others as the host form on the neighbour's first d_nB[k] rows gives them."""
    sc = chain_small
    A = sc["A"]
    capA, capB, nBs = 160, 140, (50, 0, 1000)
    got, n_new = _batch(sc, (0, 1, 2), (130, 130, 130), capA, capB, nB_rows=nBs)
    for k, nB in enumerate(nBs):
        nb, nB = sc["neighbors"][k], min(nB, 130)
        mA = M.true_matches(sc, k)
        want, nn = mapping.triangulate_matches(A["view"], A["keys"], A["u_right"], A["depth"], nb["view"], nb["keys"][:nB],
                                               nb["u_right"][:nB], nb["depth"][:nB], mA)
        assert (want["code"][mA >= nB] == M.NO_MATCH).all() and (mA >= nB).sum() == 130 - nB
        assert got[k, :130 * 44].tobytes() == want.tobytes() and n_new[k] == nn
        assert (got[k, 130 * 44:] == 0xAB).all()


def _oracle_search(*a):
    a = list(a)
    a[10] = np.ascontiguousarray(a[10]).astype(ol.EPIPOLAR_DTYPE)
    return ol.search_for_triangulation(*a)


@pytest.mark.parametrize("monocular", [False, True])
def test_neighbour_loop_against_the_replay(monocular):
    """300 keypoints, K = 3: neighbour 2 is gated out (stereo: baseline < mb; monocular: baseline / median depth < 0.01).  The
    device's loop must equal the replay of oracle search -> R32 -> mask update, neighbour after neighbour."""
    sc = M.make_chain_scene(seed=41, n=300, monocular=monocular)
    A, nbs = sc["A"], sc["neighbors"]
    nA, K = 300, 3
    pts, n_matches, n_new, has = mapping.create_new_map_points(A["keys"], A["desc"], A["u_right"], A["depth"], A["has_mp"], A["groups"],
                                                               A["view"], nbs, monocular=monocular, check_orientation=True)
    want, w_matches, w_new, w_has, adopted, searched = M.replay_chain(sc, _oracle_search, device_points=pts)
    print(f"monocular={monocular}: matches {n_matches}, new points {n_new}, adopted {adopted} of {int((w_matches.clip(0)).sum())} pairs")
    assert adopted <= M.NON_PARITY_CAP * nA * K
    assert np.array_equal(n_matches, w_matches) and n_matches[2] == -1 and n_matches[0] > 50 and n_matches[1] > 20
    assert np.array_equal(n_new, w_new) and n_new[0] >= 20 and n_new[1] >= 5 and n_new[2] == 0
    for k in range(K):
        assert np.array_equal(pts[k]["idx2"], searched[k]), k
        for f in ("code", "path", "idx2"):
            assert np.array_equal(pts[k][f], want[k][f]), (k, f)
        nb = nbs[k]                                  # the same kernel on the same matches: the host form's bytes
        alone = mapping.triangulate_matches(A["view"], A["keys"], A["u_right"], A["depth"], nb["view"], nb["keys"], nb["u_right"],
                                            nb["depth"], searched[k])[0]
        assert pts[k].tobytes() == alone.tobytes(), k
    assert (pts[2]["code"] == M.NO_MATCH).all()
    assert np.array_equal(has, w_has) and has.sum() == A["has_mp"].sum() + n_new.sum()
    # a feature that got its map point with neighbour 0 is not searched again, although its descriptor matches in neighbour 1 ...
    _, free = _oracle_search(A["keys"], A["desc"], A["u_right"], A["has_mp"], A["groups"], nbs[1]["keys"], nbs[1]["desc"], nbs[1]["u_right"],
                             nbs[1]["has_mp"], nbs[1]["groups"], nbs[1]["epipolar"], False, True)
    taken = (pts[0]["code"] == M.OK) & (free >= 0)
    assert taken.sum() >= 1 and (pts[1]["idx2"][taken] == -1).all()
    # ... and one that neighbour 0 rejected is
    rejected = pts[0]["code"] >= M.W_ZERO
    assert (pts[1]["idx2"][rejected] >= 0).sum() >= 1
    # the input mask is not touched, a second run is byte-identical
    pts2 = mapping.create_new_map_points(A["keys"], A["desc"], A["u_right"], A["depth"], A["has_mp"], A["groups"], A["view"], nbs,
                                         monocular=monocular, check_orientation=True)[0]
    assert pts2.tobytes() == pts.tobytes()


def test_neighbour_loop_degenerate_shapes():
    sc = M.make_chain_scene(seed=44, n=65)
    A, nbs = sc["A"], sc["neighbors"]
    args = (A["keys"], A["desc"], A["u_right"], A["depth"], A["has_mp"], A["groups"], A["view"])
    pts, nm, nn, has = mapping.create_new_map_points(*args, [])                      # K == 0
    assert pts.shape == (0, 65) and len(nm) == 0 and np.array_equal(has, A["has_mp"])
    empty = dict(nbs[0], keys=nbs[0]["keys"][:0], desc=nbs[0]["desc"][:0], u_right=nbs[0]["u_right"][:0], depth=nbs[0]["depth"][:0],
                 has_mp=nbs[0]["has_mp"][:0], groups={})
    pts, nm, nn, has = mapping.create_new_map_points(*args, [empty, nbs[0]])          # a neighbour with nB == 0 in front
    alone = mapping.create_new_map_points(*args, [nbs[0]])
    assert nm[0] == 0 and nn[0] == 0 and (pts[0]["code"] == M.NO_MATCH).all()
    assert pts[1].tobytes() == alone[0][0].tobytes() and nm[1] == alone[1][0] and np.array_equal(has, alone[3])
    full = np.ones(65, np.uint8)                                                      # every feature already has a map point
    pts, nm, nn, has = mapping.create_new_map_points(A["keys"], A["desc"], A["u_right"], A["depth"], full, A["groups"], A["view"], nbs[:2])
    assert (nm == 0).all() and (nn == 0).all() and (pts["code"] == M.NO_MATCH).all() and has.all()
