"""GPU: orbfe_gba_update_map / orbfe_gba_update_map_device (the map update of LoopClosing::RunGlobalBundleAdjustment,
L/src/LoopClosing.cc:648-703) against the numpy reading of tests/np_gba_map.py -- never against itself.  Every comparison is byte
equality: keyframe records, points and the result record; the two forms equal each other and the reading."""
import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from tests import np_gba as G
from tests import np_gba_map as M

pytestmark = pytest.mark.gpu
PAD = 3
FILL = 0x5A


def _host(s):
    kf, pts, res = optimizer.gba_update_map(s["poses"], s["parent"], s["kf_gba_row"], s["gba_poses"], s["half_baseline"], s["points"],
                                            s["point_gba_row"], s["ref"], s["gba_points"])
    return kf, pts, {f: int(res[f]) for f in M.RESULT_FIELDS}


def _device(s, stride=12, tables=None):
    """The device form on the scene: points as records of `stride` bytes, PAD guard rows around every output.  tables: the two
    adjustment tables as device tensors that are handed in as they lie.  Returns (keyframes, points, result) and whether the inputs
    and the guard rows are what they were."""
    import torch
    n, m = len(s["poses"]), len(s["points"])
    rng = np.random.default_rng(3)
    recs = rng.integers(0, 256, (m, stride), dtype=np.uint8)
    recs[:, :12] = s["points"].view(np.uint8).reshape(m, 12)
    host_in = [s["poses"], s["parent"], s["kf_gba_row"], recs if stride != 12 else s["points"], s["point_gba_row"], s["ref"]]
    up = lambda a: torch.from_numpy(np.array(a)).to("cuda")
    d_in = [up(a) for a in host_in]
    d_G, d_GX = (up(s["gba_poses"]), up(s["gba_points"])) if tables is None else tables
    kf_out = torch.full((n + 2 * PAD, 112), FILL, dtype=torch.uint8, device="cuda")
    pts_out = torch.full((m + 2 * PAD, 3), 777.0, dtype=torch.float32, device="cuda")
    result = torch.full((3, 32), FILL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    optimizer.gba_update_map_device(d_in[0], d_in[1], d_in[2], d_G, float(s["half_baseline"]), d_in[3], d_in[4], d_in[5], d_GX,
                                    kf_out[PAD:PAD + n], pts_out[PAD:PAD + m], result[1], stream=st)
    st.synchronize()
    kf, pts, res = kf_out.cpu().numpy(), pts_out.cpu().numpy(), result.cpu().numpy()
    unmodified = all(d.cpu().numpy().tobytes() == np.asarray(h).tobytes() for d, h in zip(d_in, host_in))
    unmodified = unmodified and d_G.cpu().numpy().tobytes() == s["gba_poses"].tobytes() and d_GX.cpu().numpy().tobytes() == s["gba_points"].tobytes()
    guards = bool((kf[:PAD] == FILL).all() and (kf[PAD + n:] == FILL).all() and (pts[:PAD] == 777.0).all() and (pts[PAD + m:] == 777.0).all()
                  and (res[[0, 2]] == FILL).all())
    rec = np.ascontiguousarray(kf[PAD:PAD + n]).view(M.KEYFRAME_DTYPE).reshape(n)
    r = res[1].view(_lib.GBA_MAP_RESULT_DTYPE)[0]
    return (rec, np.ascontiguousarray(pts[PAD:PAD + m]), {f: int(r[f]) for f in M.RESULT_FIELDS}), unmodified, guards


def _differs(got, want):
    """what differs between two (keyframes, points, result) triples, for the assertion message"""
    out = []
    for f in ("Tcw", "Twc", "Cw", "status"):
        bad = np.flatnonzero((got[0][f].reshape(len(got[0]), -1).view(np.uint32) != want[0][f].reshape(len(want[0]), -1).view(np.uint32)).any(axis=1))
        if len(bad):
            out.append(f"{f}: {len(bad)} keyframes, first {bad[:5].tolist()}")
    bad = np.flatnonzero((got[1].view(np.uint32) != want[1].view(np.uint32)).any(axis=1))
    if len(bad):
        out.append(f"points: {len(bad)}, first {bad[:5].tolist()}")
    if got[2] != want[2]:
        out.append(f"result {got[2]} != {want[2]}")
    return out


@pytest.mark.parametrize("name", sorted(M.SCENES))
def test_both_forms_equal_the_reading(name):
    """one optimised origin; chains of 1 .. 1 025; a fan of 1 025; two origins; the mixed scene; an origin that is not optimised; a
    cycle -- with 0 .. 1 025 points of every kind, as 12-byte and as 32-byte records"""
    s, want = M.scene(name), M.reading(name)
    got = _host(s)
    print(f"{name}: {want[2]}")
    assert not _differs(got, want), ("host form", name)
    for stride in (12, 32):
        dev, unmodified, guards = _device(s, stride)
        assert not _differs(dev, want), ("device form", name, stride)
        assert unmodified and guards, (name, stride)


def test_the_result_record_counts_every_keyframe_and_point():
    s = M.scene("mixed")
    kf, pts, res = _host(s)
    assert res == M.reading("mixed")[2]
    assert res["n_optimised"] + res["n_propagated"] + res["n_unreached"] == len(s["poses"])
    assert res["n_taken"] + res["n_moved"] + res["n_left"] == len(s["points"])
    assert (res["n_optimised"], res["n_propagated"], res["n_unreached"], res["rounds"]) == (10, 21, 6, 5)
    assert [int((kf["status"] == k).sum()) for k in range(3)] == [10, 21, 6]
    stay = (s["point_gba_row"] < 0) & ((s["ref"] < 0) | (kf["status"][np.maximum(s["ref"], 0)] == M.UNREACHED))
    assert pts[stay].tobytes() == s["points"][stay].tobytes() and int(stay.sum()) == res["n_left"]


def test_device_form_rows_out_of_range_are_unreached_or_left_alone():
    """parents, reference keyframes and table rows the host cannot check: never read, the keyframe unreached, the point as it was"""
    s = M.out_of_range_scene()
    want = M.rule(s)
    for stride in (12, 32):
        dev, unmodified, guards = _device(s, stride)
        assert not _differs(dev, want), stride
        assert unmodified and guards
    with pytest.raises(_lib.OrbfeError) as e:
        _host(s)
    assert e.value.code == _lib.ERR_INVALID


def test_the_adjustments_tables_are_read_where_they_lie():
    """orbfe_global_bundle_adjustment_device on plain_65, then its d_poses_out / d_points_out handed to the map update with no copy, with
    eight more keyframes and forty more points the adjustment has not seen"""
    import torch
    g = G.case_scene("plain_65")
    n_kf, n_pt, n_e = len(g["poses"]), len(g["points"]), len(g["edges"])
    cam = optimizer.pose_camera(g["cam"]["fx"], g["cam"]["fy"], g["cam"]["cx"], g["cam"]["cy"], g["cam"]["mbf"], [1.0])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_poses_out = torch.zeros((n_kf, 12), dtype=torch.float32, device="cuda")
    d_points_out = torch.zeros((n_pt, 3), dtype=torch.float32, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(optimizer.gba_workspace_bytes(n_kf, n_pt, n_e), dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    optimizer.global_bundle_adjustment_device(up(cam.view(np.uint8)), up(g["poses"]), up(g["fixed"]), up(g["points"]),
                                              up(g["edges"].view(np.uint8).reshape(-1, 24)), d_poses_out, d_points_out, d_res, ws,
                                              n_iterations=g["n_iterations"], robust=g["robust"], stream=st)
    st.synchronize()
    assert int(d_res.cpu().numpy().view(_lib.BA_RESULT_DTYPE)[0]["rounds"]) != -1   # not refused
    rng = np.random.default_rng(65)
    extra, more = 8, 40
    parent = np.concatenate([np.full(n_kf, -1), [n_kf - 1, n_kf, n_kf + 1, 10, n_kf + 3, n_kf + 3, n_kf + 5, 0]]).astype(np.int32)
    parent[1:n_kf] = np.arange(n_kf - 1)                     # the spanning tree of a sequence: every keyframe under the one before
    s = dict(poses=np.concatenate([g["poses"].reshape(-1, 12), M._poses(rng, extra)]), parent=parent,
             kf_gba_row=np.concatenate([np.arange(n_kf), np.full(extra, -1)]).astype(np.int32),
             gba_poses=d_poses_out.cpu().numpy(), half_baseline=np.float32(g["cam"]["mbf"] / g["cam"]["fx"] / 2),
             points=np.concatenate([g["points"].reshape(-1, 3), rng.uniform(-20, 20, (more, 3)).astype(np.float32)]),
             point_gba_row=np.concatenate([np.arange(n_pt), np.full(more, -1)]).astype(np.int32),
             ref=np.concatenate([rng.integers(0, n_kf, n_pt), rng.integers(0, n_kf + extra, more)]).astype(np.int32),
             gba_points=d_points_out.cpu().numpy())
    assert s["gba_poses"].tobytes() != g["poses"].tobytes()  # the adjustment moved something
    want = M.rule(s)
    dev, unmodified, guards = _device(s, 32, tables=(d_poses_out, d_points_out))
    print(f"behind plain_65: {want[2]}")
    assert not _differs(dev, want)
    assert unmodified and guards
    assert want[2]["n_optimised"] == n_kf and want[2]["n_propagated"] == extra and want[2]["n_taken"] == n_pt and want[2]["n_moved"] == more


def test_the_keyframe_limit_passes_and_one_more_is_refused():
    """ORBFE_GBA_MAP_MAX_KEYFRAMES keyframes: one optimised origin and a fan under it, no deep chain"""
    n = _lib.GBA_MAP_MAX_KEYFRAMES
    parent, optimised = M.fan(n - 1)
    s = M.make_scene(77, parent, optimised, 257)
    want = M.rule(s)
    assert want[2]["n_propagated"] == n - 1 and want[2]["rounds"] == 1
    assert not _differs(_host(s), want)
    dev, unmodified, guards = _device(s, 12)
    assert not _differs(dev, want) and unmodified and guards
    parent, optimised = M.fan(n)
    with pytest.raises(_lib.OrbfeError) as e:
        _host(M.make_scene(78, parent, optimised, 1))
    assert e.value.code == _lib.ERR_INVALID
