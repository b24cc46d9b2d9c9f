"""GPU suite of the covisibility graph (covis_kernels.hip behind orbfe_covis_count* and orbfe_covis_cull_keyframes*) against the second
reading of tests/np_covis.py, which tests/test_covis_cpu.py ties to the literal one.  Everything is compared byte for byte: headers,
entries (what is not written keeps a canary, and guard records on both sides of every output array must survive) and verdicts.  The
shapes are the directed scenes of np_covis.directed_count_cases / directed_cull_cases -- 0, 1, 63, 64, 65 and 257 slots, points with 1,
64 and 65 observations, weights 14 / 15 / 16, ties below, at and above 15, conn_cap met and exceeded by one and by many, the highest
legal keyframe row, a bad keyframe holding the vote's maximum, refused subjects between good ones, the 0.9 ratio from both sides,
Observations() of 3 and 4, octave + 1 and + 2, the depth gate at its threshold, both sensor kinds, IS_ID0, NOT_ERASE, the three chains
of carry-over, local lists of 0, 1 and 65 rows, keyframes of 65 and 300 slots -- plus seeded maps, a subject and a problem alone and
inside a batch, two runs, and both the host-array and the device forms."""
import numpy as np
import pytest
import torch

from refactored_orb_slam2_amd import _lib, covisibility
from tests import np_covis as M
from tests.test_covis_cpu import canary_entries, cull_refusal_scene

pytestmark = pytest.mark.gpu
GUARD = 3   # canary records on either side of an output array
CANARY = 0x5C


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is None:
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(a.view(np.uint8).reshape(len(a), a.dtype.itemsize).copy()).cuda()


class Resident:
    """a scene in device memory: the map tables, every keyframe's four arrays, and the culling table with their device addresses"""

    def __init__(self, scene):
        self.scene = scene
        p = self.pack = covisibility.pack_covisibility(scene["keyframes"], scene["points"])
        self.obs, self.recs, self.point_bad, self.weighted = _dev(p["obs"]), _dev(p["recs"]), _dev(p["point_bad"]), _dev(p["n_obs_weighted"])
        self.kf_order, self.kf_bad = _dev(p["kf_order"]), _dev(p["kf_bad"])
        n = [len(s) for s in p["slots"]]
        offs = np.cumsum([0] + n)
        cat = lambda parts, dtype: np.concatenate([np.zeros(1, dtype)] + [np.zeros(k, dtype) if a is None else a for a, k in zip(parts, n)])
        self.keys, self.right = _dev(cat(p["keys"], _lib.KP_DTYPE)), _dev(cat(p["u_right"], np.float32))
        self.depth, self.slots = _dev(cat(p["depth"], np.float32)), _dev(cat(p["slots"], np.int32))
        table = p["table"].copy()
        for k in range(len(table)):
            if n[k]:
                at = 1 + int(offs[k])
                table[k]["keys_un"], table[k]["slots"] = self.keys.data_ptr() + 28 * at, self.slots.data_ptr() + 4 * at
                table[k]["u_right"] = 0 if p["u_right"][k] is None else self.right.data_ptr() + 4 * at
                table[k]["depth"] = 0 if p["depth"][k] is None else self.depth.data_ptr() + 4 * at
        self.table = _dev(table)

    def count(self, subjects, cap):
        """(headers, entries) of one device call; every entry starts as a canary, and the guards around both arrays must survive"""
        slots, recs = covisibility.pack_subjects(subjects)
        S = len(recs)
        hbuf = torch.full((S + 2 * GUARD, 32), CANARY, dtype=torch.uint8).cuda()
        ebuf = torch.full((S * cap + 2 * GUARD, 8), CANARY, dtype=torch.uint8).cuda()
        covisibility.covisibility_counts_device(self.obs, self.recs, self.point_bad, self.kf_order, self.kf_bad, _dev(slots), _dev(recs), cap,
                                                hbuf[GUARD:], ebuf[GUARD:])
        torch.cuda.synchronize()
        h, e = hbuf.cpu().numpy(), ebuf.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + S:] == CANARY).all(), "a header outside the array was written"
        assert (e[:GUARD] == CANARY).all() and (e[GUARD + S * cap:] == CANARY).all(), "an entry outside the array was written"
        return (h[GUARD:GUARD + S].copy().view(_lib.COV_HEADER_DTYPE).reshape(S),
                e[GUARD:GUARD + S * cap].copy().view(_lib.COV_ENTRY_DTYPE).reshape(S, cap))

    def cull(self, problems):
        local, recs = covisibility.pack_problems(problems)
        n = len(local)
        buf = torch.full((n + 2 * GUARD, 16), CANARY, dtype=torch.uint8).cuda()
        covisibility.cull_keyframes_device(self.obs, self.recs, self.point_bad, self.weighted, self.table, _dev(np.append(local, 0).astype(np.int32))[:n],
                                           _dev(recs), buf[GUARD:])
        torch.cuda.synchronize()
        v = buf.cpu().numpy()
        assert (v[:GUARD] == CANARY).all() and (v[GUARD + n:] == CANARY).all(), "a verdict outside the array was written"
        return v[GUARD:GUARD + n].copy().view(_lib.COV_VERDICT_DTYPE).reshape(n)


def _want_counts(scene, subjects, cap):
    return M.count_records(scene, subjects, cap, prior=canary_entries(len(subjects), cap))


def _same(got, want, what):
    if got.tobytes() == want.tobytes():
        return True
    g, w = got.reshape(-1), want.reshape(-1)
    for i in range(len(g)):
        if g[i].tobytes() != w[i].tobytes():
            print(what, i, "\n got ", g[i], "\n want", w[i])
            break
    return False


@pytest.fixture(scope="module")
def count_cases():
    return M.directed_count_cases()


@pytest.fixture(scope="module")
def cull_cases():
    return M.directed_cull_cases()


@pytest.fixture(scope="module")
def a_map():
    sc = M.make_map(1)
    return sc, Resident(sc), M.map_subjects(sc)


@pytest.fixture(scope="module")
def a_cull_map():
    sc = M.make_cull_map(2)
    return sc, Resident(sc), M.map_problems(sc, 2, 5)


# ---- counts ------------------------------------------------------------------------------------------------------------------------
def test_directed_counts_device_and_host_forms(count_cases):
    for name, (sc, subjects, cap) in count_cases.items():
        want_h, want_e = _want_counts(sc, subjects, cap)
        R = Resident(sc)
        got_h, got_e = R.count(subjects, cap)
        assert _same(got_h, want_h, name + " header") and _same(got_e, want_e, name + " entry"), name
        got_h, got_e = covisibility.covisibility_counts(R.pack, subjects, cap, entries=canary_entries(len(subjects), cap))
        assert _same(got_h, want_h, name + " host header") and _same(got_e, want_e, name + " host entry"), name


def test_map_counts_both_modes_in_one_batch(a_map):
    sc, R, subjects = a_map
    assert {m for _, _, m in subjects} == {M.CONNECTIONS, M.VOTES}
    for cap in (4, 64):
        want_h, want_e = _want_counts(sc, subjects, cap)
        got_h, got_e = R.count(subjects, cap)
        assert _same(got_h, want_h, "header") and _same(got_e, want_e, "entry"), cap
    assert (want_h["status"] == M.OK).sum() >= 20 and (_want_counts(sc, subjects, 4)[0]["status"] == M.OVERFLOW).sum() >= 20


def test_a_subject_alone_in_a_batch_and_twice(a_map):
    sc, R, subjects = a_map
    batch = (subjects * 2)[:40]
    assert len(batch) == 40
    all_h, all_e = R.count(batch, 16)
    again_h, again_e = R.count(batch, 16)
    assert all_h.tobytes() == again_h.tobytes() and all_e.tobytes() == again_e.tobytes()
    for s in (0, 7, 23, 39):
        h, e = R.count([batch[s]], 16)
        assert h[0].tobytes() == all_h[s].tobytes() and e[0].tobytes() == all_e[s].tobytes(), s


# ---- culling -----------------------------------------------------------------------------------------------------------------------
def test_directed_culling_device_and_host_forms(cull_cases):
    for name, (sc, problems, verdicts) in cull_cases.items():
        want = M.cull_records(sc, problems)
        if verdicts is not None:
            assert [tuple(r)[:3] for r in want.tolist()] == verdicts, name
        R = Resident(sc)
        assert _same(R.cull(problems), want, name), name
        assert _same(covisibility.cull_keyframes(R.pack, problems), want, name + " host"), name


def test_map_culling_alone_and_in_a_batch(a_cull_map):
    sc, R, problems = a_cull_map
    assert len(problems) == 5
    want = M.cull_records(sc, problems)
    got = R.cull(problems)
    assert _same(got, want, "verdict") and got.tobytes() == R.cull(problems).tobytes()
    assert (want["verdict"] == M.CULLED).sum() >= 5
    at = 0
    for local, mono in problems:
        alone = R.cull([(local, mono)])
        assert alone.tobytes() == got[at:at + len(local)].tobytes()
        at += len(local)
    assert _same(covisibility.cull_keyframes(R.pack, problems), want, "host verdict")


def test_refused_rows_between_good_ones():
    sc, problems = cull_refusal_scene()
    want = M.cull_records(sc, problems)
    R = Resident(sc)
    assert _same(R.cull(problems), want, "verdict")
    assert _same(covisibility.cull_keyframes(R.pack, problems), want, "host verdict")
    # a problem whose range lies outside the local array writes nothing
    local, recs = covisibility.pack_problems([([1, 2], False), ([3], False)])
    recs[0]["local_offset"] = 2
    buf = torch.full((3 + 2 * GUARD, 16), CANARY, dtype=torch.uint8).cuda()
    covisibility.cull_keyframes_device(R.obs, R.recs, R.point_bad, R.weighted, R.table, _dev(local), _dev(recs), buf[GUARD:])
    torch.cuda.synchronize()
    v = buf.cpu().numpy()
    assert (v[:GUARD + 2] == CANARY).all() and (v[GUARD + 3:] == CANARY).all()
    assert v[GUARD + 2].tobytes() == M.cull_records(sc, [([3], False)]).tobytes()


def test_the_most_subjects_and_problems_of_one_launch():
    """the device forms at ORBFE_COV_MAX_SUBJECTS and ORBFE_COV_MAX_PROBLEMS: empty subjects and problems, one workgroup each"""
    S = _lib.COV_MAX_SUBJECTS
    subjects = np.zeros(S, _lib.COV_SUBJECT_DTYPE)
    subjects["self"] = -1
    subjects["mode"][1::2] = M.VOTES
    h = torch.full((S + GUARD, 32), CANARY, dtype=torch.uint8).cuda()
    e = torch.full((S + GUARD, 8), CANARY, dtype=torch.uint8).cuda()
    one = torch.zeros(4, dtype=torch.int32).cuda()
    covisibility.covisibility_counts_device(one[:0].view(torch.uint8).reshape(0, 8), one[:0].view(torch.uint8).reshape(0, 16), one[:0], one[:0], one[:0],
                                            one[:0], _dev(subjects), 1, h, e)
    torch.cuda.synchronize()
    got = h.cpu().numpy()
    assert (got[S:] == CANARY).all() and (e.cpu().numpy() == CANARY).all()
    got = got[:S].copy().view(_lib.COV_HEADER_DTYPE).reshape(S)
    assert (got["status"] == M.EMPTY).all() and (got["kf_max"] == -1).all() and (got["n_written"] == 0).all()
    Q = _lib.COV_MAX_PROBLEMS
    problems = np.zeros(Q, _lib.COV_PROBLEM_DTYPE)
    problems["n_local"][Q - 1] = 1
    local = torch.full((1,), 5, dtype=torch.int32).cuda()       # a row outside an empty table
    v = torch.full((1 + GUARD, 16), CANARY, dtype=torch.uint8).cuda()
    covisibility.cull_keyframes_device(one[:0].view(torch.uint8).reshape(0, 8), one[:0].view(torch.uint8).reshape(0, 16), one[:0], one[:0],
                                       one[:0].view(torch.uint8).reshape(0, 48), local, _dev(problems), v)
    torch.cuda.synchronize()
    got = v.cpu().numpy()
    assert (got[1:] == CANARY).all() and got[:1].copy().view(_lib.COV_VERDICT_DTYPE).reshape(-1)[0].tolist() == (0, 0, M.ROW_REFUSED, 0)
