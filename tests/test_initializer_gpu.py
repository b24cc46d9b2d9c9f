"""GPU suite of the Initializer (orbfe_initializer_initialize, orbfe_initializer_initialize_batch_device): every case of
tests/np_initializer.py against the yardstick with the criteria of its docstring, the device against the host build of the same
header, the shapes at which the kernels take another path, the selection rule on engineered ties, the order statistic of CheckRT
on engineered good-point counts, degenerate sets and NaN, and the batch form against the host form byte for byte."""
import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, initializer
from tests import initializer_host as IH
from tests import np_initializer as Y

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _run(c, **kw):
    return initializer.initialize(IH.params_of(c["params"]), c["keys1"], c["keys2"], c["matches12"], c["sets"], want_hypotheses=True,
                                  want_words=True, want_candidates=True, **kw)


def _same_as_host(out, host, where):
    """The device and the host build of initializer_internal.h execute the same operations in the same order: the same bytes, except
    that the one libm call (acos, in double) may round a parallax to the neighbouring float"""
    for k in ("hyps_h", "hyps_f", "words_h", "words_f", "P3D", "triangulated_words", "inlier_words"):
        assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint8), np.ascontiguousarray(host[k]).view(np.uint8)), (where, k)
    for f in _lib.INIT_CANDIDATE_DTYPE.names:
        a, b = np.ascontiguousarray(out["candidates"][f]), np.ascontiguousarray(host["candidates"][f])
        if f == "parallax":
            assert (np.abs(a.view(np.int32) - b.view(np.int32)) <= 1).all(), (where, f, a, b)
        else:
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (where, f)
    for f in _lib.INIT_RESULT_DTYPE.names:
        a, b = np.ascontiguousarray(out["result"][f]).reshape(-1), np.ascontiguousarray(host["result"][f]).reshape(-1)
        if f == "parallax":
            assert abs(int(a.view(np.int32)[0]) - int(b.view(np.int32)[0])) <= 1, (where, f, a, b)
        else:
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (where, f, a, b)


@pytest.fixture(scope="module")
def table():
    rows = []
    yield rows
    print("\n| case | quantity | n | e(R32) median | e(R32) max | e(device) median | e(device) max |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.3g} | {r[4]:.3g} | {r[5]:.3g} | {r[6]:.3g} |")


@pytest.mark.parametrize("name", list(Y.CASES))
def test_case_against_the_yardstick(name, table):
    c = Y.solved(name)
    out = _run(c)
    Y.compare(name, out, table)
    Y.assert_followed_to_its_exit(name, out)
    if name == "identical":   # every homography of identical lists is the identity: the exit of :590 whichever hypothesis wins
        assert (int(out["result"]["model"]), int(out["result"]["reason"])) == (1, Y.H_DEGENERATE)
    _same_as_host(out, IH.host_run(c["keys1"], c["keys2"], c["matches12"], c["sets"], IH.params_of(c["params"])), name)
    # the outputs a caller may skip do not change the others
    lean = initializer.initialize(IH.params_of(c["params"]), c["keys1"], c["keys2"], c["matches12"], c["sets"], want_candidates=False)
    assert lean["result"].tobytes() == out["result"].tobytes() and np.array_equal(lean["P3D"], out["P3D"])
    assert np.array_equal(lean["triangulated"], out["triangulated"]) and np.array_equal(lean["inliers"], out["inliers"])


def test_match_counts_around_the_word_and_the_minimum():
    c = dict(Y.solved("general"))
    i1 = np.flatnonzero(c["matches12"] >= 0)
    sets = np.tile(np.arange(8, dtype=np.int32), (3, 1))
    sets[1] = sets[1][::-1]
    c["sets"] = sets
    ref = _run(c)
    n1 = len(c["matches12"])
    for N in (7, 8, 9, 63, 64, 65, 129):
        d = dict(c)
        d["matches12"] = c["matches12"].copy()
        d["matches12"][i1[N:]] = -1
        out = _run(d)
        assert int(out["result"]["n_matches"]) == N
        if N < 8:
            assert (int(out["result"]["model"]), int(out["result"]["reason"])) == (0, Y.FEW_MATCHES)
            assert not out["hyps_h"].view(np.uint8).any() and not out["P3D"].any() and not out["triangulated"].any()
            continue
        for k in ("words_h", "words_f"):   # the first N verdicts of the full run, zero tail bits
            got, want = initializer.bits(out[k], n1), initializer.bits(ref[k], n1)
            assert np.array_equal(got[:, :N], want[:, :N]) and not got[:, N:].any(), (N, k)
        assert np.array_equal(out["hyps_h"]["M"], ref["hyps_h"]["M"]) and np.array_equal(out["hyps_f"]["M"], ref["hyps_f"]["M"])
        _same_as_host(out, IH.host_run(d["keys1"], d["keys2"], d["matches12"], d["sets"], IH.params_of(d["params"])), N)


def test_hypothesis_counts_around_the_workgroup():
    c = dict(Y.solved("general"))
    full = _run(c)
    W = _lib.INIT_WAVES
    for H in (0, 1, W - 1, W, W + 1):   # hypothesis h's record and words do not depend on H
        d = dict(c)
        d["sets"] = c["sets"][:H]
        out = _run(d)
        for k in ("hyps_h", "hyps_f", "words_h", "words_f"):
            assert np.array_equal(out[k], full[k][:H]), (H, k)
        if H == 0:   # nothing scored: SH = SF = 0, where the reference would pass an empty matrix on
            assert (int(out["result"]["model"]), int(out["result"]["reason"]), int(out["result"]["best_h"])) == (0, Y.NO_MODEL, -1)
        else:
            assert int(out["result"]["best_f"]) == Y.first_max(full["hyps_f"]["score"][:H])


@pytest.mark.parametrize("n1", [63, 64, 65])
def test_triangulated_words_around_the_word(n1):
    k1, k2, m12, params, _ = Y.scene(seed=31, kind="general", N=60, n_extra=n1 - 60, noise=0.1)
    assert len(k1) == n1 and len(k2) != n1
    c = {"keys1": k1, "keys2": k2, "matches12": m12, "sets": Y.draw_sets(60, 32, 1), "params": params}
    out = _run(c)
    host = IH.host_run(k1, k2, m12, c["sets"], IH.params_of(params))
    _same_as_host(out, host, n1)
    assert int(out["result"]["success"]) == 1 and int(out["result"]["n_triangulated"]) == int(out["triangulated"].sum()) > 50
    r64 = Y.run(k1, k2, m12, c["sets"], params, "R64")
    assert r64["success"] and np.array_equal(out["triangulated"], r64["triangulated"])
    assert not out["triangulated"][m12 < 0].any() and not out["P3D"][m12 < 0].any()


def _counted_scene(k, extra=24, min_triangulated=50):
    """k noise-free matches of a general scene plus `extra` matches that satisfy the same epipolar geometry exactly but lie beyond the
    point at infinity of their ray: perfect inliers of F that triangulate behind the cameras.  nGood of the true motion is k."""
    rng = np.random.default_rng(100 + k)
    fx, fy, cx, cy = 520.0, 525.0, 320.0, 240.0
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    n = k + extra
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)], 1)
    R, t = Y.look_at(0.05, -0.02), np.array([-0.4, 0.03, 0.05])
    proj = lambda Yc: (Yc @ K.T)[:, :2] / (Yc @ K.T)[:, 2:3]
    a, b = proj(X), proj(X @ R.T + t)
    b_inf = proj(X @ R.T)
    b[k:] = b_inf[k:] - 3.0 * (b[k:] - b_inf[k:])
    m12 = np.arange(n, dtype=np.int32)
    return {"keys1": a.astype(F32), "keys2": b.astype(F32), "matches12": m12, "sets": Y.draw_sets(n, 8, k),
            "params": (fx, fy, cx, cy, 1.0, 1.0, min_triangulated)}


@pytest.mark.parametrize("k,extra,want", [(40, 5, 0), (40, 6, Y.F_FEW_GOOD), (34, 24, Y.F_FEW_GOOD | Y.F_SIMILAR), (35, 24, Y.F_FEW_GOOD)])
def test_acceptance_rules_at_engineered_counts(k, extra, want):
    """The decide kernel on counts engineered through the scene: the true motion sees k points, the motion with -t the `extra` ones,
    N = k + extra inliers, minTriangulated 10.  40 < int(0.9 * 46) = 41 but not < int(0.9 * 45) = 40 (:502, :516); 24 > 0.7 * 34 = 23.8
    but not > 0.7 * 35 = 24.5 (:505-512)."""
    c = _counted_scene(k, extra, min_triangulated=10)
    out = _run(c)
    r64 = Y.run(c["keys1"], c["keys2"], c["matches12"], c["sets"], c["params"], "R64")
    res = out["result"]
    assert int(res["model"]) == 2 == r64["model"] and int(res["n_inliers"]) == k + extra == r64["n_inliers"]
    assert sorted(out["candidates"]["n_good"][:4].tolist()) == sorted(x["n_good"] for x in r64["cands"])
    assert {k, extra} <= set(out["candidates"]["n_good"][:4].tolist()) and int(res["n_good"]) == k
    assert (int(res["reason"]), int(res["success"])) == (want, int(want == 0)) == (r64["reason"], int(r64["success"]))
    assert int(res["second_good_or_n_similar"]) == (2 if want & Y.F_SIMILAR else 1)
    assert int(res["n_triangulated"]) == (k if want == 0 else 0)


@pytest.mark.parametrize("k", [1, 50, 51, 52, 200])
def test_order_statistic_on_engineered_good_counts(k):
    c = _counted_scene(k)
    out = _run(c)
    r64 = Y.run(c["keys1"], c["keys2"], c["matches12"], c["sets"], c["params"], "R64")
    r32 = Y.run(c["keys1"], c["keys2"], c["matches12"], c["sets"], c["params"], "R32")
    assert r64["model"] == 2 == int(out["result"]["model"]) and int(out["result"]["n_inliers"]) == r64["n_inliers"] == k + 24
    got = [{"R": out["candidates"]["R"][j].reshape(3, 3), "t": out["candidates"]["t"][j]} for j in range(4)]
    order, o32 = Y.match_candidates(r64["cands"], got), Y.match_candidates(r64["cands"], r32["cands"])
    goods = [cr["n_good"] for cr in r64["cands"]]
    assert k in goods and 24 in goods   # the true motion sees the k points, the motion with -t the 24 beyond infinity
    cosd = lambda x: np.cos(np.deg2rad(F64(x)))
    for cr, j, j32 in zip(r64["cands"], order, o32):
        assert int(out["candidates"]["n_good"][j]) == cr["n_good"] == r32["cands"][j32]["n_good"]
        e = abs(cosd(out["candidates"]["parallax"][j]) - cosd(cr["parallax"]))
        e32 = abs(cosd(r32["cands"][j32]["parallax"]) - cosd(cr["parallax"]))
        print(f"k = {k}: n_good {cr['n_good']}: parallax {out['candidates']['parallax'][j]:.6f} (R64 {cr['parallax']:.6f}), cosine error "
              f"{e:.3g} (R32 {e32:.3g})")
        assert e <= 4 * e32 + 2 * 2.0 ** -23
    assert (int(out["result"]["success"]), int(out["result"]["reason"])) == (int(r64["success"]), r64["reason"])
    _same_as_host(out, IH.host_run(c["keys1"], c["keys2"], c["matches12"], c["sets"], IH.params_of(c["params"])), k)


def test_selection_is_the_first_maximum_on_engineered_ties():
    c = dict(Y.solved("general"))
    one = c["sets"][7]
    c["sets"] = np.tile(one, (130, 1))                      # 130 equal scores, spread over the 64 lanes of the scan
    out = _run(c)
    assert len(np.unique(out["hyps_f"]["score"])) == 1 and (int(out["result"]["best_h"]), int(out["result"]["best_f"])) == (0, 0)
    c["sets"][:3, 0] = -1                                   # the first three are no draws: score 0, never selected
    c["sets"][70] = Y.solved("general")["sets"][int(Y.solved("general")["r64"]["best_f"])]
    out = _run(c)
    sc = out["hyps_f"]["score"]
    assert (sc[:3] == 0).all() and int(out["result"]["best_h"]) == Y.first_max(out["hyps_h"]["score"])
    assert int(out["result"]["best_f"]) == Y.first_max(sc) and Y.first_max(sc) in (3, 70)
    assert out["result"]["score_f"] == sc.max()


def test_degenerate_sets_and_nan_touch_nothing_else():
    c = dict(Y.solved("general"))
    full = _run(c)
    bad = c["sets"].copy()
    bad[3, 2], bad[5, 7], bad[9, 0], bad[63, 4] = 300, bad[5, 0], -1, 1 << 30
    c["sets"] = bad
    out = _run(c)
    rows, keep = [3, 5, 9, 63], np.setdiff1d(np.arange(64), [3, 5, 9, 63])
    for k in ("hyps_h", "hyps_f", "words_h", "words_f"):
        assert not np.ascontiguousarray(out[k][rows]).view(np.uint8).any() and np.array_equal(out[k][keep], full[k][keep]), k
    # eight collinear, coincident matches: a null space of more than one dimension; whatever comes out, the neighbours are untouched
    d = dict(Y.solved("general"))
    d["keys1"], d["keys2"] = d["keys1"].copy(), d["keys2"].copy()
    i1 = np.flatnonzero(d["matches12"] >= 0)[:8]
    d["keys1"][i1] = d["keys1"][i1[0]]
    d["keys2"][d["matches12"][i1]] = d["keys2"][d["matches12"][i1[0]]]
    sets = d["sets"].copy()
    sets[1] = np.arange(8)
    d["sets"] = sets
    out = _run(d)
    host = IH.host_run(d["keys1"], d["keys2"], d["matches12"], sets, IH.params_of(d["params"]))
    others = np.setdiff1d(np.arange(64), [1])
    for k in ("hyps_h", "hyps_f", "words_h", "words_f"):   # row 1 may hold NaN, whose bits are the machine's; the others are the host's
        assert np.array_equal(np.ascontiguousarray(out[k][others]).view(np.uint8), np.ascontiguousarray(host[k][others]).view(np.uint8)), k
    assert int(out["hyps_h"]["status"][1]) == 1 and int(out["hyps_f"]["status"][1]) == 1
    # a NaN keypoint poisons Normalize, hence every hypothesis: no score is positive, nothing is selected, nothing traps
    e = dict(Y.solved("general"))
    e["keys1"] = e["keys1"].copy()
    e["keys1"][np.flatnonzero(e["matches12"] < 0)[0], 0] = np.nan
    out = _run(e)
    assert (int(out["result"]["model"]), int(out["result"]["reason"]), int(out["result"]["success"])) == (0, Y.NO_MODEL, 0)
    assert not out["P3D"].any() and not out["triangulated"].any() and not out["inliers"].any()
    again = _run(Y.solved("general"))                       # and the next call is what it was
    assert again["result"].tobytes() == full["result"].tobytes()


def test_batch_form_equals_the_host_form():
    import torch
    dev = torch.device("cuda:0")
    a, b = Y.solved("general"), Y.solved("few_points")
    cap, h_cap, P = 360, 64, 3                              # below n2 = 380 of `general`: its second key list is clamped
    probs = [a, None, b]
    W = (cap + 63) // 64
    keys1, keys2 = np.zeros((P, cap, 2), F32), np.zeros((P, cap, 2), F32)
    m12, sets = np.full((P, cap), -1, np.int32), np.zeros((P, h_cap, 8), np.int32)
    n1, n2, H = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    par = np.zeros(P, _lib.INIT_PARAMS_DTYPE)
    hosts = []
    for p, c in enumerate(probs):
        par[p] = IH.params_of(a["params"])[0]
        if c is None:
            hosts.append(initializer.initialize(par[p:p + 1], np.zeros((0, 2), F32), np.zeros((0, 2), F32), np.zeros(0, np.int32),
                                                np.zeros((0, 8), np.int32), want_hypotheses=True, want_words=True))
            continue
        k1, k2, m = c["keys1"][:cap], c["keys2"][:cap], c["matches12"][:cap].copy()
        n1[p], n2[p] = len(c["keys1"]), len(c["keys2"])     # the true counts: the device clamps them to cap
        m_host = m.copy()
        m_host[m_host >= cap] = -1                          # what the clamp means: a match into the cut tail is no match
        N = int((m_host >= 0).sum())
        s = Y.draw_sets(N, 40 + p, 50 + p)
        keys1[p, :len(k1)], keys2[p, :len(k2)], m12[p, :len(m)], sets[p, :len(s)], H[p] = k1, k2, m, s, len(s) + (1000 if p == 2 else 0)
        sets[p, len(s):] = s[0] if p == 2 else 0            # problem 2 announces more sets than h_cap holds: clamped to h_cap
        hosts.append(initializer.initialize(par[p:p + 1], k1, k2, m_host, sets[p, :min(int(H[p]), h_cap)], want_hypotheses=True,
                                            want_words=True))
    assert n2[0] > cap and (m12[0] >= cap).any()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    inputs = [t(par.view(np.uint8).reshape(P, 32)), t(keys1), t(n1), t(keys2), t(n2), t(m12), t(sets), t(H)]

    def launch():
        o = {"result": torch.zeros((P, 224), dtype=torch.uint8, device=dev), "P3D": torch.zeros((P, cap, 3), dtype=torch.float32, device=dev),
             "tri": torch.zeros((P, W), dtype=torch.int64, device=dev), "inl": torch.zeros((P, W), dtype=torch.int64, device=dev),
             "hyps": torch.zeros((P, 2, h_cap, 64), dtype=torch.uint8, device=dev),
             "words": torch.zeros((P, 2, h_cap, W), dtype=torch.int64, device=dev),
             "cands": torch.zeros((P, 8, 64), dtype=torch.uint8, device=dev),
             "ws": torch.zeros(initializer.workspace_bytes(P, cap), dtype=torch.uint8, device=dev)}
        stream = torch.cuda.Stream(device=dev)
        initializer.initialize_batch(inputs[0], inputs[1], inputs[2], inputs[3], inputs[4], inputs[5], inputs[6], inputs[7], o["result"],
                                     o["P3D"], o["tri"], o["inl"], o["hyps"], o["words"], o["cands"], o["ws"], stream=stream)
        stream.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items() if k != "ws"}

    o1, o2 = launch(), launch()
    for k in o1:
        assert o1[k].tobytes() == o2[k].tobytes(), f"two runs differ in {k}"
    for p, h in enumerate(hosts):
        c = probs[p]
        nn1 = 0 if c is None else min(len(c["keys1"]), cap)
        nw, Hp = (nn1 + 63) // 64, len(h["hyps_h"])
        assert o1["result"][p].tobytes() == h["result"].tobytes(), p
        assert np.array_equal(o1["P3D"][p, :nn1], h["P3D"]) and not o1["P3D"][p, nn1:].any()
        assert np.array_equal(o1["tri"][p, :nw].view(np.uint64), h["triangulated_words"]), p
        assert np.array_equal(o1["inl"][p, :nw].view(np.uint64), h["inlier_words"]), p
        assert o1["cands"][p].tobytes() == h["candidates"].tobytes(), p
        if c is None:
            assert int(h["result"]["reason"]) == Y.FEW_MATCHES
            continue
        for m, k in enumerate(("h", "f")):
            assert o1["hyps"][p, m, :Hp].tobytes() == h["hyps_" + k].tobytes(), (p, k)
            assert np.array_equal(o1["words"][p, m, :Hp, :nw].view(np.uint64), h["words_" + k]), (p, k)
    assert int(hosts[0]["result"]["success"]) == 1 and len(hosts[2]["hyps_h"]) == h_cap
