"""ORBextractor::operator() (L/src/ORBextractor.cc) on DIRECTED images: a builder of small scenes that reach every FAST cell and
quadtree edge, the instrumented reading, and the census of what the scenes reach.

  read           np_restatement's fast_score_map / level_cells / fast_candidates / distribute_octree / ic_angle / orb_descriptor in
                 ref_extract's composition, with a record per FAST cell (cell_records: a parallel walk over the cells), per quadtree
                 call (octree_walk: a literal node list) and per level; each walk is asserted equal to the function it walks beside
  build_scenes   per geometry a tuple of scenes: an image composed of named patches on the cell boundaries that level_cells
                 computes and of stamps (isolated pixels: corners whose response the contrast sets), the extractor parameters it is
                 made for, and the edges it is named for
  census         {edge: [(scene, where)]} from the readings' records alone (never from the library's output); EDGES is the table

The recycle verdict of a cell (recycle_verdict) does not imitate the kernel's bookkeeping: at least 385 quick-test survivors on all
eight antipodal ring pairs recycle the 384-entry list for certain, at most 256 - tested height survivors of the four-pair test
cannot; directed cells stay out of the band between (either_band).

Geometries and the fast_cells_kernel instantiation the launcher picks for them (kernel_variant):
  wide    393 x 159   <64, 3>   4 x 12 cells at level 0, runs of four, clipped last column and row, nIni 3 - 4
  tall    247 x 203   <64, 7>   5 x 7 cells, runs of four and three, nIni 1; a cell of 50 rows at level 5
  square  121 x 121   <64, 7>   2 x 2 cells (45 and 38 columns, 51 rows), a square level with nIni 1
  <96, 7> (staged span > 64) cannot be selected by any image: UNREACHABLE, tests/test_extractor_edges_cpu.py

Edge and the scene named for it (any: no scene is named for it; the census finds it in the listed scene and others):

  fast.recycle_keeps_many                dense (square, tall, wide)
  fast.recycle_ini_empty_min_keeps       run_order (tall, wide)
  fast.recycle_both_empty                run_order (tall, wide)
  fast.recycle_min_only                  dense (tall, wide)
  fast.plateau_then_keeps                scores (tall, wide)
  fast.plateau_stays_empty               scores (tall, wide)
  fast.plateau_recycled                  dense (tall, wide)
  fast.both_few                          dense (square, tall, wide)
  fast.both_full                         ramp (square, tall, wide)
  fast.score_eq_ini                      scores (tall, wide)
  fast.score_eq_ini_minus_1              scores (tall, wide)
  fast.score_eq_min                      scores (tall, wide)
  fast.score_eq_min_minus_1              scores (tall, wide)
  fast.extreme_dark_ring                 extremes_20_7, extremes_250_1, extremes_60_20, extremes_7_7, ramp (tall, wide)
  fast.extreme_bright_ring               extremes_20_7, extremes_250_1, extremes_60_20, extremes_7_7, ramp (tall, wide)
  fast.kept_first_row                    scores (tall, wide)
  fast.kept_last_row                     scores (tall, wide)
  fast.kept_first_col                    scores (tall, wide)
  fast.kept_last_col                     scores (tall, wide)
  fast.width_odd                         any: square/borders and 44 more
  fast.width_even                        any: square/borders and 37 more
  fast.first_col_odd                     any: square/borders and 41 more
  fast.first_col_even                    any: square/borders and 42 more
  fast.clipped_last_col                  any: square/borders and 31 more
  fast.clipped_last_row                  any: square/borders and 38 more
  fast.rows_gt_48                        any: square/borders and 23 more
  fast.extreme_th1                       ramp (tall, wide)
  fast.extreme_th7                       extremes_7_7 (tall, wide)
  fast.extreme_th20                      extremes_20_7 (tall, wide)
  fast.extreme_th60                      extremes_60_20 (tall, wide)
  fast.extreme_th250                     extremes_250_1 (tall, wide)
  tree.fewer_than_N                      tree_sparse (square, tall, wide)
  tree.exactly_N                         tree_exact (square, tall, wide)
  tree.more_than_N                       tree_many (square, tall, wide)
  tree.end_size_ge_N                     any: square/dense and 13 more
  tree.phase2                            any: square/dense and 12 more
  tree.phase2_tie_ordered                any: square/dense and 12 more
  tree.phase2_early_stop                 any: square/dense and 10 more
  tree.phase2_stop_in_tie                tree_phase2 (square, tall, wide)
  tree.response_tie_first_left           tree_phase2 (square, tall, wide)
  tree.response_tie_first_right          tree_phase2 (square, tall, wide)
  tree.empty_root_between                tree_phase2 (wide)
  tree.empty_quadrant                    any: square/borders and 37 more
  tree.side1                             tree_cluster (square, tall, wide)
  tree.n_ini_ge_3                        any: wide/borders and 16 more
  tree.n_ini_1                           any: square/borders and 27 more
  fast.equal_pair_across_boundary        scores (tall, wide)
  desc.at_19_left / right / top / bottom borders (square, tall, wide)
  desc.phases_left / phases_right        borders (square, tall, wide)
  level.n_keys_1 / 7 / 8 / 9             tree_single / tree_sparse / tree_eight / tree_exact (square, tall, wide)
  run.recycled_empty_fallback_ordinary   run_order (tall, wide)
  run.mirror                             run_order (wide)
  level.empty_between                    level_gap (square, tall, wide)
  variant.span<=64,rows<=48              any: every scene of wide
  variant.span<=64,rows>48               any: every scene of tall and square

Scenes keep iniThFAST >= minThFAST: fast_candidates is the single-pass form, which states the reference's two calls only in that
order of the thresholds (tests/test_extractor_gpu.py runs the inverted order on other images, against the oracle).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import np_restatement as nr

_f32 = np.float32
N_LEVELS, SCALE = 8, 1.2
LIST_CAP, LIST_RECYCLE = 384, 256          # fast_cells_kernel: the survivor list holds 384, emptied when more than 256 are waiting
FG_MAX, FG_MAX_WIDTH = 4, 176              # csrc/orbfe_internal.h: cells per run, pixels a run may span


# ---- geometry: levels, cells, kernel variant, runs of cells ------------------------------------------------------------------------
def level_sizes(w, h, nlevels=N_LEVELS, scale=SCALE):
    _, inv, _ = nr.extractor_tables(100, scale, nlevels)
    return [(int(np.rint(np.float64(_f32(w) * inv[l]))), int(np.rint(np.float64(_f32(h) * inv[l])))) for l in range(nlevels)]


def n_ini(lw, lh):
    """root nodes of DistributeOctTree (L/src/ORBextractor.cc:535) for a level of lw x lh pixels"""
    return int(np.floor(_f32(lw - 32) / _f32(lh - 32) + _f32(0.5)))


def cell_runs(n_row, wcell):
    """the plan's rule (csrc/extractor.cpp): a cell row of n_row cells is cut into runs of at most G = min(4, 170 / wCell) cells of
    near-equal length.  Returns the list of (first, count)."""
    G = max(1, min(FG_MAX, (FG_MAX_WIDTH - 6) // wcell))
    n_grp = (n_row + G - 1) // G
    runs, done = [], 0
    for k in range(n_grp):
        cnt = (n_row - done + (n_grp - k) - 1) // (n_grp - k)
        runs.append((done, cnt)); done += cnt
    return runs


def kernel_variant(w, h, nlevels=N_LEVELS, scale=SCALE):
    """the fast_cells_kernel instantiation the launcher picks (csrc/fast_kernels.hip, orbfe_launch_fast_cells) from the largest cell
    of all levels: staged span (x0 & 15) + 1 + cols and rows.  Returns (name, span, rows)."""
    span = rows = 0
    for lw, lh in level_sizes(w, h, nlevels, scale):
        for (_, _, x0, y0, x1, y1) in nr.level_cells(lw, lh)[0]:
            span = max(span, (x0 & 15) + 1 + (x1 - x0)); rows = max(rows, y1 - y0)
    name = "span<=64,rows<=48" if span <= 64 and rows <= 48 else "span<=64,rows>48" if span <= 64 else "span>64"
    return name, span, rows


# ---- FAST: the quick test, stated once ---------------------------------------------------------------------------------------------
def quick_test(img, th, pairs=8):
    """(dark, bright) maps: pixel v passes as DARK-ring candidate when every one of the antipodal ring pairs (k, k + 8) has a pixel
    darker than v - th, as BRIGHT-ring candidate when every pair has one brighter than v + th.  pairs = 8: all eight pairs (the
    necessary condition of a 9-arc); pairs = 4: the pairs (0, 8), (2, 10), (4, 12), (6, 14) only -- a superset of the former.
    Pixels without a full ring are False."""
    h, w = img.shape
    I = img.astype(np.int64)
    c = I[3:h - 3, 3:w - 3]
    ring = [I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in nr.RING]
    dark = np.ones(c.shape, bool); bright = np.ones(c.shape, bool)
    for k in range(0, 8, 8 // pairs):
        dark &= np.minimum(ring[k], ring[k + 8]) < c - th
        bright &= np.maximum(ring[k], ring[k + 8]) > c + th
    D = np.zeros((h, w), bool); B = np.zeros((h, w), bool)
    D[3:h - 3, 3:w - 3] = dark; B[3:h - 3, 3:w - 3] = bright
    return D, B


def recycle_verdict(survivors8, survivors4, tested_rows):
    """Does a pass over a cell recycle its survivor list?  From counts alone, not from the kernel's bookkeeping: the list holds
    LIST_CAP entries and is emptied only when more than LIST_RECYCLE are waiting, so a pass with at least LIST_CAP + 1 survivors
    recycles whatever quick test between the eight-pair and the four-pair one the kernel runs ("certain"); with at most
    LIST_RECYCLE - tested_rows survivors of the loosest test it cannot (a pair that straddles the right edge of an odd-width
    region adds at most one entry per row: "never").  Everything between is "either"."""
    if survivors8 >= LIST_CAP + 1:
        return "certain"
    if survivors4 <= LIST_RECYCLE - tested_rows:
        return "never"
    return "either"


def _nms(C):
    """strict 3 x 3 maximum inside the region C (zero frame outside), and the plateau map: scored, >= every neighbour, == one"""
    R = np.zeros((C.shape[0] + 2, C.shape[1] + 2), np.int64)
    R[1:-1, 1:-1] = C
    gt = C > 0; ge = C > 0; eq = np.zeros(C.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                nb = R[1 + dy:R.shape[0] - 1 + dy, 1 + dx:R.shape[1] - 1 + dx]
                gt &= C > nb; ge &= C >= nb; eq |= (C == nb) & (C > 0)
    return gt, ge & eq


def cell_records(img, ini_th, min_th, level=0):
    """A parallel walk over the cells of one level: (records, x, y, score).  The candidate lists are built cell by cell from the
    reference's own two calls -- FAST at iniThFAST, FAST at minThFAST only for a cell that came back empty
    (L/src/ORBextractor.cc:773-780) -- and must equal np_restatement.fast_candidates, which the caller asserts."""
    h, w = img.shape
    S = nr.fast_score_map(img)
    cells, (wcell, hcell) = nr.level_cells(w, h)
    q = {(t, p): quick_test(img, t, p) for t in {ini_th, min_th} for p in (8, 4)}
    recs, xs, ys, ss = [], [], [], []
    for (i, j, iniX, iniY, maxX, maxY) in cells:
        x0, x1, y0, y1 = iniX + 3, maxX - 3, iniY + 3, maxY - 3
        r = dict(level=level, row=i, col=j, x0=x0, y0=y0, tw=x1 - x0, th=y1 - y0, first_col_odd=bool(x0 & 1),
                 span=(iniX & 15) + 1 + (maxX - iniX), rows=maxY - iniY, clipped_x=maxX - iniX < wcell + 6, clipped_y=maxY - iniY < hcell + 6)
        if r["tw"] <= 0 or r["th"] <= 0:
            r.update(produced="none", empty_region=True); recs.append(r)
            continue
        Sc = S[y0:y1, x0:x1]
        out = None
        for name, t in (("ini", ini_th), ("min", min_th)):
            C = np.where(Sc >= t, Sc, 0)
            keep, plat = _nms(C)
            d8, b8 = (m[y0:y1, x0:x1] for m in q[(t, 8)]); d4, b4 = (m[y0:y1, x0:x1] for m in q[(t, 4)])
            s8, s4 = int((d8 | b8).sum()), int((d4 | b4).sum())
            yy, xx = np.nonzero(keep)
            r[name] = dict(th=t, survivors=s8, survivors4=s4, both=int((d8 & b8).sum()), both4=int((d4 & b4).sum()),
                           corners=int((C > 0).sum()), kept=int(keep.sum()), plateau=bool(plat.any()),
                           recycle=recycle_verdict(s8, s4, y1 - y0),
                           on_first_row=bool((yy == 0).any()), on_last_row=bool((yy == y1 - y0 - 1).any()),
                           on_first_col=bool((xx == 0).any()), on_last_col=bool((xx == x1 - x0 - 1).any()),
                           at_threshold=bool((C[yy, xx] == t).any()), scores=[int(v) for v in C[yy, xx]],
                           centres=[int(v) for v in img[y0:y1, x0:x1][yy, xx]], max_score=int(Sc.max()))
            if out is None and len(xx):
                out = (name, xx + x0 - 16, yy + y0 - 16, C[yy, xx])
        r["produced"] = out[0] if out else "none"
        r["pass"] = r[r["produced"]] if out else r["min"]          # the record of the pass that ended the cell
        if out:
            xs.append(out[1]); ys.append(out[2]); ss.append(out[3])
        recs.append(r)
    z = np.zeros(0, np.int64)
    cat = lambda a: np.concatenate(a) if a else z
    return recs, cat(xs), cat(ys), cat(ss)


# ---- DistributeOctTree (L/src/ORBextractor.cc:529-731) as a literal walk over a node list, with its facts ----------------------------
class _Node:
    __slots__ = ("x0", "x1", "y0", "y1", "keys", "seq")

    def __init__(self, x0, x1, y0, y1, keys, seq):
        self.x0, self.x1, self.y0, self.y1, self.keys, self.seq = x0, x1, y0, y1, keys, seq


def octree_walk(x, y, score, minX, maxX, minY, maxY, N):
    """-> (selected candidate indices in list order, facts).  Nodes live in a Python list whose head is index 0 (push_front =
    insert(0)); `seq` is the creation number that stands for the node's address in the reference's sort by (size, pointer)."""
    x = [int(v) for v in x]; y = [int(v) for v in y]; score = [int(v) for v in score]
    f = dict(n_ini=0, empty_roots=0, empty_root_between=False, rounds1=0, rounds2=0, end=None, early_stop=False, stop_in_tie=False,
             tie_ordered=False, empty_quadrant=False, side1=False, response_tie=False, response_tie_orders=set(), n_out=0, N=N,
             n_cand=len(x))
    nini = int(np.floor(_f32(maxX - minX) / _f32(maxY - minY) + _f32(0.5)))
    f["n_ini"] = nini
    if nini < 1:
        return np.zeros(0, np.int64), f
    hX = _f32(maxX - minX) / _f32(nini)
    seq = 0
    roots = []
    for i in range(nini):
        roots.append(_Node(int(hX * _f32(i)), int(hX * _f32(i + 1)), 0, maxY - minY, [], seq)); seq += 1
    for k in range(len(x)):
        roots[min(int(_f32(x[k]) / hX), nini - 1)].keys.append(k)
    full = [bool(n.keys) for n in roots]
    f["empty_roots"] = full.count(False)
    f["empty_root_between"] = any(not full[i] and any(full[:i]) and any(full[i + 1:]) for i in range(nini))
    nodes = [n for n in roots if n.keys]

    def divide(n):
        nonlocal seq
        hx, hy = (n.x1 - n.x0 + 1) // 2, (n.y1 - n.y0 + 1) // 2
        mx, my = n.x0 + hx, n.y0 + hy
        boxes = ((n.x0, mx, n.y0, my), (mx, n.x1, n.y0, my), (n.x0, mx, my, n.y1), (mx, n.x1, my, n.y1))
        keys = ([], [], [], [])
        for k in n.keys:
            keys[(1 if x[k] >= mx else 0) + (2 if y[k] >= my else 0)].append(k)
        out = []
        for b, ks in zip(boxes, keys):
            if ks:
                out.append(_Node(*b, ks, seq)); seq += 1
                if b[1] - b[0] == 1 or b[3] - b[2] == 1:
                    f["side1"] = True
            else:
                f["empty_quadrant"] = True
        return out

    def split(n):
        """children to the front, one by one (the last one created ends up at the head), the parent out of the list"""
        for c in divide(n):
            nodes.insert(0, c)
        nodes.remove(n)

    phase = 1
    while True:
        prev = len(nodes)
        todo = [n for n in nodes if len(n.keys) > 1]
        if phase == 1:
            f["rounds1"] += 1
            for n in todo:                                   # list order
                split(n)
        else:
            f["rounds2"] += 1
            todo.sort(key=lambda n: (len(n.keys), n.seq))    # std::sort of (size, pointer) pairs ...
            todo.reverse()                                   # ... walked from the back
            for a, b in zip(todo, todo[1:]):
                if len(a.keys) == len(b.keys):
                    f["tie_ordered"] = True
            for j, n in enumerate(todo):
                split(n)
                if len(nodes) >= N:
                    if j + 1 < len(todo):
                        f["early_stop"] = True
                        if len(todo[j + 1].keys) == len(n.keys):
                            f["stop_in_tie"] = True
                    break
        size = len(nodes)
        if size >= N or size == prev:
            f["end"] = "size>=N" if size >= N else "size==prev"
            break
        if phase == 1 and size + 3 * sum(1 for n in nodes if len(n.keys) > 1) > N:
            phase = 2
    out = []
    for n in nodes:
        best = n.keys[0]
        for k in n.keys[1:]:
            if score[k] > score[best]:
                best = k
        ties = [k for k in n.keys if score[k] == score[best]]
        if len(ties) > 1:
            f["response_tie"] = True
            f["response_tie_orders"].add("first_left" if x[ties[0]] < x[ties[1]] else "first_right" if x[ties[0]] > x[ties[1]] else "same_x")
        out.append(best)
    f["n_out"] = len(out)
    return np.array(out, np.int64), f


# ---- the reading -------------------------------------------------------------------------------------------------------------------
def read(img, nfeatures, ini_th, min_th, pattern, nlevels=N_LEVELS, scale=SCALE, census_only=False):
    """ORBextractor::operator() (np_restatement.ref_extract's composition) with a record per FAST cell, per quadtree call and per
    level.  Returns a dict: levels[l] = dict(size, cand=(x, y, score), sel, kx, ky, ks, n_keys, keys_mod8, cells=[...], tree={...}), keypoints (list of
    (x, y, size, angle, response, octave)), descriptors (n, 32), variant.  census_only: the records alone (large images: the node
    list walks without its cross-check, no angles and descriptors)."""
    f = _f32
    sf, inv, per = nr.extractor_tables(nfeatures, scale, nlevels)
    h0, w0 = img.shape
    sizes = level_sizes(w0, h0, nlevels, scale)
    pyr, levels, kps, descs = [], [], [], []
    for l in range(nlevels):
        w, h = sizes[l]
        im = img.copy() if l == 0 else nr.resize_linear(pyr[l - 1], w, h)
        pyr.append(im)
        x, y, s = nr.fast_candidates(im, ini_th, min_th)
        recs, wx, wy, ws = cell_records(im, ini_th, min_th, l)
        assert np.array_equal(x, wx) and np.array_equal(y, wy) and np.array_equal(s, ws), f"the cell walk disagrees with fast_candidates at level {l}"
        lev = dict(size=(w, h), cand=(x, y, s), cells=recs, N=per[l], pixels=im, blurred=None)
        if len(x) and nr.level_cells(w, h)[0]:
            sel, facts = octree_walk(x, y, s, 16, w - 16, 16, h - 16, per[l])
            if not census_only:
                sel2 = nr.distribute_octree(x, y, s, 16, w - 16, 16, h - 16, per[l])
                assert np.array_equal(sel, sel2), f"the node-list walk disagrees with distribute_octree at level {l}"
        else:
            sel, facts = np.zeros(0, np.int64), None
        lev.update(sel=sel, tree=facts, kx=x[sel] + 16, ky=y[sel] + 16, ks=s[sel], n_keys=len(sel), keys_mod8=len(sel) % 8)
        if len(sel) and not census_only:
            blurred = nr.gaussian_blur7(im)
            lev["blurred"] = blurred
            size = int(f(31) * sf[l])
            for k in sel:
                px, py = int(x[k]) + 16, int(y[k]) + 16
                ang = nr.ic_angle(im, px, py)
                descs.append(nr.orb_descriptor(blurred, px, py, ang, pattern))
                fx, fy = f(px), f(py)
                if l != 0:
                    fx, fy = fx * sf[l], fy * sf[l]
                kps.append((fx, fy, f(size), ang, f(s[k]), l))
        levels.append(lev)
    return dict(levels=levels, keypoints=kps, descriptors=np.stack(descs) if descs else np.zeros((0, 32), np.uint8),
                variant=kernel_variant(w0, h0, nlevels, scale)[0], thresholds=(ini_th, min_th), nfeatures=nfeatures)


# ---- the builder -------------------------------------------------------------------------------------------------------------------
GEOMETRIES = {"wide": (393, 159), "tall": (247, 203), "square": (121, 121)}
GROUND = 100


class Geometry:
    """level-0 cells of a w x h image: cells[(row, col)] = dict(x0, y0, tw, th: the tested region; roi: the rectangle cv::FAST gets)"""

    def __init__(self, name):
        self.name = name
        self.w, self.h = GEOMETRIES[name]
        cells, (self.wcell, self.hcell) = nr.level_cells(self.w, self.h)
        self.cells = {(i, j): dict(x0=a + 3, y0=b + 3, tw=c - a - 6, th=d - b - 6, roi=(a, b, c, d)) for (i, j, a, b, c, d) in cells}
        self.n_rows = max(i for i, _ in self.cells) + 1
        self.n_cols = max(j for _, j in self.cells) + 1
        self.runs = cell_runs(self.n_cols, self.wcell)
        self.variant = kernel_variant(self.w, self.h)[0]


def _xy(w, h):
    return np.meshgrid(np.arange(w), np.arange(h))


PATCHES = {
    # name: f(x, y, rng) -> grey values; x, y are IMAGE coordinates, so one pattern painted over neighbouring cells is seamless
    # (the ground of every scene is flat GROUND)
    "black": lambda x, y, rng: np.zeros(x.shape, np.int64),
    "white": lambda x, y, rng: np.full(x.shape, 255),
    "stripes": lambda x, y, rng: 100 + 60 * (((2 * x + y) % 4) < 2),                   # every pixel passes the quick test, none is a corner
    # the same below threshold 20, with noise of +-2 on it: the cell that recycles at minThFAST only.  (Noise alone does not get
    # there: of uniform noise of +-10 some 6 % of the pixels survive at threshold 7, and 385 of 992 are needed.)
    "soft_stripes": lambda x, y, rng: 100 + 12 * (((2 * x + y) % 4) < 2) + rng.integers(-2, 3, x.shape),
    "checker": lambda x, y, rng: 100 + 60 * (((x // 3) + (y // 3)) % 2),             # corners of one score: strict NMS keeps none
    "noise": lambda x, y, rng: rng.integers(0, 256, x.shape),
    "low_noise": lambda x, y, rng: GROUND + rng.integers(-10, 11, x.shape),            # no survivor at 20, a few dozen at 7
    "ramp": lambda x, y, rng: (2 * (2 * x + y)) & 255,                                 # at threshold 1 every pixel survives in both polarities
}


class Scene:
    """one image, the extractor parameters it is made for and the edges it is named for: expect = [(edge, where)], where =
    ("cell", level, row, col) | ("tree", level) | ("level", level) | ("image",)"""

    def __init__(self, geom, name, nfeatures=300, ini=20, mn=7, ground=GROUND):
        self.g, self.name, self.nfeatures, self.ini, self.mn = geom, name, nfeatures, ini, mn
        self.img = np.full((geom.h, geom.w), ground, np.int64)
        self.rng = np.random.default_rng([geom.w, geom.h, sum(name.encode())])
        self.expect = []

    @property
    def params(self):
        return (self.nfeatures, self.ini, self.mn)

    @property
    def image(self):
        assert self.img.min() >= 0 and self.img.max() <= 255, self.name
        return self.img.astype(np.uint8)

    def want(self, edge, *where):
        assert edge in EDGES, edge
        self.expect.append((edge, where))

    def want_cell(self, edge, row, col):
        self.want(edge, "cell", 0, row, col)

    def fill(self, cells, patch, inner=False):
        """paint `patch` over the union of the cells' ROIs (tested region + 3: what the ring of a tested pixel can reach; the
        neighbours' tested regions take the spill), or with inner=True over the tested region shrunk by 3 (nothing leaves the cell)"""
        m = -3 if inner else 3
        cs = [self.g.cells[c] for c in cells]
        x0 = min(c["x0"] for c in cs) - m; y0 = min(c["y0"] for c in cs) - m
        x1 = max(c["x0"] + c["tw"] for c in cs) + m; y1 = max(c["y0"] + c["th"] for c in cs) + m
        x, y = _xy(self.g.w, self.g.h)
        self.img[y0:y1, x0:x1] = PATCHES[patch](x[y0:y1, x0:x1], y[y0:y1, x0:x1], self.rng)

    def stamp(self, x, y, c, tail=None):
        """an isolated pixel c grey levels above (below) its surroundings: on a flat ground a corner of response |c| - 1 and nothing
        else.  tail = 0 .. 7: a faint 2 x 2 blob (contrast <= minThFAST, so never a corner) six pixels away, which turns the patch
        moments and with them the keypoint's angle."""
        self.img[y, x] += c
        if tail is not None and self.mn >= 2:
            dx, dy = ((6, 0), (5, 5), (0, 6), (-5, 5), (-6, 0), (-5, -5), (0, -6), (5, -5))[tail % 8]
            self.img[y + dy:y + dy + 2, x + dx:x + dx + 2] += min(self.mn, 6) - 1

    def at(self, row, col, fx=0.5, fy=0.5):
        """pixel of the cell's tested region at the given fractions"""
        c = self.g.cells[(row, col)]
        return c["x0"] + int(fx * (c["tw"] - 1)), c["y0"] + int(fy * (c["th"] - 1))

    def spike(self, x, y, c):
        """the same inside a texture: the pixel c grey levels above the brightest pixel of its ring (response c - 1)"""
        self.img[y, x] = max(self.img[y + dy, x + dx] for dx, dy in nr.RING) + c

    def plateau_pairs(self, row, col, value):
        """four pairs of 8-adjacent pixels of one grey value and so of one response, one pair per direction (each of the eight
        comparisons of the strict NMS meets an equal neighbour): none of the eight pixels is kept"""
        c = self.g.cells[(row, col)]
        assert c["tw"] >= 28 and c["th"] >= 28
        for ox, oy, dx, dy in ((4, 4, 1, 0), (23, 4, 0, 1), (4, 23, 1, 1), (24, 23, -1, 1)):
            self.img[c["y0"] + oy, c["x0"] + ox] = value
            self.img[c["y0"] + oy + dy, c["x0"] + ox + dx] = value

    def both_polarity_pixel(self, x, y):
        """centre 128, ring half 0, half 255: every antipodal pair has one darker and one brighter pixel"""
        self.img[y, x] = 128
        for k, (dx, dy) in enumerate(nr.RING):
            self.img[y + dy, x + dx] = 0 if k < 8 else 255


def _clean_cells(g):
    """(row, col) of cells that are unclipped, in rows 0, 2, ... and not in the last column: the directed rows; the rows between
    them take the spill of ROI fills"""
    return [(i, j) for (i, j), c in sorted(g.cells.items()) if i % 2 == 0 and c["tw"] == g.wcell and c["th"] == g.hcell]


def _add_extremes(sc, c_black, c_white):
    """255 on a ground of 0 and 0 on a ground of 255: the ends of the biased 16-bit fields of the quick test; response 254"""
    sc.fill([c_black], "black"); sc.fill([c_white], "white")
    sc.stamp(*sc.at(*c_black), 255); sc.stamp(*sc.at(*c_white), -255)
    sc.want_cell("fast.extreme_dark_ring", *c_black); sc.want_cell("fast.extreme_bright_ring", *c_white)
    sc.want_cell(f"fast.extreme_th{sc.ini}", *c_black)


def _scene_run_order(g):
    """one cell row: recycled | empty | fallback | ordinary, its mirror image, and the same with seamless stripes"""
    sc = Scene(g, "run_order")
    for k, (first, cnt) in enumerate(g.runs[:2]):
        if cnt != 4:
            continue
        mirror = k == 1
        cols = list(range(first, first + 4))
        R, E, F, O = cols[::-1] if mirror else cols
        sc.fill([(0, R)], "stripes", inner=True)
        sc.stamp(*sc.at(0, R, 0.3, 0.4), 95); sc.stamp(*sc.at(0, R, 0.7, 0.6), -100)
        sc.stamp(*sc.at(0, F), 12, tail=1)
        sc.stamp(*sc.at(0, O, 0.3, 0.3), 50, tail=2); sc.stamp(*sc.at(0, O, 0.7, 0.7), -35, tail=5)
        sc.want("run.mirror" if mirror else "run.recycled_empty_fallback_ordinary", "run", 0, 0, first)
        if (2, 0) not in g.cells or g.cells[(2, 0)]["th"] != g.hcell:
            continue
        # row 2: three cells of seamless stripes (spikes of response 59 and 79 | none | a spike of response 11), then a flat cell
        sc.fill([(2, R), (2, E), (2, F)], "stripes")
        sc.spike(*sc.at(2, R, 0.45, 0.35), 60); sc.spike(*sc.at(2, R, 0.55, 0.65), 80)
        sc.plateau_pairs(2, R, 230)                         # ... and plateaus for the NMS on the bitmap
        sc.spike(*sc.at(2, F), 12)
        sc.stamp(*sc.at(2, O, 0.5, 0.5), 50, tail=3)
        sc.want_cell("fast.recycle_both_empty", 2, E)
        sc.want_cell("fast.recycle_ini_empty_min_keeps", 2, F)
    return sc


def _scene_dense(g):
    """full-range noise (recycles, keeps many; a few planted two-polarity pixels), the checkerboard (recycles, a plateau, empty) and
    soft stripes (nothing at 20, everything at 7) with a faint stamp"""
    sc = Scene(g, "dense")
    cc = _clean_cells(g)
    a = cc[0]
    sc.fill([a], "noise")
    for fx, fy in ((0.25, 0.25), (0.7, 0.3), (0.4, 0.75)):
        sc.both_polarity_pixel(*sc.at(*a, fx, fy))
    sc.want_cell("fast.recycle_keeps_many", *a); sc.want_cell("fast.both_few", *a)
    if len(cc) > 4:                                         # (a geometry of 2 x 2 cells has room for the noise alone)
        b, c = cc[2], cc[4]
        sc.fill([b], "checker")
        sc.want_cell("fast.plateau_recycled", *b)
        sc.fill([c], "soft_stripes")
        sc.spike(*sc.at(*c, 0.3, 0.5), 12); sc.spike(*sc.at(*c, 0.7, 0.5), 14)
        sc.want_cell("fast.recycle_min_only", *c)
    if len(cc) > 6:
        sc.fill([cc[6]], "low_noise")                       # pass 0 without a survivor, pass 1 with a short list
    return sc


def _scene_scores(g):
    """otherwise empty cells with one corner of response ini, ini - 1, min, min - 1; a plateau of two equal neighbours with and
    without a faint corner beside it; corners on the first and last tested row and column; an equal pair across a cell boundary"""
    sc = Scene(g, "scores")
    cc = _clean_cells(g)
    ini, mn = sc.ini, sc.mn
    for k, (resp, edge) in enumerate(((ini, "fast.score_eq_ini"), (ini - 1, "fast.score_eq_ini_minus_1"), (mn, "fast.score_eq_min"),
                                      (mn - 1, "fast.score_eq_min_minus_1"))):
        c = cc[k]
        sc.stamp(*sc.at(*c), (resp + 1) * (1 if k % 2 == 0 else -1))
        sc.want_cell(edge, *c)
    p1, p2 = cc[4], cc[5]
    for c in (p1, p2):
        sc.plateau_pairs(*c, GROUND + 40)
    x, y = sc.at(*p1, 0.5, 0.5)
    sc.stamp(x, y, 13, tail=0)
    sc.want_cell("fast.plateau_then_keeps", *p1); sc.want_cell("fast.plateau_stays_empty", *p2)
    # the four corners of a tested region, and an equal pair that straddles the boundary to the next cell
    e = cc[6]
    ce = g.cells[e]
    for (x, y), c in zip(((ce["x0"], ce["y0"]), (ce["x0"] + ce["tw"] - 1, ce["y0"] + ce["th"] - 1)), (45, -55)):
        sc.stamp(x, y, c)
    for edge in ("fast.kept_first_row", "fast.kept_first_col", "fast.kept_last_row", "fast.kept_last_col"):
        sc.want_cell(edge, *e)
    x, y = ce["x0"] + ce["tw"] - 1, ce["y0"] + ce["th"] // 2
    sc.stamp(x, y, 70); sc.stamp(x + 1, y, 70)
    sc.want("fast.equal_pair_across_boundary", "level", 0)
    return sc


def _scene_ramp(g):
    """the slow ramp at thresholds (1, 1): every pixel of the cell survives in both polarities, the list cannot take the second
    entries; 255 on 0 and 0 on 255 at threshold 1"""
    sc = Scene(g, "ramp", 300, 1, 1)
    cc = _clean_cells(g)
    sc.fill([cc[0]], "ramp")
    sc.want_cell("fast.both_full", *cc[0])
    if len(cc) > 4:
        _add_extremes(sc, cc[2], cc[4])
    return sc


def _scene_extremes(g, ini, mn):
    sc = Scene(g, f"extremes_{ini}_{mn}", 300, ini, mn)
    cc = _clean_cells(g)
    _add_extremes(sc, cc[1], cc[3])
    sc.stamp(*sc.at(*cc[-1]), min(ini + 5, 150), tail=4)
    return sc


def _level0_tree_box(g):
    return g.w - 32, g.h - 32, n_ini(g.w, g.h)


def _scene_tree(g, kind):
    """stamps on a flat ground for DistributeOctTree at level 0.  Coordinates below are relative to the level's border (16, 16), as
    the tree sees them."""
    W, H, nini = _level0_tree_box(g)
    hx = W / nini
    put = lambda sc, x, y, c, **kw: sc.stamp(int(x) + 16, int(y) + 16, c, **kw)
    if kind == "sparse":                                    # fewer candidates than N: every leaf down to one key
        sc = Scene(g, "tree_sparse", 300)
        for k in range(7):
            put(sc, 10 + (W - 20) * ((k * 5) % 7) / 7, 8 + (H - 16) * k / 7, 30 + 7 * k, tail=k)
        sc.want("tree.fewer_than_N", "tree", 0); sc.want("level.n_keys_7", "level", 0)
        return sc
    if kind == "exact":                                     # nine separate stamps, N = 9 at level 0
        sc = Scene(g, "tree_exact", 40)
        for k in range(9):
            put(sc, 8 + (W - 16) * (k % 3 + 0.5) / 3, 8 + (H - 16) * (k // 3 + 0.5) / 3 - 4, 40 + 5 * k, tail=k)
        sc.want("tree.exactly_N", "tree", 0); sc.want("level.n_keys_9", "level", 0)
        return sc
    if kind == "phase2":
        # N = 6.  Two root nodes with two pairs each: after round 1 four leaves of two keys, 4 + 3 * 4 > 6: phase 2 sorts four
        # equal counts and stops after the second split.  The pairs are equal in response: the two leaves that stay hold a tie, one
        # with its first candidate on the left, one with it on the right.
        sc = Scene(g, "tree_phase2", 28)
        # (with a single root node: the four pairs in its four quadrants, one more round of phase 1)
        # The leaves created last split first: with several roots the two quadrants of the first root stay, with one root its two
        # upper quadrants.
        # A pair straddles the horizontal midline of its leaf, so its split makes two nodes; its x is the centre of a column of
        # FAST cells, so the upper stamp is the first candidate whether or not a cell row ends between the two.
        half = lambda a, b: a + (b - a + 1) // 2
        col_centres = sorted({c["x0"] + c["tw"] // 2 - 16 for c in g.cells.values() if c["tw"] > 12})
        my = half(0, H)
        xboxes = [(int(_f32(hx) * _f32(r)), int(_f32(hx) * _f32(r + 1))) for r in ((0, nini - 1) if nini > 1 else (0,))]
        leaves = [(x0, half(x0, x1), y0, y1) for x0, x1 in xboxes for y0, y1 in ((0, my), (my, H))] if nini > 1 else \
                 [(x0, x1, y0, y1) for y0, y1 in ((0, my), (my, H)) for x0, x1 in ((0, half(0, W)), (half(0, W), W))]
        for k, (x0, x1, y0, y1) in enumerate(leaves):       # in creation order: the last two split, the first two stay
            left_first = k % 2 == 0
            cx = min((c for c in col_centres if x0 + 4 <= c < x1 - 6), key=lambda c: abs(c - (x0 + x1) / 2))
            ym = half(y0, y1)
            put(sc, cx + (0 if left_first else 2), ym - 5, 60); put(sc, cx + (2 if left_first else 0), ym + 4, 60)
        sc.want("tree.phase2_stop_in_tie", "tree", 0); sc.want("tree.response_tie_first_left", "tree", 0)
        sc.want("tree.response_tie_first_right", "tree", 0)
        if nini >= 3:
            sc.want("tree.empty_root_between", "tree", 0)
        return sc
    if kind == "cluster":
        # pairs 48, 24, 12, 6, 3 and 2 pixels apart: a round that splits no node ends the call (size == prev), so every round
        # needs a pair of its own to separate until the closest pair sits in nodes of side 1
        sc = Scene(g, "tree_cluster", 300)
        for k, d in enumerate((48, 24, 12, 10, 8, 6, 5, 4, 3, 3, 2, 2)):
            x, y = CLUSTER_AT[g.name][0] + (k % 2) * CLUSTER_AT[g.name][2], CLUSTER_AT[g.name][1] + 6 * k
            put(sc, x, y, 40 + 3 * k); put(sc, x + d, y + (4 if d == 3 else 0), 90 - 3 * k)     # (3, 0) is a ring position
        x, y = SIDE1_AT[g.name]                             # found by a search over octree_walk; the census checks it
        put(sc, x, y, 50); put(sc, x + 2, y, 55)
        sc.want("tree.side1", "tree", 0)
        return sc
    if kind == "many":                                     # a 4 x 4 grid of stamps and N = 5: the last round overshoots
        sc = Scene(g, "tree_many", 24)
        for k in range(16):
            put(sc, 6 + (W - 12) * (k % 4 + 0.5) / 4, 6 + (H - 12) * (k // 4 + 0.5) / 4, 30 + 4 * k, tail=k)
        sc.want("tree.more_than_N", "tree", 0)
        return sc
    if kind == "single":
        sc = Scene(g, "tree_single", 300)
        put(sc, W * 0.5, H * 0.5, 80, tail=3)
        sc.want("level.n_keys_1", "level", 0)
        return sc
    if kind == "eight":
        sc = Scene(g, "tree_eight", 300)
        for k in range(8):
            put(sc, 8 + (W - 16) * (k % 4 + 0.5) / 4, 10 + (H - 20) * (k // 4 + 0.5) / 2, (-1) ** k * (40 + 6 * k), tail=k + 1)
        sc.want("level.n_keys_8", "level", 0)
        return sc
    raise KeyError(kind)


def _scene_borders(g):
    """stamps 19 pixels from each image edge, one per value of (x - 15) & 15 near the left and the right edge"""
    sc = Scene(g, "borders", 300)
    step = max(5, min(7, (g.h - 40) // 16))
    for k in range(16):
        y = 19 + step * k
        sc.stamp(19 + k, y, 40 + 3 * k)
        sc.stamp(g.w - 20 - k, y + 2, -(40 + 3 * k))
    sc.stamp(g.w // 2, 19, 66); sc.stamp(g.w // 2 + 9, g.h - 20, -66)
    for e in ("desc.phases_left", "desc.phases_right", "desc.at_19_left", "desc.at_19_right", "desc.at_19_top", "desc.at_19_bottom"):
        sc.want(e, "level", 0)
    return sc


def _scene_gap(g):
    """a level without a single candidate between levels that have some: one stamp at a position where the resize to level 1 spreads
    it evenly over two pixels (a plateau: NMS keeps neither) and the resize to level 2 joins them again.  The positions were
    found by a search over the reading; the census checks them."""
    sc = Scene(g, "level_gap", 300)
    sc.stamp(*GAP_AT[g.name], 80)
    sc.want("level.empty_between", "image")
    return sc


GAP_AT = {"wide": (196, 77), "tall": (113, 98), "square": (51, 57)}
SIDE1_AT = {"wide": (12, 113), "tall": (166, 46), "square": (6, 75)}                 # a pair two pixels apart (tree coordinates)
CLUSTER_AT = {"wide": (40, 20, 150), "tall": (40, 40, 100), "square": (10, 8, 20)}   # first pair (tree coordinates), x step


@functools.lru_cache(maxsize=None)
def build_scenes(name):
    """-> (geometry, tuple of scenes)"""
    g = Geometry(name)
    scenes = []
    if any(cnt == 4 for _, cnt in g.runs):
        scenes.append(_scene_run_order(g))
    scenes += [_scene_dense(g)]
    if len(_clean_cells(g)) >= 7:
        scenes.append(_scene_scores(g))
    scenes.append(_scene_ramp(g))
    if len(_clean_cells(g)) > 4:
        scenes += [_scene_extremes(g, 250, 1), _scene_extremes(g, 60, 20), _scene_extremes(g, 7, 7), _scene_extremes(g, 20, 7)]
    scenes += [_scene_tree(g, k) for k in ("sparse", "exact", "phase2", "cluster", "many", "single", "eight")]
    scenes += [_scene_borders(g), _scene_gap(g)]
    return g, tuple(scenes)


# ---- the census --------------------------------------------------------------------------------------------------------------------
def _certain_overflow(p):
    """the two-polarity survivors of a recycling pass cannot all get a second list entry: the entries are scored in chunks of at most
    LIST_CAP and (but for the last) more than LIST_RECYCLE, a chunk takes second entries only while it stays within LIST_CAP, so a
    chunk with 128 two-polarity entries overflows; the last chunk can hide LIST_RECYCLE of them"""
    chunks = -(-(p["survivors4"] + 64) // (LIST_RECYCLE + 1))
    return p["recycle"] == "certain" and (p["both"] - LIST_RECYCLE) >= (LIST_CAP - LIST_RECYCLE) * max(1, chunks - 1)


def _passes(r):
    """the passes a cell runs: ini always, min when ini kept nothing"""
    return [r["ini"]] + ([r["min"]] if r["ini"]["kept"] == 0 else [])


_CELL_EDGES = {
    "fast.recycle_keeps_many": ("the list is recycled at iniThFAST and NMS on the bitmap keeps at least eight pixels",
                                lambda r: r["ini"]["recycle"] == "certain" and r["ini"]["kept"] >= 8),
    "fast.recycle_ini_empty_min_keeps": ("recycled at iniThFAST, nothing kept; pass 1 keeps some",
                                         lambda r: r["ini"]["recycle"] == "certain" and r["ini"]["kept"] == 0 and r["min"]["kept"] > 0),
    "fast.recycle_both_empty": ("recycled at both thresholds, the cell stays empty",
                                lambda r: r["ini"]["recycle"] == "certain" and r["min"]["recycle"] == "certain" and r["produced"] == "none"),
    "fast.recycle_min_only": ("no recycling at iniThFAST (nothing kept), recycled at minThFAST",
                              lambda r: r["ini"]["recycle"] == "never" and r["ini"]["kept"] == 0 and r["min"]["recycle"] == "certain"),
    "fast.plateau_then_keeps": ("pass 0 scores corners, strict NMS keeps none of them (a plateau); pass 1 keeps some",
                                lambda r: r["ini"]["corners"] > 0 and r["ini"]["plateau"] and r["ini"]["kept"] == 0 and r["min"]["kept"] > 0),
    "fast.plateau_stays_empty": ("a plateau at both thresholds: corners scored, the cell stays empty",
                                 lambda r: r["ini"]["corners"] > 0 and r["min"]["plateau"] and r["produced"] == "none"),
    "fast.plateau_recycled": ("a plateau in a cell whose list is recycled", lambda r: r["ini"]["corners"] > 0 and r["ini"]["plateau"]
                              and r["ini"]["kept"] == 0 and r["ini"]["recycle"] == "certain"),
    "fast.both_few": ("two-polarity survivors in a recycling pass, fewer than 128: they get second list entries",
                      lambda r: any(p["recycle"] == "certain" and p["both"] >= 1 and p["both4"] < LIST_CAP - LIST_RECYCLE for p in _passes(r))),
    "fast.both_full": ("so many two-polarity survivors that the list cannot take their second entries: second network in place",
                       lambda r: any(_certain_overflow(p) for p in _passes(r))),
    "fast.score_eq_ini": ("the only corner of a cell has response iniThFAST exactly",
                          lambda r: r["produced"] == "ini" and r["ini"]["corners"] == 1 and r["ini"]["at_threshold"]),
    "fast.score_eq_ini_minus_1": ("the only corner has response iniThFAST - 1: kept by pass 1",
                                  lambda r: r["produced"] == "min" and r["min"]["corners"] == 1 and r["min"]["scores"] == [r["ini"]["th"] - 1]),
    "fast.score_eq_min": ("the only corner has response minThFAST exactly",
                          lambda r: r["produced"] == "min" and r["min"]["corners"] == 1 and r["min"]["at_threshold"]),
    "fast.score_eq_min_minus_1": ("the best response of a cell is minThFAST - 1: empty",
                                  lambda r: r["produced"] == "none" and r["min"]["max_score"] == r["min"]["th"] - 1),
    "fast.extreme_dark_ring": ("255 on a ring of 0 (response 254)", lambda r: r["produced"] != "none"
                               and any(s == 254 and c == 255 for s, c in zip(r["pass"]["scores"], r["pass"]["centres"]))),
    "fast.extreme_bright_ring": ("0 on a ring of 255 (response 254)", lambda r: r["produced"] != "none"
                                 and any(s == 254 and c == 0 for s, c in zip(r["pass"]["scores"], r["pass"]["centres"]))),
    "fast.kept_first_row": ("a kept pixel on the first tested row", lambda r: r["produced"] != "none" and r["pass"]["on_first_row"]),
    "fast.kept_last_row": ("a kept pixel on the last tested row", lambda r: r["produced"] != "none" and r["pass"]["on_last_row"]),
    "fast.kept_first_col": ("a kept pixel on the first tested column", lambda r: r["produced"] != "none" and r["pass"]["on_first_col"]),
    "fast.kept_last_col": ("a kept pixel on the last tested column", lambda r: r["produced"] != "none" and r["pass"]["on_last_col"]),
    "fast.width_odd": ("a cell of odd tested width produces keypoints", lambda r: r["produced"] != "none" and r["tw"] % 2 == 1),
    "fast.width_even": ("a cell of even tested width produces keypoints", lambda r: r["produced"] != "none" and r["tw"] % 2 == 0),
    "fast.first_col_odd": ("... whose first tested column is odd", lambda r: r["produced"] != "none" and r["first_col_odd"]),
    "fast.first_col_even": ("... whose first tested column is even", lambda r: r["produced"] != "none" and not r["first_col_odd"]),
    "fast.clipped_last_col": ("a cell of the clipped last column produces keypoints", lambda r: r["produced"] != "none" and r["clipped_x"]),
    "fast.clipped_last_row": ("a cell of the clipped last row produces keypoints", lambda r: r["produced"] != "none" and r["clipped_y"]),
    "fast.rows_gt_48": ("a cell of more than 48 staged rows produces keypoints", lambda r: r["produced"] != "none" and r["rows"] > 48),
}
for _t in (1, 7, 20, 60, 250):
    _CELL_EDGES[f"fast.extreme_th{_t}"] = (f"a response of 254 kept at threshold {_t}", (lambda t: lambda r: r["produced"] != "none"
                                           and r["pass"]["th"] == t and 254 in r["pass"]["scores"])(_t))

_TREE_EDGES = {
    "tree.fewer_than_N": ("fewer candidates than N: every leaf down to one key, ended by size == prev",
                          lambda f: f["n_cand"] < f["N"] and f["end"] == "size==prev" and f["n_out"] == f["n_cand"] and f["n_cand"] > 1),
    "tree.exactly_N": ("exactly N leaves", lambda f: f["n_out"] == f["N"]),
    "tree.more_than_N": ("more than N leaves", lambda f: f["n_out"] > f["N"]),
    "tree.end_size_ge_N": ("ended by size >= N", lambda f: f["end"] == "size>=N"),
    "tree.phase2": ("phase 2 entered", lambda f: f["rounds2"] > 0),
    "tree.phase2_tie_ordered": ("phase 2 orders expandable leaves of equal count by position", lambda f: f["tie_ordered"]),
    "tree.phase2_early_stop": ("phase 2's walk stops before its last expandable leaf", lambda f: f["early_stop"]),
    "tree.phase2_stop_in_tie": ("... in the middle of a group of equal counts", lambda f: f["stop_in_tie"]),
    "tree.response_tie_first_left": ("two candidates of equal response in a final leaf, the first one on the left",
                                     lambda f: "first_left" in f["response_tie_orders"]),
    "tree.response_tie_first_right": ("... the first one on the right", lambda f: "first_right" in f["response_tie_orders"]),
    "tree.empty_root_between": ("an empty root node between full ones", lambda f: f["empty_root_between"]),
    "tree.empty_quadrant": ("a split leaves a quadrant empty", lambda f: f["empty_quadrant"]),
    "tree.side1": ("a split makes a node of width or height 1", lambda f: f["side1"]),
    "tree.n_ini_ge_3": ("three or more root nodes", lambda f: f["n_ini"] >= 3 and f["n_cand"] > 0),
    "tree.n_ini_1": ("one root node", lambda f: f["n_ini"] == 1 and f["n_cand"] > 0),
}

_LEVEL_EDGES = {
    "fast.equal_pair_across_boundary": ("two 8-adjacent candidates of equal response, one on each side of a cell boundary",
                                        lambda L: _adjacent_equal(L["cand"])),
    "desc.at_19_left": ("a keypoint 19 pixels from the left edge", lambda L: (L["kx"] == 19).any()),
    "desc.at_19_right": ("... from the right edge", lambda L: (L["kx"] == L["size"][0] - 20).any()),
    "desc.at_19_top": ("... from the top edge", lambda L: (L["ky"] == 19).any()),
    "desc.at_19_bottom": ("... from the bottom edge", lambda L: (L["ky"] == L["size"][1] - 20).any()),
    "desc.phases_left": ("keypoints with all sixteen values of (x - 15) & 15 within 16 pixels of the innermost left position",
                         lambda L: len({int(v - 15) & 15 for v in L["kx"] if v < 19 + 16}) == 16),
    "desc.phases_right": ("... of the innermost right position",
                          lambda L: len({int(v - 15) & 15 for v in L["kx"] if v > L["size"][0] - 20 - 16}) == 16),
}
for _n in (1, 7, 8, 9):
    _LEVEL_EDGES[f"level.n_keys_{_n}"] = (f"a level with {_n} keypoints ({_n % 8} in the last wave of the describe kernel)",
                                          (lambda n: lambda L: L["n_keys"] == n)(_n))

_RUN_CLASSES = "R: recycled at iniThFAST and not empty; E: empty; F: kept by pass 1; O: kept by pass 0 without recycling"
_OTHER_EDGES = {
    "run.recycled_empty_fallback_ordinary": "a four-cell run that holds, left to right, R E F O (" + _RUN_CLASSES + ")",
    "run.mirror": "a four-cell run that holds O F E R",
    "level.empty_between": "a level without a candidate between levels that have some",
    "variant.span<=64,rows<=48": "fast_cells_kernel<64, 3>: every cell stages at most 64 bytes a row and 48 rows",
    "variant.span<=64,rows>48": "fast_cells_kernel<64, 7>: a cell of more than 48 rows",
}
UNREACHABLE = {"variant.span>64": "fast_cells_kernel<96, 7>: no level width gives a cell with (x0 & 15) + 1 + cols > 64 (see "
                                  "test_no_level_width_reaches_the_96_byte_tile)"}
EDGES = {**{k: v[0] for k, v in _CELL_EDGES.items()}, **{k: v[0] for k, v in _TREE_EDGES.items()},
         **{k: v[0] for k, v in _LEVEL_EDGES.items()}, **_OTHER_EDGES}


def _adjacent_equal(cand):
    x, y, s = cand
    pos = {(int(a), int(b)): int(c) for a, b, c in zip(x, y, s)}
    return any(pos.get((a + dx, b + dy)) == c for (a, b), c in pos.items() for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy)


def _cell_class(r):
    if r["produced"] == "none":
        return "E"
    if r["produced"] == "min":
        return "F"
    return "R" if r["ini"]["recycle"] == "certain" else "O" if r["ini"]["recycle"] == "never" else "?"


def census(results):
    """results: [(scene name, reading)].  -> {edge: sorted list of (scene name, where)}; where = ("cell", level, row, col),
    ("run", level, row, first col), ("tree", level), ("level", level) or ("image",)."""
    out = {e: set() for e in EDGES}
    for name, rd in results:
        out["variant." + rd["variant"]].add((name, ("image",)))
        has = [len(L["cand"][0]) > 0 for L in rd["levels"]]
        if any(not has[l] and any(has[:l]) and any(has[l + 1:]) for l in range(len(has))):
            out["level.empty_between"].add((name, ("image",)))
        for l, L in enumerate(rd["levels"]):
            for r in L["cells"]:
                if "ini" not in r:
                    continue
                for e, (_, pred) in _CELL_EDGES.items():
                    if pred(r):
                        out[e].add((name, ("cell", l, r["row"], r["col"])))
            for e, (_, pred) in _LEVEL_EDGES.items():
                if pred(L):
                    out[e].add((name, ("level", l)))
            if L["tree"] is not None:
                for e, (_, pred) in _TREE_EDGES.items():
                    if pred(L["tree"]):
                        out[e].add((name, ("tree", l)))
            # runs of cells: the plan's rule on this level's cell rows
            w, h = L["size"]
            _, (wcell, _) = nr.level_cells(w, h)
            rows = {}
            for r in L["cells"]:
                rows.setdefault(r["row"], []).append(r)
            for i, rs in rows.items():
                rs.sort(key=lambda r: r["col"])
                for first, cnt in cell_runs(len(rs), wcell):
                    cls = "".join(_cell_class(r) if "ini" in r else "E" for r in rs[first:first + cnt])
                    if cls == "REFO":
                        out["run.recycled_empty_fallback_ordinary"].add((name, ("run", l, i, first)))
                    if cls == "OFER":
                        out["run.mirror"].add((name, ("run", l, i, first)))
    return {e: sorted(v) for e, v in out.items()}


def either_band(results, scenes):
    """directed cells (those a scene names) whose recycle verdict is "either" in a pass they run"""
    bad = []
    for (name, rd), sc in zip(results, scenes):
        cells = {(r["level"], r["row"], r["col"]): r for L in rd["levels"] for r in L["cells"]}
        for edge, where in sc.expect:
            if where[0] == "cell":
                r = cells[where[1:]]
                if any(p["recycle"] == "either" for p in _passes(r)):
                    bad.append((name, where))
    return bad


def first_differing_cell(rd, level, got, want):
    """(level, row, column) and census record of the first FAST cell in which two candidate lists (x, y, score) differ"""
    cells = rd["levels"][level]["cells"]
    key = lambda c: {(int(a), int(b)): int(s) for a, b, s in zip(*c)}
    g, w = key(got), key(want)
    for r in cells:
        inside = lambda p: r["x0"] - 16 <= p[0] < r["x0"] - 16 + r["tw"] and r["y0"] - 16 <= p[1] < r["y0"] - 16 + r["th"]
        if {p: s for p, s in g.items() if inside(p)} != {p: s for p, s in w.items() if inside(p)}:
            return (level, r["row"], r["col"]), {k: v for k, v in r.items() if k != "pass"}
    return (level, None, None), "the lists hold the same candidates in another order"
