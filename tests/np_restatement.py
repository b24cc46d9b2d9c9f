"""Independent numpy restatement of the front-end primitives (TEST INFRASTRUCTURE).

Structurally different from oracle/orb_oracle.c on purpose: vectorised whole-level formulations
instead of literal per-cell / per-node loops.  Used to cross-check the C oracle (the reference has no
golden vectors: SURVEY.md §4, §8(c)) and to validate the data-parallel formulations the HIP kernels use:

  * FAST: one score map per level at minThFAST, NMS restricted to the cell's tested region, two-threshold
    cell rule (SURVEY.md §8(a) row A3 "derived single-pass form").
  * DistributeOctTree: leaves kept as an array in std::list order; one iteration = quadrant counts per
    key, prefix sums, array rebuild (no pointers; ties ordered by list position = creation order).

Reference citations: L/ = Source/Libraries/ORB_SLAM2/.
"""
from __future__ import annotations

import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2),
        (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def cv_round(v):
    return np.rint(v).astype(np.int64)  # numpy rint = round half to even


# ------------------------------------------------------------------------------------------ resize (P2)
def _axis_tables(s, d, clamp_f):
    scale = 1.0 / (float(d) / float(s))
    i = np.arange(d, dtype=np.float64)
    f = ((i + 0.5) * scale - 0.5).astype(np.float32)
    si = np.floor(f).astype(np.int64)
    f = (f - si.astype(np.float32)).astype(np.float32)
    if clamp_f:
        neg = si < 0
        f[neg] = 0; si[neg] = 0
        hi = si >= s - 1
        f[hi] = 0; si[hi] = s - 1
    c0 = np.clip(cv_round((np.float32(1) - f) * np.float32(2048)), -32768, 32767)
    c1 = np.clip(cv_round(f * np.float32(2048)), -32768, 32767)
    return si, c0, c1


def resize_linear(src, dw, dh):
    sh, sw = src.shape
    xo, a0, a1 = _axis_tables(sw, dw, True)
    yo, b0, b1 = _axis_tables(sh, dh, False)
    S = src.astype(np.int64)
    x1 = np.minimum(xo + 1, sw - 1)
    H = S[:, xo] * a0[None, :] + S[:, x1] * a1[None, :]  # (sh, dw)
    y0 = np.clip(yo, 0, sh - 1)
    y1 = np.clip(yo + 1, 0, sh - 1)
    T0 = H[y0] >> 4
    T1 = H[y1] >> 4
    out = (((b0[:, None] * T0) >> 16) + ((b1[:, None] * T1) >> 16) + 2) >> 2
    return out.astype(np.uint8)


# -------------------------------------------------------------------------------------------- blur (P3)
GAUSS_TAPS = np.array([18, 34, 48, 56, 48, 34, 18], dtype=np.int64)


def gaussian_blur7(src):
    p = np.pad(src.astype(np.int64), 3, mode="reflect")  # numpy 'reflect' == BORDER_REFLECT_101
    h, w = src.shape
    hor = sum(GAUSS_TAPS[k] * p[:, k:k + w] for k in range(7))
    ver = sum(GAUSS_TAPS[k] * hor[k:k + h, :] for k in range(7))
    return ((ver + 32768) >> 16).astype(np.uint8)


# -------------------------------------------------------------------------------------------- FAST (P4)
def fast_score_map(img):
    """S(p) = largest t such that p is a FAST-9/16 corner at threshold t (=-1.. if never); computed for
    every pixel that has a full ring.  Border pixels get -1."""
    h, w = img.shape
    I = img.astype(np.int64)
    S = np.full((h, w), -1, dtype=np.int64)
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([c - I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])  # v - ring
    dd = np.concatenate([d, d[:8]], axis=0)
    # min / max over every 9-arc
    amin = np.full(c.shape, -10 ** 6)
    bmin = np.full(c.shape, -10 ** 6)
    for k in range(16):
        arc = dd[k:k + 9]
        amin = np.maximum(amin, arc.min(axis=0))        # dark ring: all v-p > t
        bmin = np.maximum(bmin, (-arc).min(axis=0))     # bright ring: all p-v > t
    S[3:h - 3, 3:w - 3] = np.maximum(amin, bmin) - 1
    return S


def level_cells(w, h):
    """Cell geometry of ComputeKeyPointsOctTree (L/src/ORBextractor.cc:740-771).
    Returns list of (i, j, iniX, iniY, maxX, maxY) for cells that are not skipped, plus (wCell, hCell)."""
    minB = 16
    maxBX, maxBY = w - 16, h - 16
    width, height = np.float32(maxBX - minB), np.float32(maxBY - minB)
    nCols, nRows = int(width / np.float32(30)), int(height / np.float32(30))
    if nCols < 1 or nRows < 1:
        return [], (0, 0)
    wCell = int(np.ceil(width / np.float32(nCols)))
    hCell = int(np.ceil(height / np.float32(nRows)))
    cells = []
    for i in range(nRows):
        iniY = minB + i * hCell
        maxY = iniY + hCell + 6
        if iniY >= maxBY - 3:
            continue
        maxY = min(maxY, maxBY)
        for j in range(nCols):
            iniX = minB + j * wCell
            maxX = iniX + wCell + 6
            if iniX >= maxBX - 6:
                continue
            maxX = min(maxX, maxBX)
            cells.append((i, j, iniX, iniY, maxX, maxY))
    return cells, (wCell, hCell)


def fast_candidates(img, ini_th=20, min_th=7):
    """Single-pass form: score map once, per-cell NMS region, two-threshold rule.
    Returns (x, y, score) relative to (16,16) in the reference's vToDistributeKeys order."""
    h, w = img.shape
    S = fast_score_map(img)
    S = np.where(S >= min_th, S, 0)
    cells, (wCell, hCell) = level_cells(w, h)
    xs, ys, ss = [], [], []
    for (i, j, iniX, iniY, maxX, maxY) in cells:
        x0, x1, y0, y1 = iniX + 3, maxX - 3, iniY + 3, maxY - 3  # tested region [x0,x1) x [y0,y1)
        if x1 <= x0 or y1 <= y0:
            continue
        R = np.zeros((y1 - y0 + 2, x1 - x0 + 2), dtype=np.int64)
        R[1:-1, 1:-1] = S[y0:y1, x0:x1]
        C = R[1:-1, 1:-1]
        keep = C > 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    keep &= C > R[1 + dy:R.shape[0] - 1 + dy, 1 + dx:R.shape[1] - 1 + dx]
        hi = keep & (C >= ini_th)
        sel = hi if hi.any() else keep
        yy, xx = np.nonzero(sel)  # row-major
        xs.append(xx + x0 - 16); ys.append(yy + y0 - 16); ss.append(C[yy, xx])
    if not xs:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ss)


# ------------------------------------------------------------------------------------------ octree (A4)
def distribute_octree(x, y, score, minX, maxX, minY, maxY, N):
    """Array formulation of DistributeOctTree (L/src/ORBextractor.cc:529-731).  Leaves are kept in an
    array in list order (index 0 = list head).  Returns selected candidate indices in list order."""
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64); score = np.asarray(score, np.int64)
    n = len(x)
    nIni = int(np.floor(np.float32(maxX - minX) / np.float32(maxY - minY) + np.float32(0.5)))  # std::round, positive
    if nIni < 1:
        return np.zeros(0, np.int64)
    hX = np.float32(maxX - minX) / np.float32(nIni)
    # leaves: bbox arrays + per-key node id (position in the leaf array)
    ini = np.arange(nIni)
    bx0 = (hX * ini.astype(np.float32)).astype(np.int64)
    bx1 = (hX * (ini + 1).astype(np.float32)).astype(np.int64)
    by0 = np.zeros(nIni, np.int64)
    by1 = np.full(nIni, maxY - minY, np.int64)
    node = np.minimum((x.astype(np.float32) / hX).astype(np.int64), nIni - 1) if n else np.zeros(0, np.int64)
    cnt = np.bincount(node, minlength=nIni)
    keepm = cnt > 0  # erase empty ini nodes, order preserved
    remap = np.cumsum(keepm) - 1
    bx0, bx1, by0, by1, cnt = bx0[keepm], bx1[keepm], by0[keepm], by1[keepm], cnt[keepm]
    node = remap[node]

    def quadrants():
        halfX = (bx1 - bx0 + 1) // 2  # ceil(w/2) for w >= 0
        halfY = (by1 - by0 + 1) // 2
        mx, my = bx0 + halfX, by0 + halfY
        q = (x >= mx[node]).astype(np.int64) + 2 * (y >= my[node]).astype(np.int64)  # 0:n1 1:n2 2:n3 3:n4
        c4 = np.zeros((len(bx0), 4), np.int64)
        np.add.at(c4, (node, q), 1)
        return q, c4, mx, my

    def rebuild(split_order, q, c4, mx, my):
        """split_order: leaf positions to split, in processing (= child creation) order."""
        nonlocal bx0, bx1, by0, by1, cnt, node
        L = len(bx0)
        is_split = np.zeros(L, bool); is_split[split_order] = True
        # children in creation order
        cb = []
        child_of = {}
        for p in split_order:
            for qq in range(4):
                if c4[p, qq] > 0:
                    x0 = bx0[p] if qq in (0, 2) else mx[p]
                    x1 = mx[p] if qq in (0, 2) else bx1[p]
                    y0 = by0[p] if qq in (0, 1) else my[p]
                    y1 = my[p] if qq in (0, 1) else by1[p]
                    child_of[(p, qq)] = len(cb)
                    cb.append((x0, x1, y0, y1, c4[p, qq]))
        K = len(cb)
        stay = np.nonzero(~is_split)[0]
        newpos_stay = np.full(L, -1, np.int64)
        newpos_stay[stay] = K + np.arange(len(stay))
        nb = np.zeros((K + len(stay), 5), np.int64)
        for j, rec in enumerate(cb):
            nb[K - 1 - j] = rec
        nb[K:, 0] = bx0[stay]; nb[K:, 1] = bx1[stay]; nb[K:, 2] = by0[stay]; nb[K:, 3] = by1[stay]; nb[K:, 4] = cnt[stay]
        newnode = np.empty_like(node)
        for k in range(len(node)):
            p = node[k]
            newnode[k] = K - 1 - child_of[(p, q[k])] if is_split[p] else newpos_stay[p]
        bx0, bx1, by0, by1, cnt = nb[:, 0].copy(), nb[:, 1].copy(), nb[:, 2].copy(), nb[:, 3].copy(), nb[:, 4].copy()
        node = newnode

    finish = False
    while not finish:
        prev = len(bx0)
        q, c4, mx, my = quadrants()
        expandable = np.nonzero(cnt > 1)[0]
        rebuild(list(expandable), q, c4, mx, my)  # phase 1: list order
        size = len(bx0)
        nToExpand = int((cnt > 1).sum())
        if size >= N or size == prev:
            finish = True
        elif size + 3 * nToExpand > N:
            while not finish:
                prev = len(bx0)
                q, c4, mx, my = quadrants()
                E = np.nonzero(cnt > 1)[0]
                # sort (size asc, "pointer" asc) then walk from the back: size desc, later-created first.
                # later created == smaller list position.
                order = sorted(E, key=lambda p: (-cnt[p], p))
                chosen = []
                sz = prev
                for p in order:
                    chosen.append(p)
                    sz += int((c4[p] > 0).sum()) - 1
                    if sz >= N:
                        break
                rebuild(chosen, q, c4, mx, my)
                size = len(bx0)
                if size >= N or size == prev:
                    finish = True
    # best key per leaf: max response, first (lowest candidate index) wins ties
    out = np.full(len(bx0), -1, np.int64)
    best = np.full(len(bx0), -1, np.int64)
    for k in range(n):
        p = node[k]
        if score[k] > best[p]:
            best[p] = score[k]; out[p] = k
    return out


# --------------------------------------------------------------------------------- orientation (A6, P5)
def umax_table():
    hp = 15
    vmax = int(np.floor(hp * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(hp * np.sqrt(2.0) / 2))
    um = [0] * (hp + 1)
    for v in range(vmax + 1):
        um[v] = int(np.rint(np.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while um[v0] == um[v0 + 1]:
            v0 += 1
        um[v] = v0
        v0 += 1
    return um


def fast_atan2(y, x):
    f = np.float32
    scale = f(180.0 / np.pi)
    p1 = f(0.9997878412794807) * scale
    p3 = f(-0.3258083974640975) * scale
    p5 = f(0.1555786518463281) * scale
    p7 = f(-0.04432655554792128) * scale
    y = f(y); x = f(x)
    ax, ay = abs(x), abs(y)
    eps = f(2.220446049250313e-16)
    if ax >= ay:
        c = ay / (ax + eps); c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    else:
        c = ax / (ay + eps); c2 = c * c
        a = f(90.0) - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    if x < 0:
        a = f(180.0) - a
    if y < 0:
        a = f(360.0) - a
    return f(a)


def ic_angle(img, x, y):
    um = umax_table()
    I = img.astype(np.int64)
    m10 = m01 = 0
    for v in range(-15, 16):
        d = um[abs(v)]
        row = I[y + v, x - d:x + d + 1]
        u = np.arange(-d, d + 1)
        m10 += int((u * row).sum())
        m01 += v * int(row.sum())
    return fast_atan2(m01, m10)


# ------------------------------------------------------------------------------------- descriptor (A8)
def orb_descriptor(blurred, x, y, angle_deg, pattern):
    f = np.float32
    ang = f(angle_deg) * f(np.pi / f(180.0))
    a = f(np.cos(np.float64(ang)))  # correctly rounded float cos/sin (== glibc cosf on all tested inputs)
    b = f(np.sin(np.float64(ang)))
    pat = np.asarray(pattern, np.int64).reshape(512, 2)
    px = pat[:, 0].astype(np.float32); py = pat[:, 1].astype(np.float32)
    yy = cv_round((px * b).astype(np.float32) + (py * a).astype(np.float32))
    xx = cv_round((px * a).astype(np.float32) - (py * b).astype(np.float32))
    vals = blurred[y + yy, x + xx].astype(np.int64)
    bits = (vals[0::2] < vals[1::2]).astype(np.uint8)
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


# ------------------------------------------------------------------------------ whole extraction (A1-A9)
def extractor_tables(nfeatures, scale_factor, nlevels):
    """ORBextractor::ORBextractor (L/src/ORBextractor.cc:408-441): mvScaleFactor (float x the double member scaleFactor,
    L/include/ORBextractor.h:91), mvInvScaleFactor, mnFeaturesPerLevel (float arithmetic, cvRound)."""
    f = np.float32
    sf = [f(1.0)]
    for i in range(1, nlevels):
        sf.append(f(np.float64(sf[i - 1]) * np.float64(f(scale_factor))))
    inv = [f(1.0) / v for v in sf]
    factor = f(1.0) / f(scale_factor)
    nd = f(nfeatures) * (f(1) - factor) / (f(1) - f(np.float64(factor) ** np.float64(nlevels)))
    per, tot = [], 0
    for _ in range(nlevels - 1):
        per.append(int(np.rint(np.float64(nd))))
        tot += per[-1]
        nd = nd * factor
    per.append(max(nfeatures - tot, 0))
    return sf, inv, per


def ref_extract(img, nfeatures, scale_factor, nlevels, ini_th, min_th, pattern):
    """ORBextractor::operator() (L/src/ORBextractor.cc:983-1038) composed from the primitives above: ComputePyramid (:1040-1066, each
    level resized from the previous one), ComputeKeyPointsOctTree (:733-813), computeOrientation, blur + descriptors per level,
    coordinates scaled by mvScaleFactor[level].  Returns (list of (x, y, size, angle, response, octave), descriptors (n, 32))."""
    f = np.float32
    sf, inv, per = extractor_tables(nfeatures, scale_factor, nlevels)
    h0, w0 = img.shape
    pyr = []
    for l in range(nlevels):
        w = int(np.rint(np.float64(f(w0) * inv[l]))); h = int(np.rint(np.float64(f(h0) * inv[l])))
        pyr.append(img.copy() if l == 0 else resize_linear(pyr[l - 1], w, h))
    kps, descs = [], []
    for l in range(nlevels):
        im = pyr[l]
        h, w = im.shape
        x, y, s = fast_candidates(im, ini_th, min_th)
        if len(x) == 0:
            continue
        sel = distribute_octree(x, y, s, 16, w - 16, 16, h - 16, per[l])
        if len(sel) == 0:
            continue
        size = int(f(31) * sf[l])
        blurred = gaussian_blur7(im)
        for k in sel:
            px, py = int(x[k]) + 16, int(y[k]) + 16
            ang = ic_angle(im, px, py)
            descs.append(orb_descriptor(blurred, px, py, ang, pattern))
            fx, fy = f(px), f(py)
            if l != 0:
                fx, fy = fx * sf[l], fy * sf[l]
            kps.append((fx, fy, f(size), ang, f(s[k]), l))
    return kps, (np.stack(descs) if descs else np.zeros((0, 32), np.uint8))


# ============================================================================================ matchers (second reading)
# An INDEPENDENT restatement of the order-dependent matcher loops, written from the reference sources alone
# (L/src/ORBmatcher.cc:45-128, 161-273, 388-492, 1247-1383, 1506-1556 and L/src/Frame.cc:250-263, 341-410) as plain Python
# loops over lists -- structurally unlike oracle/orb_oracle.c (per-cell Python lists instead of a CSR grid, dict FeatureVectors,
# no query records inside the loops).  tests/test_oracle_cpu.py asserts that the C oracle agrees with it on real-image pairs and
# on a ties-heavy synthetic case; a misread quirk would have to be made twice, in two languages, to go unnoticed.
import math
import operator

FRAME_GRID_ROWS, FRAME_GRID_COLS = 48, 64      # L/include/Frame.h:36-37
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30    # L/src/ORBmatcher.cc:36-38
_f32 = np.float32
_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def c_round(x):
    """C round(): halves away from zero."""
    x = float(x)
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (:1542-1556): bit count of the XOR of 8 x 32 bits."""
    return int(_POPCOUNT[np.bitwise_xor(a, b)].sum())


class RefFrame:
    """The members of Frame the matcher reads, with AssignFeaturesToGrid (Frame.cc:250-263), PosInGrid (:399-410) and
    GetFeaturesInArea (:341-397)."""

    def __init__(self, keys, desc, min_x, max_x, min_y, max_y, u_right=None):
        self.N = len(keys)
        self.x = [_f32(v) for v in keys["x"]]; self.y = [_f32(v) for v in keys["y"]]
        self.octave = [int(v) for v in keys["octave"]]; self.angle = [_f32(v) for v in keys["angle"]]
        self.desc = np.asarray(desc, np.uint8)
        self.u_right = None if u_right is None else [_f32(v) for v in u_right]
        self.mnMinX, self.mnMaxX, self.mnMinY, self.mnMaxY = _f32(min_x), _f32(max_x), _f32(min_y), _f32(max_y)
        self.mfGridElementWidthInv = _f32(FRAME_GRID_COLS) / (self.mnMaxX - self.mnMinX)     # Frame.cc:107-110
        self.mfGridElementHeightInv = _f32(FRAME_GRID_ROWS) / (self.mnMaxY - self.mnMinY)
        self.mGrid = [[[] for _ in range(FRAME_GRID_ROWS)] for _ in range(FRAME_GRID_COLS)]
        for i in range(self.N):
            posX = c_round((self.x[i] - self.mnMinX) * self.mfGridElementWidthInv)
            posY = c_round((self.y[i] - self.mnMinY) * self.mfGridElementHeightInv)
            if posX < 0 or posX >= FRAME_GRID_COLS or posY < 0 or posY >= FRAME_GRID_ROWS:
                continue
            self.mGrid[posX][posY].append(i)

    def GetFeaturesInArea(self, x, y, r, minLevel=-1, maxLevel=-1, in_box=None, info=None):
        """`in_box(|d|, r)` stands in for the box comparison `|d| < r` (proj_walk's rules).  `info`, a dict, receives what proj_walk
        records on the way: outside (one of the four early returns was taken), ncol (grid columns of the window), raw_pos (per
        returned index its place among ALL entries of the window's cells, the order a wave consumes them in)."""
        x, y, r = _f32(x), _f32(y), _f32(r)
        vIndices = []
        if info is not None:
            info.update(outside=True, ncol=0, raw_pos=[])
        nMinCellX = max(0, int(math.floor((x - self.mnMinX - r) * self.mfGridElementWidthInv)))
        if nMinCellX >= FRAME_GRID_COLS:
            return vIndices
        nMaxCellX = min(FRAME_GRID_COLS - 1, int(math.ceil((x - self.mnMinX + r) * self.mfGridElementWidthInv)))
        if nMaxCellX < 0:
            return vIndices
        nMinCellY = max(0, int(math.floor((y - self.mnMinY - r) * self.mfGridElementHeightInv)))
        if nMinCellY >= FRAME_GRID_ROWS:
            return vIndices
        nMaxCellY = min(FRAME_GRID_ROWS - 1, int(math.ceil((y - self.mnMinY + r) * self.mfGridElementHeightInv)))
        if nMaxCellY < 0:
            return vIndices
        if info is not None:
            info.update(outside=False, ncol=nMaxCellX - nMinCellX + 1)
        bCheckLevels = (minLevel > 0) or (maxLevel >= 0)
        raw = 0
        for ix in range(nMinCellX, nMaxCellX + 1):
            for iy in range(nMinCellY, nMaxCellY + 1):
                for j in self.mGrid[ix][iy]:
                    raw += 1
                    if bCheckLevels:
                        if self.octave[j] < minLevel:
                            continue
                        if maxLevel >= 0 and self.octave[j] > maxLevel:
                            continue
                    distx = self.x[j] - x
                    disty = self.y[j] - y
                    if (abs(distx) < r and abs(disty) < r) if in_box is None else (in_box(abs(distx), r) and in_box(abs(disty), r)):
                        vIndices.append(j)
                        if info is not None:
                            info["raw_pos"].append(raw - 1)
        return vIndices


def compute_three_maxima(sizes, lt=operator.lt, gt1=operator.gt, gt2=operator.gt, gt3=operator.gt, lt3=None):
    """ORBmatcher::ComputeThreeMaxima (:1506-1538) on the bin sizes.  `lt` stands in for the `<` of the 0.1 rule (proj_walk's rules);
    node_walk's rules swap each of the five comparisons on its own: gt1 / gt2 / gt3 the three `s > max`, lt the tenth test of max2,
    lt3 the tenth test of max3 (None: the same as lt)."""
    lt3 = lt if lt3 is None else lt3
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if gt1(s, max1):
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif gt2(s, max2):
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif gt3(s, max3):
            max3 = s
            ind3 = i
    if lt(_f32(max2), _f32(0.1) * _f32(max1)):
        ind2 = ind3 = -1
    elif lt3(_f32(max3), _f32(0.1) * _f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


def _rot_bin(angle_a, angle_b, rnd=c_round):
    rot = _f32(angle_a) - _f32(angle_b)
    if rot < 0.0:
        rot = rot + _f32(360.0)
    b = rnd(rot * (_f32(1.0) / _f32(HISTO_LENGTH)))
    return 0 if b == HISTO_LENGTH else b


# ------------------------------------------------------------------------------------------------------------------------------
# The ordered projection searches, one body: SearchByProjection(Frame&, vector<MapPoint*>&, th) (:45-128, mode 0),
# SearchByProjection(Frame& cur, const Frame& last, th, bMono) from the window search on (:1289-1383, mode 1) and
# SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) from the window search on (:1439-1501: mode 1 without the stereo
# gate, with ORBdist for TH_HIGH and every match blocking).
(PX_SKIPPED, PX_OUTSIDE_GRID, PX_EMPTY_WINDOW, PX_ALL_GONE, PX_TOO_FAR, PX_RATIO, PX_MATCHED, PX_OVERWRITTEN, PX_ROTATION) = range(9)

# The reference's comparisons.  A test swaps exactly one of them to show that the directed scenes tell the two readings apart.
PROJ_RULES = dict(
    best_lt=operator.lt,          # dist < bestDist: the first minimum in enumeration order wins
    second_lt=operator.lt,        # dist < bestDist2: the first of tied second-best candidates gives bestLevel2
    accept=operator.le,           # bestDist <= TH_HIGH
    ratio_reject=operator.gt,     # bestDist > mfNNratio * bestDist2
    same_level=operator.eq,       # bestLevel == bestLevel2
    last_taker_wins=True,         # F.mvpMapPoints[bestIdx] = pMP overwrites
    blocks=bool,                  # only a point with Observations() > 0 keeps later queries off its keypoint
    rot_unblocks=True,            # the rotation check leaves NULL: the slot is free again
    rot_clears_all=True,          # ... through every entry of a removed bin, whoever took the keypoint last
    in_box=operator.lt,           # fabs(distx) < r && fabs(disty) < r
    gate_fail=operator.gt,        # er > radius
    has_right=lambda ur: ur > 0,  # mvuRight[idx] > 0
    maxima_lt=operator.lt,        # max2 < 0.1f * max1
    round=c_round,                # round(): halves away from zero
)


def proj_walk(F, queries, mode, nnratio, check_orientation, has_observed_point, th_high=TH_HIGH, stereo_gate=True, rules=None):
    """The reference read literally, one query after the other.  queries[i] is indexable by the fields of the library's query record
    (u, v, u_r, radius, min_level, max_level, valid, blocks, angle, desc); min_level / max_level go to GetFeaturesInArea as they are.
    Returns (nmatches, assigned, blocked, exits, facts): assigned[idx] the query F.mvpMapPoints[idx] was written by (-1: none, or NULL
    again), blocked[idx] whether the slot holds a point with Observations() > 0 after the call, exits one PX_* code per query, facts
    what the walk saw.  Facts are counted on the indices that pass level, box AND stereo gate -- the list proj_candidates_kernel
    writes -- so a keypoint that is blocked and fails the gate counts as gated.
    per query: n_window, n_blocked_before, n_blocked_by_call, depth (0 without a by-call skip, else 1 + the largest depth among the
    queries whose matches were skipped), dep_min (the earliest of those queries, -1), best_idx, best_dist, second_dist (256: none),
    best_ties, best_tie_out_of_index_order, second_level_tied, matters_kept (not blocked before the call and d <= th_high, or in
    mode 0 nnratio * d < th_high), ncol, best_pos / second_pos (place of the two among all entries of the window's cells),
    first_choice / first_accept (what the query would do if no match of this call blocked anything), rot_bin (-1: none).
    per call: hist, maxima, cleared_but_won_by_kept_bin."""
    R = PROJ_RULES if rules is None else rules
    nq, N = len(queries), F.N
    blocked = [bool(b) for b in has_observed_point]
    by_call = [-1] * N                      # the query of this call whose match blocks the slot
    assigned = [-1] * N
    takers = [[] for _ in range(N)]
    exits = np.full(nq, PX_SKIPPED, np.int32)
    zi = lambda v=0: np.full(nq, v, np.int32)
    facts = dict(n_window=zi(), n_blocked_before=zi(), n_blocked_by_call=zi(), depth=zi(), dep_min=zi(-1), best_idx=zi(-1),
                 best_dist=zi(256), second_dist=zi(256), best_ties=zi(), best_tie_out_of_index_order=np.zeros(nq, bool),
                 second_level_tied=np.zeros(nq, bool), matters_kept=zi(), ncol=zi(), best_pos=zi(-1), second_pos=zi(-1),
                 first_choice=zi(-1), first_accept=np.zeros(nq, bool), rot_bin=zi(-1))
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    use_gate = stereo_gate and F.u_right is not None
    use_hist = mode == 1 and check_orientation
    nn, thf = _f32(nnratio), _f32(th_high)
    nmatches = 0

    def step(s, dist, idx, pos):
        if R["best_lt"](dist, s[0]):
            s[2], s[3], s[6] = s[0], s[1], s[5]
            s[0], s[1], s[4], s[5] = dist, F.octave[idx], idx, pos
        elif R["second_lt"](dist, s[2]):
            s[2], s[3], s[6] = dist, F.octave[idx], pos

    def decide(s):
        if s[4] < 0:
            return PX_ALL_GONE
        if not R["accept"](s[0], th_high):
            return PX_TOO_FAR
        if mode == 0 and R["same_level"](s[1], s[3]) and R["ratio_reject"](_f32(s[0]), nn * _f32(s[2])):
            return PX_RATIO
        return PX_MATCHED

    for i in range(nq):
        q = queries[i]
        if not q["valid"]:
            continue
        info = {}
        r = _f32(q["radius"])
        vIndices = F.GetFeaturesInArea(q["u"], q["v"], r, int(q["min_level"]), int(q["max_level"]), R["in_box"], info)
        facts["ncol"][i] = info["ncol"]
        if not vIndices:
            exits[i] = PX_OUTSIDE_GRID if info["outside"] else PX_EMPTY_WINDOW
            continue
        s = [256, -1, 256, -1, -1, -1, -1]      # bestDist, bestLevel, bestDist2, bestLevel2, bestIdx and the places of the two
        s0 = list(s)                            # the same without the blocks this call has made
        open_ = []
        for idx, pos in zip(vIndices, info["raw_pos"]):
            gated = use_gate and R["has_right"](F.u_right[idx]) and R["gate_fail"](abs(_f32(q["u_r"]) - F.u_right[idx]), r)
            if gated:
                continue
            facts["n_window"][i] += 1
            dist = descriptor_distance(q["desc"], F.desc[idx])
            if blocked[idx] and by_call[idx] < 0:
                facts["n_blocked_before"][i] += 1
                continue
            if dist <= th_high or (mode == 0 and nn * _f32(dist) < thf):
                facts["matters_kept"][i] += 1
            step(s0, dist, idx, pos)
            if blocked[idx]:
                j = by_call[idx]
                facts["n_blocked_by_call"][i] += 1
                facts["depth"][i] = max(facts["depth"][i], 1 + facts["depth"][j])
                facts["dep_min"][i] = j if facts["dep_min"][i] < 0 else min(facts["dep_min"][i], j)
                continue
            step(s, dist, idx, pos)
            open_.append((idx, dist))
        facts["first_choice"][i] = s0[4]
        facts["first_accept"][i] = decide(s0) == PX_MATCHED
        exits[i] = decide(s)
        if s[4] >= 0:
            bestIdx = s[4]
            facts["best_idx"][i], facts["best_dist"][i], facts["second_dist"][i] = bestIdx, s[0], s[2]
            facts["best_pos"][i], facts["second_pos"][i] = s[5], s[6]
            tied = [idx for idx, d in open_ if d == s[0] and idx != bestIdx]
            facts["best_ties"][i] = len(tied)
            facts["best_tie_out_of_index_order"][i] = any(idx < bestIdx for idx in tied)
            facts["second_level_tied"][i] = len({F.octave[idx] for idx, d in open_ if d == s[2] and idx != bestIdx}) > 1
        if exits[i] != PX_MATCHED:
            continue
        if R["last_taker_wins"] or not takers[bestIdx]:
            assigned[bestIdx] = i
        takers[bestIdx].append(i)
        blocked[bestIdx] = R["blocks"](q["blocks"])
        by_call[bestIdx] = i if blocked[bestIdx] else -1
        nmatches += 1
        if use_hist:
            facts["rot_bin"][i] = _rot_bin(q["angle"], F.angle[bestIdx], R["round"])
            rotHist[facts["rot_bin"][i]].append((bestIdx, i))
    for t in takers:
        for i in t[:-1]:
            exits[i] = PX_OVERWRITTEN
    facts["hist"] = [len(h) for h in rotHist]
    facts["maxima"] = (-1, -1, -1)
    won = set()
    if use_hist:
        ind = facts["maxima"] = compute_three_maxima(facts["hist"], R["maxima_lt"])
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for idx, i in rotHist[b]:
                if R["rot_clears_all"] or assigned[idx] == i:
                    assigned[idx] = -1              # static_cast<MapPoint*>(NULL)
                    if R["rot_unblocks"]:
                        blocked[idx] = False
                    if takers[idx][-1] != i and facts["rot_bin"][takers[idx][-1]] in ind:
                        won.add(idx)
                nmatches -= 1
                exits[i] = PX_ROTATION
    facts["cleared_but_won_by_kept_bin"] = len(won)
    return nmatches, assigned, blocked, exits, facts


def ref_search_by_projection_points(F, points, nnratio, has_observed_point):
    """SearchByProjection(Frame&, vector<MapPoint*>&, th) (:45-128).  points: list of dicts with the MapPoint fields the loop
    reads after the caller's part -- skip (= !mbTrackInView || isBad()), proj_x, proj_y, proj_xr, level, radius
    (= r * mvScaleFactors[level]), observed (Observations() > 0), desc.  has_observed_point[idx]: F.mvpMapPoints[idx] exists
    with Observations() > 0 before the call.  Returns (nmatches, point index per keypoint or -1, and per keypoint whether
    F.mvpMapPoints[idx] holds a point with Observations() > 0 after the call)."""
    q = [dict(valid=False) if p["skip"] else
         dict(valid=True, u=p["proj_x"], v=p["proj_y"], u_r=p["proj_xr"], radius=p["radius"], min_level=p["level"] - 1,
              max_level=p["level"], blocks=p["observed"], angle=0.0, desc=p["desc"]) for p in points]
    return proj_walk(F, q, 0, nnratio, False, has_observed_point)[:3]


def _last_as_queries(last, blocks=None):
    return [dict(valid=False) if p["skip"] else
            dict(valid=True, u=p["u"], v=p["v"], u_r=p.get("ur", 0.0), radius=p["radius"], min_level=p["min_level"],
                 max_level=p["max_level"], blocks=p["observed"] if blocks is None else blocks, angle=p["angle"], desc=p["desc"])
            for p in last]


def ref_search_by_projection_frame(F, last, check_orientation, has_observed_point):
    """SearchByProjection(Frame& cur, const Frame& last, th, bMono) from the window search on (:1289-1383).  last: list of
    dicts per LastFrame keypoint -- skip (no point / outlier / behind the camera / outside the image), u, v, ur
    (= u - mbf * invzc), radius, min_level, max_level (the bForward / bBackward / default choice made by the caller),
    observed, angle (LastFrame.mvKeysUn[i].angle), desc.  Returns (nmatches, last-frame index per keypoint or -1, and per
    keypoint whether CurrentFrame.mvpMapPoints[idx] holds a point with Observations() > 0 after the call -- a slot the rotation
    check cleared is NULL again)."""
    return proj_walk(F, _last_as_queries(last), 1, 0.0, check_orientation, has_observed_point)[:3]


def ref_search_by_projection_keyframe(F, points, orb_dist, check_orientation, has_point):
    """SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) from the window search on (:1439-1501).
    points: as `last` above without ur and observed (there is no stereo gate, :1453 tests the slot for NULL and :1468 fills it:
    every match blocks).  has_point[i2]: CurrentFrame.mvpMapPoints[i2] != NULL on entry.  Returns (nmatches, point index per
    keypoint or -1, has_point after the call)."""
    return proj_walk(F, _last_as_queries(points, True), 1, 0.0, check_orientation, has_point, th_high=orb_dist, stereo_gate=False)[:3]


# ------------------------------------------------------------------------------------------------------------------------------
# The searches over common vocabulary nodes -- SearchByBoW(KeyFrame*, Frame&) (:161-273), SearchByBoW(KeyFrame*, KeyFrame*) (:494-612),
# SearchForTriangulation (:614-764) -- and SearchForInitialization (:388-492): one instrumented body each (bow_walk serves both
# SearchByBoW forms).  The ref_search_* functions below are thin readings of them, as the ref_search_by_projection_* are of proj_walk.
# Exits, one per VISIT of a first-side feature (a feature listed under several common nodes is visited once per node) and, in
# `exits`, the one of the last visit per first-side feature:
(NX_UNVISITED, NX_INVALID, NX_EMPTY, NX_ALL_GONE, NX_TOO_FAR, NX_RATIO, NX_MATCHED, NX_STOLEN, NX_ROTATION) = range(-1, 8)
# what removed a candidate of SearchForTriangulation, in the order the reference asks
(TG_INVALID, TG_FAR, TG_WORSE, TG_EPIPOLE, TG_DEN, TG_EPIPOLAR, TG_PASSED) = range(7)

# The reference's comparisons; a test swaps exactly one of them.  Swapping best_lt or second_lt changes no result where a ratio test
# follows (equal best candidates make best == second-best, which it rejects): see test_nodesearch_cpu.EQUIVALENT.
NODE_RULES = dict(
    best_lt=operator.lt,             # dist < bestDist1: of equal best candidates the first is named
    second_lt=operator.lt,           # dist < bestDist2
    accept_frame=operator.le,        # SearchByBoW(KF, F): bestDist1 <= TH_LOW
    accept_kf=operator.lt,           # SearchByBoW(KF, KF): bestDist1 < TH_LOW
    accept_init=operator.le,         # SearchForInitialization: bestDist <= TH_LOW
    ratio_lt=operator.lt,            # (float)bestDist1 < mfNNratio * (float)bestDist2
    ratio_float=True,                # ... a float product (False: the same in double)
    tri_far=operator.gt,             # dist > TH_LOW
    tri_worse=operator.gt,           # dist > bestDist: of equal candidates the LAST one wins
    has_right=lambda ur: ur >= 0,    # mvuRight[idx] >= 0
    disc_lt=operator.lt,             # distex * distex + distey * distey < 100 * mvScaleFactors[octave]
    disc_float=True,                 # ... in float (False: in double)
    epi_lt=operator.lt,              # dsqr < 3.84 * sigma2
    epi_double=True,                 # ... in double, 3.84 being a double constant (False: in float)
    den_zero=lambda den: den == 0,   # CheckDistEpipolarLine refuses a degenerate line
    kept_le=operator.le,             # vMatchedDistance[i2] <= dist: an equal distance cannot steal
    stolen_stay_in_hist=True,        # SearchForInitialization leaves the rotHist entry of a match that was stolen later
    max_gt1=operator.gt, max_gt2=operator.gt, max_gt3=operator.gt,    # ComputeThreeMaxima: s > max1 / max2 / max3
    max_lt2=operator.lt, max_lt3=operator.lt,                         # max2 < 0.1f * max1, max3 < 0.1f * max1
    round=c_round,                   # round(): halves away from zero
)


def _node_maxima(hist, R):
    return compute_three_maxima(hist, R["max_lt2"], R["max_gt1"], R["max_gt2"], R["max_gt3"], R["max_lt3"])


def _ratio_ok(R, best, second, nnratio):
    if R["ratio_float"]:
        return R["ratio_lt"](_f32(best), _f32(nnratio) * _f32(second))
    return R["ratio_lt"](float(best), float(_f32(nnratio)) * float(second))


def _featvec_pairs(fvA, fvB):
    """The lock-step walk over two DBoW2::FeatureVector maps (ascending node ids, lower_bound on a mismatch): yields
    (node id, list of A, list of B) for every node both hold."""
    idsA, idsB = sorted(fvA), sorted(fvB)
    a = b = 0
    while a < len(idsA) and b < len(idsB):
        if idsA[a] == idsB[b]:
            yield idsA[a], fvA[idsA[a]], fvB[idsB[b]]
            a += 1
            b += 1
        elif idsA[a] < idsB[b]:
            while a < len(idsA) and idsA[a] < idsB[b]:      # lower_bound
                a += 1
        else:
            while b < len(idsB) and idsB[b] < idsA[a]:
                b += 1


def _best_two(free, R):
    """free: [(position in the node's list, distance)] in list order.  Returns the walk's (bestDist1, position, bestDist2) and
    the facts of the pick: position of the first candidate at the second-best distance (-1), the positions tied at the best."""
    best, bpos, second = 256, -1, 256
    for pos, d in free:
        if R["best_lt"](d, best):
            second, best, bpos = best, d, pos
        elif R["second_lt"](d, second):
            second = d
    spos = next((p for p, d in free if d == second and p != bpos), -1)
    return best, bpos, second, spos, [p for p, d in free if d == best]


def _visit_facts(v, n_list, free, best, bpos, second, spos, ties):
    v.update(n_list=n_list, n_free=len(free), best=best, second=second, best_pos=bpos, second_pos=spos, tie_pos=ties,
             second_same_lane=spos >= 0 and spos % 64 == bpos % 64)


def _close_rotation(R, rotHist, visits, clear):
    """the rotation check behind a walk: rotHist[bin] = [visit index]; clear(visit) removes its match and tells whether the reference
    decrements nmatches for it.  Returns (hist, maxima, decrements)."""
    hist = [len(h) for h in rotHist]
    ind = _node_maxima(hist, R)
    dec = 0
    for b in range(HISTO_LENGTH):
        if b in ind:
            continue
        for k in rotHist[b]:
            if clear(visits[k]):
                dec += 1
    return hist, ind, dec


def _node_result(n_first, visits, **facts):
    exits = np.full(n_first, NX_UNVISITED, np.int32)
    pushes = np.zeros(n_first, np.int32)
    for v in visits:
        exits[v["a"]] = v["exit"]
        pushes[v["a"]] += v["bin"] >= 0
    facts.update(visits=visits, pushes=pushes)
    return exits, facts


def bow_walk(descA, angleA, validA, fvA, descB, angleB, validB, fvB, nnratio, check_orientation, kf_mode, rules=None):
    """Both SearchByBoW forms read literally.  kf_mode False: SearchByBoW(KeyFrame*, Frame&) -- validB is not read, the result is the
    keyframe feature per frame feature; True: SearchByBoW(pKF1, pKF2) -- the result is the index in keyframe 2 per feature of keyframe 1.
    Returns (nmatches, result, exits, facts).  facts["visits"]: one dict per visit -- a, node, exit, n_list, n_free, best, second
    (256: none), best_pos / second_pos (places in the node's second-side list, the lane being place % 64), second_same_lane, tie_pos,
    match (the second-side feature, -1), bin (-1: no entry pushed); facts["pushes"] per first-side feature; hist, maxima, n_pairs,
    dup_a / dup_b (a feature met under two visits / listed twice among the common nodes)."""
    R = NODE_RULES if rules is None else rules
    nA, nB = len(descA), len(descB)
    matchesB = [-1] * nB                 # KF-F: vpMapPointMatches;  KF-KF: vbMatched2 as "the visit that took it"
    matches12 = [-1] * nA
    owner12 = [-1] * nA                  # the visit whose match vpMatches12[idx1] holds
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    visits = []
    nmatches = n_pairs = 0
    seenA, seenB, dup_a, dup_b = set(), set(), False, False
    accept = R["accept_kf"] if kf_mode else R["accept_frame"]
    for nid, listA, listB in _featvec_pairs(fvA, fvB):
        n_pairs += 1
        dup_b = dup_b or len(set(listB)) < len(listB) or bool(seenB & set(listB))
        seenB |= set(listB)
        for idxA in listA:
            dup_a = dup_a or idxA in seenA
            seenA.add(idxA)
            v = dict(a=idxA, node=nid, exit=NX_INVALID, match=-1, bin=-1)
            visits.append(v)
            if not validA[idxA]:
                continue
            free = [(pos, descriptor_distance(descA[idxA], descB[j])) for pos, j in enumerate(listB)
                    if matchesB[j] < 0 and not (kf_mode and not validB[j])]
            best, bpos, second, spos, ties = _best_two(free, R)
            _visit_facts(v, len(listB), free, best, bpos, second, spos, ties)
            if bpos < 0:
                v["exit"] = NX_EMPTY if not listB else NX_ALL_GONE
            elif not accept(best, TH_LOW):
                v["exit"] = NX_TOO_FAR
            elif not _ratio_ok(R, best, second, nnratio):
                v["exit"] = NX_RATIO
            else:
                j = listB[bpos]
                v["exit"], v["match"] = NX_MATCHED, j
                matchesB[j] = idxA
                if kf_mode:
                    if owner12[idxA] >= 0:
                        visits[owner12[idxA]]["exit"] = NX_STOLEN      # overwritten: both stay counted
                    matches12[idxA], owner12[idxA] = j, len(visits) - 1
                nmatches += 1
                if check_orientation:
                    v["bin"] = _rot_bin(angleA[idxA], angleB[j], R["round"])
                    rotHist[v["bin"]].append(len(visits) - 1)
    hist, ind = [0] * HISTO_LENGTH, (-1, -1, -1)
    if check_orientation:
        def clear(v):
            v["exit"] = NX_ROTATION
            if kf_mode:
                matches12[v["a"]] = -1          # vpMatches12[rotHist[i][j]] = NULL, whichever visit wrote it last
            else:
                matchesB[v["match"]] = -1
            return True
        hist, ind, dec = _close_rotation(R, rotHist, visits, clear)
        nmatches -= dec
    result = np.array(matches12 if kf_mode else matchesB, np.int32).reshape(-1)
    exits, facts = _node_result(nA, visits, hist=hist, maxima=ind, n_pairs=n_pairs, dup_a=dup_a, dup_b=dup_b)
    return nmatches, result, exits, facts


def ref_search_by_bow(descKF, angleKF, validKF, featvecKF, descF, angleF, featvecF, nnratio, check_orientation):
    """SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (:161-273).  featvec*: {node id: [feature indices]} (DBoW2::FeatureVector
    is a std::map: ascending ids); validKF[i]: the keyframe's map point i exists and is not bad.  Returns (nmatches,
    keyframe feature index per frame feature or -1)."""
    nm, matches = bow_walk(descKF, angleKF, validKF, featvecKF, descF, angleF, None, featvecF, nnratio, check_orientation, False)[:2]
    return nm, matches.tolist()


def ref_search_by_bow_kf(desc1, angle1, valid1, featvec1, desc2, angle2, valid2, featvec2, nnratio, check_orientation):
    """SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (:494-612).  valid*[i]: the keyframe's map point i exists and is not
    bad.  Returns (nmatches, index in keyframe 2 per feature of keyframe 1 or -1)."""
    nm, m12 = bow_walk(desc1, angle1, valid1, featvec1, desc2, angle2, valid2, featvec2, nnratio, check_orientation, True)[:2]
    return nm, m12.tolist()


def check_dist_epipolar_line(x1, y1, x2, y2, octave2, F12, level_sigma2):
    """ORBmatcher::CheckDistEpipolarLine (:137-159)"""
    return _epipolar_gate(x1, y1, x2, y2, octave2, F12, level_sigma2) == TG_PASSED


def _epipolar_gate(x1, y1, x2, y2, octave2, F12, level_sigma2, rules=None):
    """CheckDistEpipolarLine: float products and sums left to right, the last comparison in double (3.84 is a double constant).
    Returns the gate that refused (TG_DEN, TG_EPIPOLAR) or TG_PASSED."""
    R = NODE_RULES if rules is None else rules
    F = [[_f32(F12[r][c]) for c in range(3)] for r in range(3)]
    x1, y1, x2, y2 = _f32(x1), _f32(y1), _f32(x2), _f32(y2)
    a = x1 * F[0][0] + y1 * F[1][0] + F[2][0]
    b = x1 * F[0][1] + y1 * F[1][1] + F[2][1]
    c = x1 * F[0][2] + y1 * F[1][2] + F[2][2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if R["den_zero"](den):
        return TG_DEN
    dsqr = num * num / den
    if R["epi_double"]:
        ok = R["epi_lt"](float(dsqr), 3.84 * float(_f32(level_sigma2[octave2])))
    else:
        ok = R["epi_lt"](dsqr, _f32(3.84) * _f32(level_sigma2[octave2]))
    return TG_PASSED if ok else TG_EPIPOLAR


def tri_walk(keys1, desc1, u_right1, has_mp1, featvec1, keys2, desc2, u_right2, has_mp2, featvec2, F12, ex, ey, scale_factors,
             level_sigma2, only_stereo, check_orientation, rules=None):
    """SearchForTriangulation read literally.  Returns (nmatches, vMatches12, exits, facts); a visit carries, beside the fields of
    bow_walk's, gates: one TG_* per entry of the node's second-side list (which gate removed the candidate), and best_pos / tie_pos
    over the candidates that passed every gate at the winning distance."""
    R = NODE_RULES if rules is None else rules
    n1, n2 = len(keys1), len(keys2)
    ur1 = [_f32(-1)] * n1 if u_right1 is None else [_f32(v) for v in u_right1]
    ur2 = [_f32(-1)] * n2 if u_right2 is None else [_f32(v) for v in u_right2]
    ex, ey = _f32(ex), _f32(ey)
    vbMatched2 = [False] * n2           # read, never set (:677) -- kept so
    vMatches12 = [-1] * n1
    owner12 = [-1] * n1
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    visits = []
    nmatches = n_pairs = 0
    seenA, dup_a = set(), False
    for nid, node1, node2 in _featvec_pairs(featvec1, featvec2):
        n_pairs += 1
        for idx1 in node1:
            dup_a = dup_a or idx1 in seenA
            seenA.add(idx1)
            v = dict(a=idx1, node=nid, exit=NX_INVALID, match=-1, bin=-1, gates=[])
            visits.append(v)
            if has_mp1[idx1]:
                continue
            bStereo1 = bool(R["has_right"](ur1[idx1]))
            if only_stereo and not bStereo1:
                continue
            bestDist, bestIdx2, bpos = TH_LOW, -1, -1
            passed = []
            for pos, idx2 in enumerate(node2):
                bStereo2 = bool(R["has_right"](ur2[idx2]))
                if vbMatched2[idx2] or has_mp2[idx2] or (only_stereo and not bStereo2):
                    v["gates"].append(TG_INVALID)
                    continue
                dist = descriptor_distance(desc1[idx1], desc2[idx2])
                if R["tri_far"](dist, TH_LOW):
                    v["gates"].append(TG_FAR)
                    continue
                if R["tri_worse"](dist, bestDist):
                    v["gates"].append(TG_WORSE)
                    continue
                x2, y2, o2 = _f32(keys2["x"][idx2]), _f32(keys2["y"][idx2]), int(keys2["octave"][idx2])
                if not bStereo1 and not bStereo2:
                    distex = ex - x2
                    distey = ey - y2
                    if R["disc_float"]:
                        inside = R["disc_lt"](distex * distex + distey * distey, _f32(100) * _f32(scale_factors[o2]))
                    else:
                        inside = R["disc_lt"](float(distex) * float(distex) + float(distey) * float(distey), 100.0 * float(_f32(scale_factors[o2])))
                    if inside:
                        v["gates"].append(TG_EPIPOLE)
                        continue
                g = _epipolar_gate(keys1["x"][idx1], keys1["y"][idx1], x2, y2, o2, F12, level_sigma2, R)
                v["gates"].append(g)
                if g == TG_PASSED:
                    bestIdx2, bestDist, bpos = idx2, dist, pos
                    passed.append((pos, dist))
            g = v["gates"]
            v.update(n_list=len(node2), n_free=len(passed), best=bestDist if bpos >= 0 else 256, second=256, best_pos=bpos, second_pos=-1,
                     tie_pos=[p for p, d in passed if d == bestDist], second_same_lane=False)
            if bestIdx2 < 0:
                v["exit"] = (NX_EMPTY if not node2 else NX_ALL_GONE if any(t in (TG_EPIPOLE, TG_DEN, TG_EPIPOLAR) for t in g) or TG_FAR not in g
                             else NX_TOO_FAR)
                continue
            v["exit"], v["match"] = NX_MATCHED, bestIdx2
            if owner12[idx1] >= 0:
                visits[owner12[idx1]]["exit"] = NX_STOLEN
            vMatches12[idx1], owner12[idx1] = bestIdx2, len(visits) - 1
            nmatches += 1
            if check_orientation:
                v["bin"] = _rot_bin(keys1["angle"][idx1], keys2["angle"][bestIdx2], R["round"])
                rotHist[v["bin"]].append(len(visits) - 1)
    hist, ind = [0] * HISTO_LENGTH, (-1, -1, -1)
    if check_orientation:
        def clear(v):
            v["exit"] = NX_ROTATION
            vMatches12[v["a"]] = -1
            return True
        hist, ind, dec = _close_rotation(R, rotHist, visits, clear)
        nmatches -= dec
    exits, facts = _node_result(n1, visits, hist=hist, maxima=ind, n_pairs=n_pairs, dup_a=dup_a, dup_b=False)
    return nmatches, np.array(vMatches12, np.int32).reshape(-1), exits, facts


def ref_search_for_triangulation(keys1, desc1, u_right1, has_mp1, featvec1, keys2, desc2, u_right2, has_mp2, featvec2, F12, ex, ey,
                                 scale_factors, level_sigma2, only_stereo, check_orientation):
    """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (:614-764) after the epipole (ex, ey) has been formed.
    u_right*: mvuRight or None (monocular: every value -1).  vbMatched2 is read but never set by the reference -- kept so.  Returns
    (nmatches, vMatches12)."""
    nm, m12 = tri_walk(keys1, desc1, u_right1, has_mp1, featvec1, keys2, desc2, u_right2, has_mp2, featvec2, F12, ex, ey, scale_factors,
                       level_sigma2, only_stereo, check_orientation)[:2]
    return nm, m12.tolist()


def init_walk(keys1, desc1, F2, prev_matched, window, nnratio, check_orientation, rules=None):
    """SearchForInitialization read literally.  Returns (nmatches, vnMatches12, updated vbPrevMatched, exits, facts): one visit per
    keypoint of F1 (facts["visits"][i1]) with, beside bow_walk's fields, outside (the window missed the grid), n_kept (candidates
    an earlier, closer or equal match keeps), n_kept_equal (... at exactly the distance), victim (the F1 keypoint the match was
    stolen from, -1), depth (1 + the victim's depth), bin; facts["hist_stolen"]: histogram entries whose match was stolen before
    the rotation check ran."""
    R = NODE_RULES if rules is None else rules
    INT_MAX = 2 ** 31 - 1
    n1 = len(keys1)
    prev = [(_f32(p[0]), _f32(p[1])) for p in prev_matched]
    vnMatches12 = [-1] * n1
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    vMatchedDistance = [INT_MAX] * F2.N
    vnMatches21 = [-1] * F2.N
    visits = []
    nmatches = 0
    for i1 in range(n1):
        v = dict(a=i1, node=0, exit=NX_INVALID, match=-1, bin=-1, victim=-1, depth=0, outside=False, n_kept=0, n_kept_equal=0)
        visits.append(v)
        level1 = int(keys1["octave"][i1])
        if level1 > 0:
            continue
        info = {}
        vIndices2 = F2.GetFeaturesInArea(prev[i1][0], prev[i1][1], window, level1, level1, info=info)
        v["outside"] = info["outside"]
        if not vIndices2:
            v["exit"] = NX_EMPTY
            _visit_facts(v, 0, [], 256, -1, 256, -1, [])
            continue
        free = []
        for pos, i2 in enumerate(vIndices2):
            dist = descriptor_distance(desc1[i1], F2.desc[i2])
            if R["kept_le"](vMatchedDistance[i2], dist):
                v["n_kept"] += 1
                v["n_kept_equal"] += vMatchedDistance[i2] == dist
                continue
            free.append((pos, dist))
        best, bpos, second, spos, ties = _best_two(free, R)
        _visit_facts(v, len(vIndices2), free, best, bpos, second, spos, ties)
        if bpos < 0:
            v["exit"] = NX_ALL_GONE
        elif not R["accept_init"](best, TH_LOW):
            v["exit"] = NX_TOO_FAR
        elif not _ratio_ok(R, best, INT_MAX if second == 256 else second, nnratio):
            v["exit"] = NX_RATIO
        else:
            bestIdx2 = vIndices2[bpos]
            if vnMatches21[bestIdx2] >= 0:
                w = vnMatches21[bestIdx2]
                vnMatches12[w] = -1
                nmatches -= 1
                visits[w]["exit"] = NX_STOLEN
                v["victim"], v["depth"] = w, 1 + visits[w]["depth"]
                if not R["stolen_stay_in_hist"] and visits[w]["bin"] >= 0:
                    rotHist[visits[w]["bin"]].remove(w)
            vnMatches12[i1] = bestIdx2
            vnMatches21[bestIdx2] = i1
            vMatchedDistance[bestIdx2] = best
            nmatches += 1
            v["exit"], v["match"] = NX_MATCHED, bestIdx2
            if check_orientation:
                v["bin"] = _rot_bin(keys1["angle"][i1], F2.angle[bestIdx2], R["round"])
                rotHist[v["bin"]].append(i1)
    hist, ind, hist_stolen = [0] * HISTO_LENGTH, (-1, -1, -1), 0
    if check_orientation:
        hist_stolen = sum(vnMatches12[i] < 0 for h in rotHist for i in h)

        def clear(v):
            if vnMatches12[v["a"]] >= 0:
                vnMatches12[v["a"]] = -1
                v["exit"] = NX_ROTATION
                return True
            return False
        hist, ind, dec = _close_rotation(R, rotHist, visits, clear)
        nmatches -= dec
    for i1 in range(n1):
        if vnMatches12[i1] >= 0:
            prev[i1] = (F2.x[vnMatches12[i1]], F2.y[vnMatches12[i1]])
    exits, facts = _node_result(n1, visits, hist=hist, maxima=ind, hist_stolen=hist_stolen)
    return nmatches, np.array(vnMatches12, np.int32).reshape(-1), prev, exits, facts


def ref_search_for_initialization(keys1, desc1, F2, prev_matched, window, nnratio, check_orientation):
    """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (:388-492).  Returns (nmatches, vnMatches12,
    updated vbPrevMatched)."""
    nm, m12, prev = init_walk(keys1, desc1, F2, prev_matched, window, nnratio, check_orientation)[:3]
    return nm, m12.tolist(), prev


# the ways a left keypoint leaves Frame::ComputeStereoMatches, in the order the walk below meets them
(SX_OUTSIDE, SX_ROW_EMPTY, SX_NO_CANDIDATE, SX_HAMMING, SX_LEFT_WINDOW, SX_RIGHT_SPAN, SX_RIGHT_WINDOW, SX_END_SHIFT, SX_DELTA,
 SX_DISPARITY, SX_CLAMPED, SX_MATCHED, SX_MEDIAN) = range(13)


def stereo_walk(keysL, descL, keysR, descR, pyrL, pyrR, scale_factors, inv_scale_factors, mbf, mb):
    """The one body of the second reading of Frame::ComputeStereoMatches (L/src/Frame.cc:477-646).  Returns (mvuRight, mvDepth,
    exits, facts): `exits` holds one SX_* code per left keypoint (SX_MEDIAN replaces SX_MATCHED / SX_CLAMPED where the median rule
    removed the match), `facts` what the walk saw on its way (tests/np_stereo.py names the entries).  ref_compute_stereo_matches
    keeps the first two; tests/np_stereo.stereo_exits hands out all four."""
    N = len(keysL)
    mvuRight = np.full(N, -1.0, np.float32); mvDepth = np.full(N, -1.0, np.float32)
    exits = np.full(N, SX_OUTSIDE, np.int32)
    facts = dict(run=np.zeros(N, np.int32), hamming_ties=np.zeros(N, np.int32), hamming_ties_dx=np.zeros(N, bool),
                 best_dist=np.full(N, -1, np.int32), best_idx=np.full(N, -1, np.int32), sad_ties=np.zeros(N, np.int32),
                 sad=np.full(N, -1, np.int32), best_inc=np.zeros(N, np.int32), delta=np.full(N, np.nan, np.float32),
                 touches=np.zeros(N, bool), at_min_u=np.zeros(N, np.int32), at_max_u=np.zeros(N, np.int32),
                 clamped=np.zeros(N, bool), clipped_top=np.zeros(len(keysR), bool), clipped_bottom=np.zeros(len(keysR), bool),
                 median_in=[], median=None)
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyrL[0].shape[0]
    vRowIndices = [[] for _ in range(nRows)]
    for iR in range(len(keysR)):
        kpY = _f32(keysR["y"][iR])
        r = _f32(2.0) * _f32(scale_factors[int(keysR["octave"][iR])])
        maxr = int(math.ceil(kpY + r)); minr = int(math.floor(kpY - r))
        facts["clipped_top"][iR] = minr < 0; facts["clipped_bottom"][iR] = maxr >= nRows
        for yi in range(minr, maxr + 1):
            if 0 <= yi < nRows:
                vRowIndices[yi].append(iR)
    minZ = _f32(mb); minD = _f32(0); maxD = _f32(mbf) / minZ
    vDistIdx = []
    descR = np.asarray(descR, np.uint8)
    for iL in range(N):
        levelL = int(keysL["octave"][iL]); vL = _f32(keysL["y"][iL]); uL = _f32(keysL["x"][iL])
        row = int(vL)
        if row < 0 or row >= nRows:
            continue
        vCandidates = vRowIndices[row]
        exits[iL] = SX_ROW_EMPTY
        if not vCandidates:
            continue
        minU = uL - maxD; maxU = uL - minD
        exits[iL] = SX_OUTSIDE
        if maxU < 0:
            continue
        bestDist = TH_HIGH; bestIdxR = 0
        nCand = 0; tied = []
        for iR in vCandidates:
            oR = int(keysR["octave"][iR])
            if oR < levelL - 1 or oR > levelL + 1:
                continue
            facts["run"][iL] += 1
            uR = _f32(keysR["x"][iR])
            if uR >= minU and uR <= maxU:
                nCand += 1
                facts["at_min_u"][iL] += int(uR == minU); facts["at_max_u"][iL] += int(uR == maxU)
                dist = descriptor_distance(descL[iL], descR[iR])
                if dist < bestDist:
                    bestDist = dist; bestIdxR = iR; tied = [iR]
                elif dist == bestDist:
                    tied.append(iR)
        exits[iL] = SX_HAMMING if nCand else SX_NO_CANDIDATE
        if nCand:
            facts["best_dist"][iL] = bestDist
        if not (bestDist < thOrbDist):
            continue
        facts["best_idx"][iL] = bestIdxR
        facts["hamming_ties"][iL] = len(tied) - 1
        facts["hamming_ties_dx"][iL] = any(keysR["x"][j] != keysR["x"][bestIdxR] for j in tied)
        uR0 = _f32(keysR["x"][bestIdxR])
        scaleFactor = _f32(inv_scale_factors[levelL])
        scaleduL = _f32(c_round(uL * scaleFactor)); scaledvL = _f32(c_round(vL * scaleFactor)); scaleduR0 = _f32(c_round(uR0 * scaleFactor))
        w = 5; L = 5
        imL, imR = pyrL[levelL], pyrR[levelL]
        y0, x0 = int(scaledvL - w), int(scaleduL - w)
        exits[iL] = SX_LEFT_WINDOW
        if y0 < 0 or y0 + 2 * w + 1 > imL.shape[0] or x0 < 0 or x0 + 2 * w + 1 > imL.shape[1]:
            continue      # cv::Mat::rowRange / colRange would throw
        IL = imL[y0:y0 + 2 * w + 1, x0:x0 + 2 * w + 1].astype(np.float32)
        IL = IL - IL[w, w]
        iniu = scaleduR0 + _f32(L) - _f32(w); endu = scaleduR0 + _f32(L) + _f32(w) + _f32(1)
        exits[iL] = SX_RIGHT_SPAN
        if iniu < 0 or endu >= imR.shape[1]:
            continue
        xr = int(scaleduR0)
        exits[iL] = SX_RIGHT_WINDOW
        if xr - L - w < 0 or xr + L + w + 1 > imR.shape[1] or y0 + 2 * w + 1 > imR.shape[0]:
            continue
        facts["touches"][iL] = (y0 == 0 or y0 + 2 * w + 1 == imL.shape[0] or x0 == 0 or x0 + 2 * w + 1 == imL.shape[1] or
                                xr - L - w == 0 or xr + L + w + 1 == imR.shape[1])
        bestD = 2 ** 31 - 1; bestincR = 0
        vDists = [0.0] * (2 * L + 1)
        for incR in range(-L, L + 1):
            IR = imR[y0:y0 + 2 * w + 1, xr + incR - w:xr + incR + w + 1].astype(np.float32)
            IR = IR - IR[w, w]
            dist = _f32(np.abs(IL - IR).sum(dtype=np.float64))     # NORM_L1 of integer-valued floats: exact
            if dist < bestD:
                bestD = int(dist); bestincR = incR
            vDists[L + incR] = dist
        facts["sad_ties"][iL] = sum(1 for d in vDists if d == bestD) - 1
        facts["sad"][iL] = bestD; facts["best_inc"][iL] = bestincR
        exits[iL] = SX_END_SHIFT
        if bestincR == -L or bestincR == L:
            continue
        dist1, dist2, dist3 = _f32(vDists[L + bestincR - 1]), _f32(vDists[L + bestincR]), _f32(vDists[L + bestincR + 1])
        den = _f32(2.0) * (dist1 + dist3 - _f32(2.0) * dist2)
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = (dist1 - dist3) / den
        facts["delta"][iL] = deltaR
        exits[iL] = SX_DELTA
        if deltaR < -1 or deltaR > 1:
            continue
        bestuR = _f32(scale_factors[levelL]) * (scaleduR0 + _f32(bestincR) + deltaR)
        disparity = uL - bestuR
        exits[iL] = SX_DISPARITY
        if disparity >= minD and disparity < maxD:
            exits[iL] = SX_MATCHED
            if disparity <= 0:
                disparity = _f32(0.01)
                bestuR = _f32(float(uL) - 0.01)
                exits[iL] = SX_CLAMPED; facts["clamped"][iL] = True
            mvDepth[iL] = _f32(mbf) / disparity
            mvuRight[iL] = bestuR
            vDistIdx.append((bestD, iL))
    if vDistIdx:
        vDistIdx.sort()
        facts["median_in"] = [d for d, _ in vDistIdx]
        median = _f32(vDistIdx[len(vDistIdx) // 2][0])
        facts["median"] = int(median)
        thDist = _f32(1.5) * _f32(1.4) * median
        for i in range(len(vDistIdx) - 1, -1, -1):
            if vDistIdx[i][0] < thDist:
                break
            mvuRight[vDistIdx[i][1]] = -1; mvDepth[vDistIdx[i][1]] = -1
            exits[vDistIdx[i][1]] = SX_MEDIAN
    return mvuRight, mvDepth, exits, facts


def ref_compute_stereo_matches(keysL, descL, keysR, descR, pyrL, pyrR, scale_factors, inv_scale_factors, mbf, mb):
    """Frame::ComputeStereoMatches (L/src/Frame.cc:477-646), second reading (per-row Python lists, numpy windows).  pyrL / pyrR:
    lists of the level images of the two extractors' mvImagePyramid.  Returns (mvuRight, mvDepth) as float32 arrays.  Where the
    reference would index out of range (rows outside the image, windows leaving a level) the keypoint gets no match."""
    return stereo_walk(keysL, descL, keysR, descR, pyrL, pyrR, scale_factors, inv_scale_factors, mbf, mb)[:2]


# ------------------------------------------------------------------------------------------------------------------------------
# Second reading of the keyframe-rate projection searches (Fuse x2, SearchBySim3, SearchByProjection(KF, Scw) and
# SearchByProjection(Frame, KF)).  cv::Mat arithmetic as DESIGN.md's primitive list has it (the same assumptions as the C
# oracle -- this reading checks the loops, gates and orders, not OpenCV's kernels): A * x + b on 3x3 / 3x1 CV_32F = float dot
# products, the sum with b in double, rounded once; cv::norm and Mat::dot accumulate in double.  logf comes from the C library
# (MapPoint::PredictScale calls std::log on a float).
import ctypes as _ct
import ctypes.util as _ctu

_libm = _ct.CDLL(_ctu.find_library("m") or "libm.so.6")
_libm.logf.restype = _ct.c_float
_libm.logf.argtypes = [_ct.c_float]


def _gemm3(R, x, t):
    out = []
    for r in range(3):
        d = _f32(R[3 * r]) * _f32(x[0]) + _f32(R[3 * r + 1]) * _f32(x[1]) + _f32(R[3 * r + 2]) * _f32(x[2])
        out.append(_f32(float(d) * 1.0 + float(_f32(t[r])) * 1.0))
    return out


def _norm3(v):
    s = 0.0
    for e in v:
        s += float(e) * float(e)
    return _f32(math.sqrt(s))


def _dot3(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s += float(x) * float(y)
    return s


def predict_scale(max_distance, current_dist, log_scale_factor, n_levels):
    """MapPoint::PredictScale (MapPoint.cc:393-423): ceil(logf(ratio) / mfLogScaleFactor) in float, clamped."""
    ratio = _f32(max_distance) / _f32(current_dist)
    n = int(math.ceil(_f32(_libm.logf(float(ratio))) / _f32(log_scale_factor)))
    return 0 if n < 0 else (n_levels - 1 if n >= n_levels else n)


def _kf_in_image(cam, u, v):
    """KeyFrame::IsInImage (KeyFrame.cc:569-571)."""
    return u >= cam["min_x"] and u < cam["max_x"] and v >= cam["min_y"] and v < cam["max_y"]


def _pinhole(cam, pc, double_invz):
    """u, v of a camera-frame point.  `1 / z` is a float division in Fuse and SearchByProjection(KF, Scw) (:797, :317), `1.0 / z` a
    double one in Fuse(Sim3) and SearchBySim3 (:945, :1083)."""
    invz = _f32(1.0 / float(pc[2])) if double_invz else _f32(1) / pc[2]
    x = pc[0] * invz
    y = pc[1] * invz
    return cam["fx"] * x + cam["cx"], cam["fy"] * y + cam["cy"], invz


def _viewing_gates(cam, p):
    """dist3D inside [0.8 min, 1.2 max] and PO . Pn >= 0.5 dist3D; returns dist3D or None."""
    PO = [_f32(p["pos"][k]) - _f32(cam["Ow"][k]) for k in range(3)]
    dist3D = _norm3(PO)
    if dist3D < _f32(0.8) * _f32(p["min_distance"]) or dist3D > _f32(1.2) * _f32(p["max_distance"]):
        return None
    if _dot3(PO, [_f32(v) for v in p["normal"]]) < 0.5 * float(dist3D):
        return None
    return dist3D


def _cam_f32(cam):
    c = {k: (_f32(v) if np.ndim(v) == 0 and k != "n_levels" else v) for k, v in cam.items()}
    c["n_levels"] = int(cam["n_levels"])
    return c


def ref_fuse(KF, inv_level_sigma2, cam, points):
    """Fuse(KeyFrame*, vpMapPoints, th) (:766-912) up to the map update: per point the keypoint the reference acts on (bestIdx when
    bestDist <= TH_LOW is the caller's test; here (bestIdx, bestDist) or (-1, 256)).  KF: RefFrame of the keyframe (the grid is the
    Frame's); points[i]: pos, normal, min_distance, max_distance, skip (NULL / isBad / IsInKeyFrame), desc."""
    cam = _cam_f32(cam)
    out = []
    for p in points:
        res = (-1, 256)
        out.append(res)
        if p["skip"]:
            continue
        pc = _gemm3(cam["R"], p["pos"], cam["t"])
        if pc[2] < _f32(0.0):
            continue
        u, v, invz = _pinhole(cam, pc, False)
        if not _kf_in_image(cam, u, v):
            continue
        ur = u - cam["mbf"] * invz
        dist3D = _viewing_gates(cam, p)
        if dist3D is None:
            continue
        lvl = predict_scale(p["max_distance"], dist3D, cam["log_scale_factor"], cam["n_levels"])
        radius = cam["th"] * _f32(cam["scale_factors"][lvl])
        vIndices = KF.GetFeaturesInArea(u, v, radius)
        if not vIndices:
            continue
        bestDist, bestIdx = 256, -1
        for idx in vIndices:
            kpLevel = KF.octave[idx]
            if kpLevel < lvl - 1 or kpLevel > lvl:
                continue
            ex = u - KF.x[idx]
            ey = v - KF.y[idx]
            if KF.u_right is not None and KF.u_right[idx] >= 0:
                er = ur - KF.u_right[idx]
                e2 = ex * ex + ey * ey + er * er
                if float(e2 * _f32(inv_level_sigma2[kpLevel])) > 7.8:
                    continue
            else:
                e2 = ex * ex + ey * ey
                if float(e2 * _f32(inv_level_sigma2[kpLevel])) > 5.99:
                    continue
            dist = descriptor_distance(p["desc"], KF.desc[idx])
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
        out[-1] = (bestIdx, bestDist if bestIdx >= 0 else 256)
    return out


def ref_fuse_sim3(KF, cam, points):
    """Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:914-1041) after Scw has been decomposed (cam: R, t, Ow), up to the map
    update.  skip = isBad() or already a point of the keyframe."""
    cam = _cam_f32(cam)
    out = []
    for p in points:
        out.append((-1, 256))
        if p["skip"]:
            continue
        pc = _gemm3(cam["R"], p["pos"], cam["t"])
        if pc[2] < _f32(0.0):
            continue
        u, v, _ = _pinhole(cam, pc, True)
        if not _kf_in_image(cam, u, v):
            continue
        dist3D = _viewing_gates(cam, p)
        if dist3D is None:
            continue
        lvl = predict_scale(p["max_distance"], dist3D, cam["log_scale_factor"], cam["n_levels"])
        vIndices = KF.GetFeaturesInArea(u, v, cam["th"] * _f32(cam["scale_factors"][lvl]))
        if not vIndices:
            continue
        bestDist, bestIdx = 2 ** 31 - 1, -1
        for idx in vIndices:
            if KF.octave[idx] < lvl - 1 or KF.octave[idx] > lvl:
                continue
            dist = descriptor_distance(p["desc"], KF.desc[idx])
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
        out[-1] = (bestIdx, bestDist if bestIdx >= 0 else 256)
    return out


def ref_search_by_sim3_dir(KF, cam, points):
    """One direction of SearchBySim3 (:1063-1146; :1149-1222 with the roles swapped): cam R/t = the source keyframe's pose, R2/t2 =
    sR21 / t21; no viewing-angle gate, the distance is that of the point in the target camera."""
    cam = _cam_f32(cam)
    out = []
    for p in points:
        out.append((-1, 256))
        if p["skip"]:
            continue
        pc1 = _gemm3(cam["R"], p["pos"], cam["t"])
        pc2 = _gemm3(cam["R2"], pc1, cam["t2"])
        if float(pc2[2]) < 0.0:
            continue
        u, v, _ = _pinhole(cam, pc2, True)
        if not _kf_in_image(cam, u, v):
            continue
        dist3D = _norm3(pc2)
        if dist3D < _f32(0.8) * _f32(p["min_distance"]) or dist3D > _f32(1.2) * _f32(p["max_distance"]):
            continue
        lvl = predict_scale(p["max_distance"], dist3D, cam["log_scale_factor"], cam["n_levels"])
        vIndices = KF.GetFeaturesInArea(u, v, cam["th"] * _f32(cam["scale_factors"][lvl]))
        if not vIndices:
            continue
        bestDist, bestIdx = 2 ** 31 - 1, -1
        for idx in vIndices:
            if KF.octave[idx] < lvl - 1 or KF.octave[idx] > lvl:
                continue
            dist = descriptor_distance(p["desc"], KF.desc[idx])
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
        out[-1] = (bestIdx, bestDist if bestIdx >= 0 else 256)
    return out


def ref_search_by_projection_kf_scw(KF, cam, points, matched, th_low=TH_LOW):
    """SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (:275-386) after the decomposition of Scw.  matched[idx]:
    vpMatched[idx] != NULL on entry.  Returns (nmatches, keypoint index written per point or -1, updated matched)."""
    cam = _cam_f32(cam)
    vpMatched = [bool(m) for m in matched]
    written = []
    nmatches = 0
    for p in points:
        written.append(-1)
        if p["skip"]:
            continue
        pc = _gemm3(cam["R"], p["pos"], cam["t"])
        if float(pc[2]) < 0.0:
            continue
        u, v, _ = _pinhole(cam, pc, False)
        if not _kf_in_image(cam, u, v):
            continue
        dist = _viewing_gates(cam, p)
        if dist is None:
            continue
        lvl = predict_scale(p["max_distance"], dist, cam["log_scale_factor"], cam["n_levels"])
        vIndices = KF.GetFeaturesInArea(u, v, cam["th"] * _f32(cam["scale_factors"][lvl]))
        if not vIndices:
            continue
        bestDist, bestIdx = 256, -1
        for idx in vIndices:
            if vpMatched[idx]:
                continue
            if KF.octave[idx] < lvl - 1 or KF.octave[idx] > lvl:
                continue
            d = descriptor_distance(p["desc"], KF.desc[idx])
            if d < bestDist:
                bestDist, bestIdx = d, idx
        if bestDist <= th_low:
            vpMatched[bestIdx] = True
            written[-1] = bestIdx
            nmatches += 1
    return nmatches, written, vpMatched


def ref_search_by_projection_frame_kf(F, cam, points, has_point, orb_dist, check_orientation):
    """SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (:1385-1504).  points[i] = the keyframe's map
    point i: skip (NULL / isBad / in sAlreadyFound), pos, min/max_distance, desc, angle (pKF->mvKeysUn[i].angle).  has_point[i2]:
    CurrentFrame.mvpMapPoints[i2] != NULL on entry.  Returns (nmatches, point index per frame keypoint or -1, updated has_point)."""
    cam = _cam_f32(cam)
    mvp = [bool(m) for m in has_point]
    who = [-1] * F.N
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i, p in enumerate(points):
        if p["skip"]:
            continue
        xc3 = _gemm3(cam["R"], p["pos"], cam["t"])
        xc, yc = xc3[0], xc3[1]
        invzc = _f32(1.0 / float(xc3[2]))
        u = cam["fx"] * xc * invzc + cam["cx"]
        v = cam["fy"] * yc * invzc + cam["cy"]
        if u < cam["min_x"] or u > cam["max_x"]:
            continue
        if v < cam["min_y"] or v > cam["max_y"]:
            continue
        PO = [_f32(p["pos"][k]) - _f32(cam["Ow"][k]) for k in range(3)]
        dist3D = _norm3(PO)
        if dist3D < _f32(0.8) * _f32(p["min_distance"]) or dist3D > _f32(1.2) * _f32(p["max_distance"]):
            continue
        lvl = predict_scale(p["max_distance"], dist3D, cam["log_scale_factor"], cam["n_levels"])
        radius = cam["th"] * _f32(cam["scale_factors"][lvl])
        vIndices2 = F.GetFeaturesInArea(u, v, radius, lvl - 1, lvl + 1)
        if not vIndices2:
            continue
        bestDist, bestIdx2 = 256, -1
        for i2 in vIndices2:
            if mvp[i2]:
                continue
            dist = descriptor_distance(p["desc"], F.desc[i2])
            if dist < bestDist:
                bestDist, bestIdx2 = dist, i2
        if bestDist <= orb_dist:
            mvp[bestIdx2] = True
            who[bestIdx2] = i
            nmatches += 1
            if check_orientation:
                rotHist[_rot_bin(p["angle"], F.angle[bestIdx2])].append(bestIdx2)
    if check_orientation:
        ind = compute_three_maxima([len(h) for h in rotHist])
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for j in rotHist[b]:
                mvp[j] = False
                who[j] = -1
                nmatches -= 1
    return nmatches, who, mvp


# ------------------------------------------------------------------------------------------------------------------------------
# Second reading of Frame::ComputeBoW's work: DBoW2 TemplatedVocabulary::transform (ThirdParty/DBoW2/DBoW2-local/include/DBoW2/
# TemplatedVocabulary.h:1125-1192 and :1216-1257) on a tree as ORBVocabulary::loadFromTextFile builds it (ORBVocabulary.cc:79-123:
# node ids in file order, children appended in that order, word ids numbering the nodes flagged leaf in that order).
def ref_vocab_transform(L, parent, leaf_flag, node_desc, node_weight, features, levelsup, scoring=0, weighting=0):
    """Returns (BowVector as {word id: value}, FeatureVector as {node id: [feature indices]}).  scoring: 0 L1, 1 L2, 2 chi-square,
    3 KL, 4 Bhattacharyya, 5 dot product (ScoringObject.h:73-88); weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY."""
    n = len(parent)
    children = [[] for _ in range(n)]
    word_id = [-1] * n
    n_words = 0
    for nid in range(1, n):
        children[int(parent[nid])].append(nid)
        if leaf_flag[nid]:
            word_id[nid] = n_words
            n_words += 1
    bow, fv = {}, {}
    if n <= 1:                                       # empty(): no words
        return bow, fv
    for i_feature, f in enumerate(features):
        nid_level = L - levelsup
        nid = 0   # root when nid_level <= 0 (:1225); ALSO when the descent ends above nid_level: the reference then reads an
                  # uninitialised NodeId (:1149, :1249 never reached) -- undefined there, defined as the root here and in the oracle
        final_id, current_level = 0, 0
        while True:
            current_level += 1
            nodes = children[final_id]
            final_id = nodes[0]
            best_d = float(descriptor_distance(f, node_desc[final_id]))
            for c in nodes[1:]:
                d = float(descriptor_distance(f, node_desc[c]))
                if d < best_d:
                    best_d, final_id = d, c
            if current_level == nid_level:
                nid = final_id
            if not children[final_id]:               # Node::isLeaf() = children.empty()
                break
        w = float(node_weight[final_id])
        if w > 0:
            wid = word_id[final_id]
            if weighting in (0, 1):
                bow[wid] = bow.get(wid, 0.0) + w     # addWeight
            elif wid not in bow:
                bow[wid] = w                         # addIfNotExist
            fv.setdefault(nid, []).append(i_feature)
    must = scoring != 5
    if weighting in (0, 1) and bow and not must:
        nd = float(len(bow))
        for k in bow:
            bow[k] /= nd
    if must:
        keys = sorted(bow)
        norm = 0.0
        if scoring == 1:
            for k in keys:
                norm += bow[k] * bow[k]
            norm = math.sqrt(norm)
        else:
            for k in keys:
                norm += abs(bow[k])
        if norm > 0.0:
            for k in keys:
                bow[k] /= norm
    return bow, fv
