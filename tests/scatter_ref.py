"""NumPy references of the two scatters into the FPN gradient maps -- the RoIAlign backward (csrc/train_bwd.hip: roi_align_bwd_kernel,
roi_bwd_meta_kernel, roi_align_bwd_tile_kernel), written from the torchvision definition of the forward and the summation order the comments
of the tile kernel document, and the sparse backward pass of the RPN head (csrc/rpn_sparse.hip, second half of this file) -- and the case
tables tests/test_scatter_ref.py (CPU), tests/test_roi_bwd_exact_gpu.py and tests/test_rpn_sparse_exact_gpu.py (the kernels) share.  Nothing
here imports oracle/.

Every fp32 step is one np.float32 operation (numpy never fuses a product into a sum), so roi_align_bwd_ref compares bit for bit with the
owner-computes kernel.  Two operand classes:
  NARROW  RoI sides of P * d * stride with d dyadic and ceil(d) in {1, 2, 4}, dyadic starts, gradients and preset maps of small integers
          times a power of two: every weight, 1 / (gh * gw), every product and every partial sum in every order is exact, so the result is
          the float64 sum whatever the order (the atomic kernel included); narrow_premise() asserts this from the inputs.
  WIDE    seeded RoIs (grids of 3 and 5 samples: 1 / 9, 1 / 15, 1 / 25 round), randn gradients and maps: the order of the sum shows.

Seeded defects (ROI_DEFECTS) restate the mistakes this code can make; tests/test_scatter_ref.py shows which case family catches which."""
import numpy as np

import proposal_ref as PR

F32 = np.float32
STRIDES = PR.STRIDES
TILE = 4
ROI_DEFECTS = ("drop_top_clamp", "skip_upper_tap", "reverse_roi_order", "footprint_minus_one", "first_64_rois_only", "bins_capped_at_14")


# ------------------------------------------------------------------------------------------------------------------ RoIAlign backward
def axis_weights(v, size, defect=None):
    """Separable tap weights of one axis: v [P, g] float32 sample coordinates -> W [P, size] float32, W[p, y] = the running fp32 sum over the
    bin's samples in order of h = 1 - l where the sample's lower tap is y, then l where its upper tap is y (edge rules of the forward:
    proposal_ref._edge_rules)."""
    P, g = v.shape
    bad, lo, hi, l, h = PR._edge_rules(v, size)
    if defect == "drop_top_clamp":        # the sample above the last row keeps its fraction and its upper tap falls off the map
        v0 = np.where(v <= 0, F32(0), v)
        top = ~bad & (v0 >= F32(size - 1))
        l0 = (v0 - F32(size - 1)).astype(F32)
        h = np.where(top, (F32(1) - l0).astype(F32), h)
        l = np.where(top, F32(0), l)
    W = np.zeros((P, size), F32)
    p = np.arange(P)
    for i in range(g):
        ok = ~bad[:, i]
        W[p[ok], lo[ok, i]] = W[p[ok], lo[ok, i]] + h[ok, i]
        if defect != "skip_upper_tap":
            W[p[ok], hi[ok, i]] = W[p[ok], hi[ok, i]] + l[ok, i]
    assert W.dtype == F32
    return W


def _roi_weights(roi, P, lv, H, W, defect):
    """(WY [P, H], WX [P, W], inv) of one RoI, or None for an empty sampling grid / a RoI without extent (NaN included)."""
    if not np.isfinite(np.asarray(roi, F32)).all():          # ceil(NaN) as an int is 0 on the device: an empty grid
        return None
    ys, xs = PR.roi_samples(roi, P, STRIDES[lv], H, W)
    if ys is None:
        return None
    gh, gw = ys.shape[1], xs.shape[1]
    WY, WX = axis_weights(ys, H, defect), axis_weights(xs, W, defect)
    if defect == "footprint_minus_one":   # the tile that holds only the footprint's last row / column as its first skips the RoI
        for Wt in (WY, WX):
            nz = np.flatnonzero((Wt != 0).any(0))
            if nz.size and nz[-1] % TILE == 0:
                Wt[:, nz[-1]] = 0
    if defect == "bins_capped_at_14":
        WY[14:] = 0
        WX[14:] = 0
    return WY, WX, F32(1) / F32(gh * gw)


def _roi_order(batch_idx, R, defect):
    order = list(range(R))
    if defect == "reverse_roi_order":
        order.reverse()
    if defect == "first_64_rois_only":    # one ballot trip: only the 64 RoI slots from the first RoI of an image on are looked at
        first = {}
        for r in range(R):
            first.setdefault(int(batch_idx[r]), r)
        order = [r for r in order if r < first[int(batch_idx[r])] + 64]
    return order


def _span(nz):
    """slice of the first .. last True"""
    i = np.flatnonzero(nz)
    return slice(int(i[0]), int(i[-1]) + 1) if i.size else None


def roi_align_bwd_ref(maps, rois, batch_idx, P, levels, dout, init=False, defect=None):
    """The specification of roi_align_bwd_tile_kernel.  maps = [p2..p5] NHWC float32 (preset; returned updated, the inputs untouched), rois
    [R, 4], batch_idx [R] (None: image 0), levels [R] (proposal_ref.level_ref), dout [R, P, P, C].
    Every cell starts an accumulator at +0 and adds, over the RoIs of its image and level in ascending index, then ph, then pw,
    fl(fl(wy * wx) * fl(g * inv)), inv = fl(1 / (gh * gw)); terms of zero weight are left out (they cannot change the bits of an accumulator
    that starts at +0).  The map becomes fl(map + acc) in every cell of every 4 x 4 tile any RoI contributes to -- which turns a stored -0.0
    of such a tile into +0.0 and leaves the other tiles' bits alone -- and fl(0 + acc) everywhere with `init`."""
    rois = np.asarray(rois, F32).reshape(-1, 4)
    R = len(rois)
    bi = np.zeros(R, np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    acc = [np.zeros(m.shape, F32) for m in maps]
    touched = [np.zeros(m.shape[:3], bool) for m in maps]
    for r in _roi_order(bi, R, defect):
        lv, b = int(levels[r]), int(bi[r])
        Bn, H, W, C = maps[lv].shape
        if not 0 <= b < Bn:
            continue
        wts = _roi_weights(rois[r], P, lv, H, W, defect)
        if wts is None:
            continue
        WY, WX, inv = wts
        gi = (np.asarray(dout[r], F32) * inv).astype(F32)                     # [P, P, C]
        rowt, colt = (WY != 0).any(0), (WX != 0).any(0)
        if not (rowt.any() and colt.any()):
            continue
        # tiles with a non-zero row weight and a non-zero column weight of some bin
        tr = np.repeat(np.logical_or.reduceat(rowt, np.arange(0, H, TILE)), TILE)[:H]
        tc = np.repeat(np.logical_or.reduceat(colt, np.arange(0, W, TILE)), TILE)[:W]
        touched[lv][b] |= tr[:, None] & tc[None, :]
        for ph in range(P):
            ry = _span(WY[ph] != 0)
            if ry is None:
                continue
            for pw in range(P):
                rx = _span(WX[pw] != 0)
                if rx is None:
                    continue
                w = (WY[ph, ry, None] * WX[pw, None, rx]).astype(F32)
                a = acc[lv][b, ry, rx]
                acc[lv][b, ry, rx] = a + w[:, :, None] * gi[ph, pw][None, None, :]
    out = []
    for m, a, t in zip(maps, acc, touched):
        m = np.asarray(m, F32)
        assert a.dtype == F32
        out.append((F32(0) + a).astype(F32) if init else np.where(t[..., None], (m + a).astype(F32), m))
    return out


def roi_align_bwd_sum64(shapes, rois, batch_idx, P, levels, dout):
    """The same sum in float64 over the same fp32 weights and fp32 inv (products and sums in float64: the only fp32 roundings a kernel adds are
    its three per term and those of its additions).  shapes = [(B, H, W, C)] * 4.  Returns per level (sum [B, H, W, C], sum |terms|
    [B, H, W, C], terms [B, H, W]): one term per (RoI, ph, pw) of non-zero weight."""
    rois = np.asarray(rois, F32).reshape(-1, 4)
    R = len(rois)
    bi = np.zeros(R, np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    s = [np.zeros(sh, np.float64) for sh in shapes]
    sa = [np.zeros(sh, np.float64) for sh in shapes]
    cnt = [np.zeros(sh[:3], np.int64) for sh in shapes]
    for r in range(R):
        lv, b = int(levels[r]), int(bi[r])
        Bn, H, W, C = shapes[lv]
        if not 0 <= b < Bn:
            continue
        wts = _roi_weights(rois[r], P, lv, H, W, None)
        if wts is None:
            continue
        WY, WX, inv = wts
        gi = np.asarray(dout[r], F32).astype(np.float64) * np.float64(inv)
        WY, WX = WY.astype(np.float64), WX.astype(np.float64)
        for ph in range(P):
            ry = _span(WY[ph] != 0)
            if ry is None:
                continue
            for pw in range(P):
                rx = _span(WX[pw] != 0)
                if rx is None:
                    continue
                w = WY[ph, ry, None] * WX[pw, None, rx]
                t = w[:, :, None] * gi[ph, pw][None, None, :]
                s[lv][b, ry, rx] += t
                sa[lv][b, ry, rx] += np.abs(t)
                cnt[lv][b, ry, rx] += (w != 0)
    return list(zip(s, sa, cnt))


def pow2_unit(x):
    """the largest power of two every entry of x is an integer multiple of (x finite; 1.0 for an all-zero x)"""
    x = np.asarray(x, np.float64).reshape(-1)
    x = x[x != 0]
    if x.size == 0:
        return 1.0
    for k in range(40, -80, -1):
        if np.all(np.mod(x, 2.0 ** k) == 0):
            return 2.0 ** k
    raise AssertionError("not dyadic")


def narrow_premise(maps, rois, batch_idx, P, levels, dout):
    """Asserts from the inputs that a case is NARROW: every gh * gw a power of two, and per output cell sum |terms| + |preset| < 2^24 units, the
    unit being the product of the units of the row weights, the column weights and g * inv -- so every partial sum in every order is an
    integer number of units below 2^24: exact in fp32.  Returns the float64 result (maps + sums)."""
    rois = np.asarray(rois, F32).reshape(-1, 4)
    bi = np.zeros(len(rois), np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    uw, ug = [], []
    for r in range(len(rois)):
        lv = int(levels[r])
        _, H, W, _ = maps[lv].shape
        wts = _roi_weights(rois[r], P, lv, H, W, None)
        if wts is None:
            continue
        WY, WX, inv = wts
        n = int(round(1.0 / float(inv)))
        assert n & (n - 1) == 0 and F32(1) / inv == F32(n), ("gh * gw is no power of two", r, n)
        uw.append(pow2_unit(WY) * pow2_unit(WX))
        ug.append(pow2_unit(np.asarray(dout[r], np.float64) * float(inv)))
    unit = (min(uw) * min(ug)) if uw else 1.0
    sums = roi_align_bwd_sum64([m.shape for m in maps], rois, bi, P, levels, dout)
    out = []
    for m, (s, sa, _) in zip(maps, sums):
        m64 = np.asarray(m, np.float64)
        assert pow2_unit(m64) >= unit or not uw, "preset map finer than the terms' unit"
        assert float((sa + np.abs(m64)).max(initial=0.0)) < 2.0 ** 24 * unit, ("sum |terms| reaches 2^24 units", float(sa.max()), unit)
        out.append(m64 + s)
    return out


# ------------------------------------------------------------------------------------------------------------------ case tables
def narrow_roi(lv, y0, x0, dy, dx, P):
    """RoI at level lv whose first sample row starts y0 cells into the map (x likewise) with bins of dy x dx cells: in px,
    [(x0 + 0.5) * stride, ...] so that roi * (1 / stride) - 0.5 = x0 exactly."""
    s = STRIDES[lv]
    return [(x0 + 0.5) * s, (y0 + 0.5) * s, (x0 + 0.5 + P * dx) * s, (y0 + 0.5 + P * dy) * s]


def assert_levels(rois, want=None):
    """every case asserts `decided` for each RoI (and the level it was built for)"""
    lv, decided = PR.level_ref(rois)
    assert decided.all(), np.flatnonzero(~decided)
    if want is not None:
        assert (lv == np.asarray(want)).all(), (lv.tolist(), want)
    return lv


EMPTY_ROIS = np.asarray([[-300, -200, -100, -50], [400, 300, 520, 420], [30, 40, 30, 90], [30, 40, 90, 40], [50, 20, 30, 60], [90, 80, 40, 20],
                         [10, np.nan, 60, 70]], F32)          # wholly outside (2), zero area (2), inverted (2), a NaN coordinate
EMPTY_IDS = ("outside-above-left", "outside-below-right", "zero-width", "zero-height", "x2-below-x1", "both-inverted", "nan-y1")

MAP_SETS = {"edge": PR.MAP_HW, "ragged": ((9, 11), (5, 6), (3, 3), (1, 2)), "multiples": ((8, 4), (4, 8), (4, 4), (1, 1))}


def ints(rng, lo, hi, shape, unit=1.0):
    """small integers times a power of two"""
    return (rng.integers(lo, hi + 1, shape) * unit).astype(F32)


def fit_level(roi_cells, lv, P):
    """(y0, x0, dy, dx) in cells at level lv -> the RoI in px, with its level asserted"""
    r = np.asarray([narrow_roi(lv, *roi_cells, P)], F32)
    assert_levels(r, [lv])
    return r[0]


def narrow_map_rois(hw, P, B=2):
    """NARROW RoIs for maps of sizes hw at P: per level bins of (1, 1), (0.5, 2), (4, 0.25 ...) cells where sqrt(area) stays inside the level,
    starting at dyadic offsets that put samples before the first cell, across tile borders and beyond the last cell.  The level rule limits
    the sides: P * sqrt(dy * dx) cells * stride must lie in the level's px range; candidates outside it are dropped (and at least two per
    level must remain)."""
    rois, lvs = [], []
    bins = ((1, 1), (0.5, 2), (2, 0.5), (1.5, 0.75), (0.75, 1.5), (4, 0.25), (0.25, 4), (0.5, 0.5), (2, 2), (3.5, 1), (1, 3.5), (4, 4), (0.25, 0.25),
            (1, 0.5), (0.5, 1), (2, 1), (1, 2), (2, 4), (4, 2), (3.5, 3.5), (4, 1.5), (1.5, 4), (2, 3.5), (3.5, 2), (4, 3.5), (1.5, 1.5))
    assert all(int(np.ceil(d)) in (1, 2, 4) for b in bins for d in b)
    for lv, (H, W) in enumerate(hw):
        kept = 0
        for k, (dy, dx) in enumerate(bins):
            for (fy, fx) in ((-0.75, 0.25), (0.5, -1.5), (H - 0.5 * P * dy, W - 0.75 * P * dx), (H - P * dy + 0.5, -0.25), (0.0, 0.0)):
                y0, x0 = np.floor(fy * 4) / 4, np.floor(fx * 4) / 4
                r = np.asarray([narrow_roi(lv, y0, x0, dy, dx, P)], F32)
                l, dec = PR.level_ref(r)
                if dec[0] and l[0] == lv:
                    rois.append(r[0]); lvs.append(lv); kept += 1
        assert kept >= 2 or (P == 1 and lv > 0), (lv, hw, P)          # (at P = 1 no bin of <= 4 cells is large enough for p3..p5)
    rois = np.asarray(rois, F32)
    return rois, (np.arange(len(rois)) % B).astype(np.int32), np.asarray(lvs)


def _case(name, cls, hw, rois, bidx, P, B=2, C=256, seed=1, **kw):
    """One RoIAlign-backward case: operands of its class drawn here (dout and the preset maps), levels from level_ref with `decided` asserted."""
    rois = np.asarray(rois, F32).reshape(-1, 4)
    lv = assert_levels(rois, kw.pop("levels", None)) if len(rois) else np.zeros(0, np.int64)
    rng = np.random.default_rng(seed)
    R = len(rois)
    if cls == "narrow":
        dout = ints(rng, -3, 3, (R, P, P, C), 0.25)
        maps = [ints(rng, -5, 5, (B, h, w, C)) for h, w in hw]
    else:
        dout = rng.standard_normal((R, P, P, C), dtype=F32)
        maps = [rng.standard_normal((B, h, w, C), dtype=F32) for h, w in hw]
    return dict(name=name, cls=cls, hw=tuple(hw), rois=rois, bidx=None if bidx is None else np.asarray(bidx, np.int32), P=P, B=B, C=C, levels=lv,
                dout=dout, maps=maps, **kw)


def _tile_rois():
    """NARROW p2 RoIs of 7 bins of 0.25 cells (1.75 cells a side) placed against the 4 x 4 tiles of the p2 map: (name, y0, x0)."""
    out = [("straddles-corner", 2.5, 2.5),
           ("last-row-is-tile-first", 6.0, 1.0), ("last-col-is-tile-first", 1.0, 6.0),             # samples 6.125 .. 7.625: rows 6, 7, 8
           ("last-row-on-tile-first-exactly", 6.375, 9.0), ("last-col-on-tile-first-exactly", 9.0, 6.375),      # last sample on 8.0: row 8 weight 1, row 9 none
           ("first-row-is-tile-last", 3.25, 13.0), ("first-col-is-tile-last", 13.0, 3.25),         # rows 3, 4, 5
           ("both-ends", 3.25 + 16, 3.25 + 16)]
    return out


def roi_cases():
    """name -> case, every family of tests/test_roi_bwd_exact_gpu.py (built on call; a few MB)."""
    cs = []
    HW = PR.MAP_HW
    # -- the edge table of the forward at P = 7, with the empty RoIs among it
    rois = np.concatenate([PR.ROI_EDGE, EMPTY_ROIS])
    cs.append(_case("edge-p7", "wide", HW, rois, np.arange(len(rois)) % 2, 7, seed=11))
    cs.append(_case("empty-only", "wide", HW, EMPTY_ROIS, np.arange(len(EMPTY_ROIS)) % 2, 7, seed=12, unchanged=True))
    # -- map sizes round the tile
    for tag in ("ragged", "multiples"):
        r, b, l = narrow_map_rois(MAP_SETS[tag], 7)
        cs.append(_case("maps-%s-p7" % tag, "narrow", MAP_SETS[tag], r, b, 7, seed=13, levels=l))
        r, b, l = narrow_map_rois(MAP_SETS[tag], 14)
        cs.append(_case("maps-%s-p14" % tag, "narrow", MAP_SETS[tag], r[::3], b[::3], 14, seed=14, levels=l[::3]))
        wr, wb = PR.seeded_rois(40, 21)
        cs.append(_case("maps-%s-wide" % tag, "wide", MAP_SETS[tag], wr * F32(0.25), wb, 7, seed=15))
    # -- tile ownership
    t = _tile_rois()
    r = [narrow_roi(0, y, x, 0.25, 0.25, 7) for _, y, x in t]
    cs.append(_case("tile-ownership", "narrow", HW, r, np.arange(len(r)) % 2, 7, seed=16, levels=[0] * len(r), tile_names=[n for n, _, _ in t]))
    r = [narrow_roi(3, -4, -4, 16, 16, 1), narrow_roi(3, -5, -5, 16, 16, 1)]
    cs.append(_case("whole-p5-one-bin", "narrow", HW, r, [0, 1], 1, seed=17, levels=[3, 3]))
    r = [narrow_roi(3, -2, -2, 8, 8, 7), narrow_roi(3, -2.5, -1.25, 8, 8, 7)]
    cs.append(_case("whole-p5-bins-of-8", "narrow", HW, r, [0, 1], 7, seed=18, levels=[3, 3]))
    # -- bin slots: a RoI of under one cell inside one tile
    for P in (14, 15, 16, 17):
        d = 1.0 / 32 if P >= 16 else 1.0 / 16
        r = [narrow_roi(0, 5.25, 9.25, d, d, P), narrow_roi(0, 13.0, 4.5, d, d, P)]
        for cls in ("narrow", "wide"):
            cs.append(_case("bin-slots-p%d-%s" % (P, cls), cls, HW, r, [0, 1], P, seed=19, levels=[0, 0], one_tile=True))
    r, b, l = narrow_map_rois(HW, 1)
    cs.append(_case("p1", "narrow", HW, r, b, 1, seed=20, levels=l))
    wr, wb = PR.seeded_rois(40, 22, max_side=100.0)
    cs.append(_case("p1-wide", "wide", HW, wr, wb, 1, seed=20))
    # -- the RoI loop
    img = np.ones(135, np.int32)
    img[[0, 40, 70, 100, 134]] = 0                           # 5 RoIs of image 0 among the 130 of image 1: its range spans them, three ballot trips
    r = [narrow_roi(0, 8.25 + 0.25 * (i % 5), 12.0 + 0.25 * (i % 4), 0.25, 0.25, 7) for i in range(135)]     # rows 8 .. 11, columns 12 .. 15: one tile
    for cls in ("narrow", "wide"):
        cs.append(_case("130-rois-one-tile-%s" % cls, cls, HW, r, img, 7, seed=23, levels=[0] * 135, many=True))
    r, b, l = narrow_map_rois(MAP_SETS["ragged"], 7)
    cs.append(_case("image-without-rois", "narrow", MAP_SETS["ragged"], r[::4], 2 * (np.arange(len(r[::4])) % 2), 7, B=3, seed=24, levels=l[::4]))
    cs.append(_case("batch-idx-none", "narrow", MAP_SETS["ragged"], r[1::4], None, 7, B=1, seed=25, levels=l[1::4]))
    wr, wb = PR.seeded_rois(60, 26)
    cs.append(_case("wide-p7", "wide", HW, wr, wb, 7, seed=27, derive_B=True))
    cs.append(_case("wide-p14", "wide", HW, wr[:30], wb[:30], 14, seed=28))
    cs.append(_case("same-box-100", "wide", HW, np.repeat(wr[3:4], 100, 0), np.zeros(100, np.int32), 7, seed=29, same_box=True))
    # -- other widths (atomic kernel only)
    r, b, l = narrow_map_rois(MAP_SETS["ragged"], 7)
    for C in (4, 64, 320):
        cs.append(_case("c%d" % C, "narrow", MAP_SETS["ragged"], r[::2], b[::2], 7, C=C, seed=30, levels=l[::2]))
    # -- more than 64 rows / columns under one bin: the atomic kernel's tap-by-tap branch
    for ax in ("y", "x"):
        hw = ((70, 3), (1, 1), (1, 1), (1, 1)) if ax == "y" else ((3, 70), (1, 1), (1, 1), (1, 1))
        tall = lambda y0, x0, n: narrow_roi(0, y0, x0, n, 1, 1) if ax == "y" else narrow_roi(0, x0, y0, 1, n, 1)
        # 128 cells under the one bin (gh = 128: inv exact), and the 280-px side of 70 cells (inv = 1 / 70 rounds; samples one cell apart)
        cs.append(_case("taps-128-%s" % ax, "narrow", hw, [tall(-1.75, 0.25, 128), tall(-40.0, 1.0, 128)], [0, 1], 1, C=64, seed=31, levels=[0, 0], taps=True))
        cs.append(_case("taps-280px-%s" % ax, "wide", hw, [tall(0.25, 0.25, 70), tall(-0.5, 1.5, 70)], [0, 1], 1, C=64, seed=32, levels=[0, 0], taps=True))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in cs}


# ------------------------------------------------------------------------------------------------------------------ sparse RPN backward
# csrc/rpn_sparse.hip, from the formulas at its top, computed densely in float64 over whole (tiny) maps:
#   d_t = (t > 0) * (d_pred . W_pred) per pixel;  dW_pred = d_pred^T . t;  db_pred = colsum(d_pred);  db_conv = colsum(d_t)
#   dW_conv = scale[n] * the 3 x 3 pad-1 weight gradient of (d_t, feat);  d_feat += the transposed convolution of d_t with scale[n] * W_conv
F64 = np.float64
NOROW = 0xffffffff
SPARSE_LEVELS = ((6, 7), (3, 4), (2, 2), (1, 1), (1, 1))
SPARSE_DEFECTS = ("border_tap_wraps", "duplicate_pixel_twice", "relu_mask_ignored", "last_row_dropped")
HID = 256
SUM_SLICES = 32


def rpn_ld(A):
    return 16 if 5 * A <= 16 else 32 if 5 * A <= 32 else 48


def anchor_offsets(levels, A):
    return np.concatenate([[0], np.cumsum([h * w * A for h, w in levels])]).astype(np.int64)


def rpn_rows_ref(levels, A, sampled, counts, batch, dedup=True):
    """rows [B * batch] uint32 and nrows [B]: per image the sorted unique (level << 26 | pixel) keys of the first min(pos + neg, batch) sampled
    anchors that are valid (0 <= index < the anchor total), NOROW beyond the count."""
    off = anchor_offsets(levels, A)
    B = len(counts)
    rows = np.full((B, batch), NOROW, np.uint32)
    nrows = np.zeros(B, np.int32)
    for b in range(B):
        n = min(int(counts[b][0]) + int(counts[b][1]), batch)
        an = np.asarray(sampled[b][:n], np.int64)
        an = an[(an >= 0) & (an < off[-1])]
        lvl = np.searchsorted(off[1:], an, side="right")
        keys = (lvl << 26) | ((an - off[lvl]) // A)
        keys = np.unique(keys) if dedup else np.sort(keys)
        rows[b, :len(keys)] = keys
        nrows[b] = len(keys)
    return rows.reshape(-1), nrows


def _taps(h, w, wrap=False):
    """per tap (ky, kx): (p, q) index arrays, q = p + (ky - 1, kx - 1) inside the map; wrap: only the flat index is checked (the seeded defect)"""
    y, x = np.divmod(np.arange(h * w), w)
    out = []
    for ky in range(3):
        for kx in range(3):
            yy, xx = y + ky - 1, x + kx - 1
            if wrap:
                q = yy * w + xx
                ok = (q >= 0) & (q < h * w)
            else:
                q = yy * w + xx
                ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            out.append((np.flatnonzero(ok), q[ok]))
    return out


def exact_sum_premise(a, b, axis_note):
    """sum |a||b| over the reduction < 2^24 units (unit = the product of the operands' power-of-two units): every partial sum in any order is an
    fp32 value.  a [M, I], b [M, J] reduce over M."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    unit = pow2_unit(a) * pow2_unit(b)
    worst = float((np.abs(a).T @ np.abs(b)).max(initial=0.0))
    assert worst < 2.0 ** 24 * unit, (axis_note, worst / unit)


def rpn_sparse_ref(levels, A, K, batch, sampled, counts, dpred, t, feat, w_pred, w_conv, scale, shift, dfeat, recompute_t=False, defect=None, premise=False):
    """Dense float64 reference.  dpred[l] [B, hw, ld], t[l] [B, hw, 256] (values; ignored with recompute_t), feat[l] [B, hw, 256] (values),
    w_pred [K, 256], w_conv [256, 3, 3, 256], scale / shift [256] or None, dfeat[l] [B, hw, 256] presets.  premise: assert the NARROW class
    (every reduction below 2^24 units).  Returns dict(rows, nrows, gw_pred, gb_pred, gw_conv, gb_conv, dfeat, t, dt)."""
    B = len(counts)
    rows, nrows = rpn_rows_ref(levels, A, sampled, counts, batch)
    sc = np.ones(HID, F64) if scale is None else np.asarray(scale, F64)
    wp, wc = np.asarray(w_pred, F64), np.asarray(w_conv, F64)
    mult = [np.ones((B, h * w)) for h, w in levels]
    if defect == "duplicate_pixel_twice":           # no duplicate removal: a pixel counts once per sampled anchor
        dup, _ = rpn_rows_ref(levels, A, sampled, counts, batch, dedup=False)
        for b in range(B):
            for key in dup.reshape(B, batch)[b]:
                if key != NOROW:
                    mult[key >> 26][b, key & 0x3ffffff] += 1
        mult = [np.maximum(m - 1, 1) for m in mult]
    if defect == "last_row_dropped":
        b = int(np.flatnonzero(nrows)[-1])
        key = int(rows.reshape(B, batch)[b, nrows[b] - 1])
        mult[key >> 26][b, key & 0x3ffffff] = 0
    out = dict(rows=rows, nrows=nrows, gw_pred=np.zeros((K, HID)), gb_pred=np.zeros(K), gw_conv=np.zeros((HID, 3, 3, HID)), gb_conv=np.zeros(HID),
               dfeat=[], t=[], dt=[])
    dp_all, t_all, dt_all = [], [], []
    sa_gw = np.zeros((HID, 9, HID))
    for l, (h, w) in enumerate(levels):
        x = np.asarray(feat[l], F64)
        taps = _taps(h, w, defect == "border_tap_wraps")
        if recompute_t:
            s = np.zeros((B, h * w, HID))
            for k, (p, q) in enumerate(taps):
                s[:, p] += x[:, q] @ wc[:, k // 3, k % 3].T
            T = np.maximum(s * sc + (0.0 if shift is None else np.asarray(shift, F64)), 0.0)
        else:
            T = np.asarray(t[l], F64)
        dp = np.asarray(dpred[l], F64)[..., :K] * mult[l][..., None]
        v = dp @ wp
        dt = v if defect == "relu_mask_ignored" else np.where(T > 0, v, 0.0)
        out["gw_pred"] += np.einsum("bpk,bpc->kc", dp, T)
        out["gb_pred"] += dp.sum((0, 1))
        out["gb_conv"] += dt.sum((0, 1))
        d = np.asarray(dfeat[l], F64).copy()
        for k, (p, q) in enumerate(taps):
            out["gw_conv"][:, k // 3, k % 3] += np.einsum("bpn,bpc->nc", dt[:, p], x[:, q])
            d[:, q] += dt[:, p] @ (wc[:, k // 3, k % 3] * sc[:, None])
        out["dfeat"].append(d)
        out["t"].append(T)
        out["dt"].append(dt)
        dp_all.append(dp.reshape(-1, K)); t_all.append(T.reshape(-1, HID)); dt_all.append(dt.reshape(-1, HID))
        if premise:         # sum |a||b| of the two GEMM-shaped reductions: over every row (dW_conv), over the 2304 patch entries (the recomputed t)
            for k, (p, q) in enumerate(taps):
                sa_gw[:, k] += np.einsum("bpn,bpc->nc", np.abs(dt[:, p]), np.abs(x[:, q]))
            if recompute_t:
                sa = np.zeros((B, h * w, HID))
                for k, (p, q) in enumerate(taps):
                    sa[:, p] += np.abs(x[:, q]) @ np.abs(wc[:, k // 3, k % 3]).T
                assert float(sa.max()) < 2.0 ** 24 * pow2_unit(x) * pow2_unit(wc), ("recomputed t", float(sa.max()))
    out["gw_conv"] = (out["gw_conv"] + 0.0) * sc[:, None, None, None]          # the accumulators start at +0; scale[n] * (+0) keeps the sign of scale
    if premise:
        dp, T, dt = np.concatenate(dp_all), np.concatenate(t_all), np.concatenate(dt_all)
        ux = min(pow2_unit(np.asarray(f, F64)) for f in feat)
        assert float(sa_gw.max()) < 2.0 ** 24 * pow2_unit(dt) * ux, ("dW_conv", float(sa_gw.max()))
        exact_sum_premise(dp, T, "dW_pred")
        exact_sum_premise(dp, np.ones((len(dp), 1)), "db_pred")
        exact_sum_premise(dt, np.ones((len(dt), 1)), "db_conv")
        exact_sum_premise(wp, np.abs(dp).max(0)[:, None], "d_t")
        exact_sum_premise(np.abs(dt).max(0)[:, None], np.abs(wc * sc[:, None, None, None]).sum((1, 2)), "G")
        for name in ("gw_pred", "gb_pred", "gw_conv", "gb_conv"):
            assert np.array_equal(out[name].astype(F32).astype(F64), out[name]), name
        for d in out["dfeat"] + out["t"] + out["dt"]:
            assert np.array_equal(d.astype(F32).astype(F64), d)
    return out


def rpn_gather_rows_ref(levels, rows, batch, dpred, t, K):
    """(dpred_rows [R, ld], act_rows [R, 256]) as rpn_dt_rows_kernel stores them: the rows' predictor gradients (columns < K; zero beyond and in
    unused rows) and hidden activations"""
    R, ld = len(rows), dpred[0].shape[-1]
    dr, ar = np.zeros((R, ld), F32), np.zeros((R, HID), F32)
    for r, key in enumerate(rows):
        if key != NOROW:
            b, l, p = r // batch, int(key >> 26), int(key & 0x3ffffff)
            dr[r, :K] = dpred[l][b, p, :K]
            ar[r] = t[l][b, p]
    return dr, ar


def rpn_gather_x_ref(levels, rows, batch, feat):
    """xg [R, 9, 256]: the 3 x 3 patch of the feature under each row's pixel, zero outside the map and in unused rows"""
    xg = np.zeros((len(rows), 9, HID), F32)
    for r, key in enumerate(rows):
        if key != NOROW:
            b, l, p = r // batch, int(key >> 26), int(key & 0x3ffffff)
            h, w = levels[l]
            for k in range(9):
                y, x = p // w + k // 3 - 1, p % w + k % 3 - 1
                if 0 <= y < h and 0 <= x < w:
                    xg[r, k] = feat[l][b, y * w + x]
    return xg


def rpn_dt_rows_ref(dpred_rows, act_rows, w_pred, K):
    """rpn_dt_rows_kernel in fp32: v = sum over k ascending of d_pred[k] * W_pred[k][c], each product and sum rounded on its own; d_t = act > 0 ? v : 0"""
    dr, w = np.asarray(dpred_rows, F32), np.asarray(w_pred, F32)
    v = np.zeros((len(dr), HID), F32)
    for k in range(K):
        v = v + dr[:, k, None] * w[k][None, :]
    assert v.dtype == F32
    return np.where(np.asarray(act_rows, F32) > 0, v, F32(0))


def rpn_head_sums_ref(dpred_rows, act_rows, dt_rows, K):
    """rpn_head_sums_kernel + rpn_head_sums_final_kernel in fp32: 32 row slices [R s / 32, R (s + 1) / 32), rows ascending inside a slice (from +0),
    slices ascending (from the first slice's sum); every product and sum rounded on its own.  Returns (gw_pred [K, 256], gb_pred [K], gb_conv [256])."""
    dr, ar, dt = np.asarray(dpred_rows, F32), np.asarray(act_rows, F32), np.asarray(dt_rows, F32)
    R = len(dr)
    parts = []
    for s in range(SUM_SLICES):
        gw, gb, gc = np.zeros((K, HID), F32), np.zeros(K, F32), np.zeros(HID, F32)
        for r in range(R * s // SUM_SLICES, R * (s + 1) // SUM_SLICES):
            gw = gw + dr[r, :K, None] * ar[r][None, :]
            gb = gb + dr[r, :K]
            gc = gc + dt[r]
        parts.append((gw, gb, gc))
    tot = list(parts[0])
    for p in parts[1:]:
        tot = [a + b for a, b in zip(tot, p)]
    assert all(a.dtype == F32 for a in tot)
    return tuple(tot)


def _border_pixels(h, w):
    return [y * w + x for y in range(h) for x in range(w) if y in (0, h - 1) or x in (0, w - 1)]


def _sparse_case(name, A, B, batch, lists, counts=None, K=None, cls="narrow", scale=True, recompute=False, shift=False, wsplit=False, seed=0):
    """lists: per image the sampled anchor indices (the counted prefix; counts default to (1, len - 1)).  The slots behind the prefix hold valid
    anchors of OTHER pixels, which must be ignored.  d_pred is non-zero only at the rows' pixels, as the RPN losses leave it."""
    import gemm_exact_ref as G
    levels, ld = SPARSE_LEVELS, rpn_ld(A)
    K = ld if K is None else K
    rng = np.random.default_rng(1000 + seed)
    total = int(anchor_offsets(levels, A)[-1])
    sampled = rng.integers(0, total, (B, batch)).astype(np.int32)
    cnt = np.zeros((B, 2), np.int32)
    for b, lst in enumerate(lists):
        n = min(len(lst), batch)
        sampled[b, :n] = lst[:n]
        cnt[b] = (min(1, len(lst)), max(len(lst) - 1, 0)) if counts is None else counts[b]
    rows, nrows = rpn_rows_ref(levels, A, sampled, cnt, batch)
    hw = [h * w for h, w in levels]
    narrow = cls == "narrow"
    dpred = [np.zeros((B, n, ld), F32) for n in hw]
    for r, key in enumerate(rows):
        if key != NOROW:
            v = G.shifted(G.class_i(rng, K, zero=0.6), 16) if narrow else (rng.standard_normal(K) * 1e-3).astype(F32)
            dpred[int(key >> 26)][r // batch, int(key & 0x3ffffff), :K] = v
    for d in dpred:
        d[..., K:] = 1.0                                         # pad columns: never read
    t = []
    for n in hw:
        v = G.class_l_low(rng, (B, n, HID)) if narrow else rng.standard_normal((B, n, HID), dtype=F32)
        v = G.unsplit_rows_ref(G.split_rows_ref(v))              # (wide: the 22-bit values the split row format holds, so one t serves both formats)
        t.append(np.where(rng.random((B, n, HID)) < 0.25, F32(0), v).astype(F32))
    c = dict(name=name, cls=cls, A=A, B=B, batch=batch, K=K, ld=ld, levels=levels, sampled=sampled, counts=cnt, rows=rows, nrows=nrows,
             dpred=dpred, t=t, feat=[G.class_l_low(rng, (B, n, HID)) for n in hw],
             w_pred=G.class_l_int(rng, (K, HID)) if narrow else rng.standard_normal((K, HID), dtype=F32),
             w_conv=G.class_i(rng, (HID, 3, 3, HID), zero=0.85), scale=G.scales(rng, HID) if scale else None,
             shift=G.small_ints(rng, HID) if shift else None, dfeat=[G.small_ints(rng, (B, n, HID)) for n in hw],
             recompute=recompute, wsplit=wsplit)
    return c


def sparse_ref_of(c, defect=None, premise=None):
    return rpn_sparse_ref(c["levels"], c["A"], c["K"], c["batch"], c["sampled"], c["counts"], c["dpred"], c["t"], c["feat"], c["w_pred"], c["w_conv"],
                          c["scale"], c["shift"], c["dfeat"], recompute_t=c["recompute"], defect=defect,
                          premise=(c["cls"] == "narrow" and defect is None) if premise is None else premise)


def sparse_cases():
    """name -> case of tests/test_rpn_sparse_exact_gpu.py, on SPARSE_LEVELS (60 pixels an image)."""
    L = SPARSE_LEVELS
    cs = []

    def an(A, l, p, a=0):
        return int(anchor_offsets(L, A)[l]) + p * A + a

    cs.append(_sparse_case("one-pixel-all-anchors", 3, 1, 8, [[an(3, 0, 17, a) for a in range(3)]], seed=1))
    border = [an(3, l, p, i % 3) for l in range(5) for i, p in enumerate(_border_pixels(*L[l]))]
    cs.append(_sparse_case("borders-and-1x1-levels", 3, 1, 256, [border], seed=2))
    cs.append(_sparse_case("adjacent-pixels", 3, 1, 8, [[an(3, 0, 16), an(3, 0, 17, 2)]], seed=3))
    same = [an(3, 0, 2), an(3, 1, 2, 1), an(3, 2, 2, 2)]
    cs.append(_sparse_case("same-pixel-levels-images", 3, 3, 8, [same, [], same], seed=4))
    total = int(anchor_offsets(L, 3)[-1])
    inv = [-1, an(3, 0, 5), total, total + 5, an(3, 1, 11, 2), -1, an(3, 4, 0), an(3, 0, 41, 1), an(3, 0, 0), an(3, 0, 1), an(3, 0, 3)]
    cs.append(_sparse_case("invalid-entries-and-overfull", 3, 1, 8, [inv], counts=[(6, 5)], seed=5))
    cs.append(_sparse_case("batch-1", 3, 1, 1, [[an(3, 0, 0, 1)]], seed=6))
    cs.append(_sparse_case("batch-1-three-images", 3, 3, 1, [[an(3, 0, 41)], [an(3, 3, 0)], [an(3, 1, 5)]], seed=7))
    rng = np.random.default_rng(77)
    for name, A, B, batch, K, n in (("a5-batch-256", 5, 3, 256, 25, 40), ("a9-batch-512", 9, 3, 512, 48, 60), ("a9-k45-one-image", 9, 1, 256, 45, 30)):
        tot = int(anchor_offsets(L, A)[-1])
        cs.append(_sparse_case(name, A, B, batch, [rng.choice(tot, n, replace=False).tolist() for _ in range(B)], K=K, seed=8 + A + B))
    few = [an(3, 0, 0), an(3, 0, 6, 1), an(3, 0, 24, 2), an(3, 1, 5), an(3, 3, 0, 1)]
    cs.append(_sparse_case("no-scale", 3, 1, 8, [few], scale=False, seed=20))
    for i, (ws, sh) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        cs.append(_sparse_case("recompute%s%s" % ("-wsplit" if ws else "", "-shift" if sh else ""), 3, 1, 8, [few], recompute=True, wsplit=bool(ws),
                               shift=bool(sh), seed=21 + i))
    cs.append(_sparse_case("recompute-no-scale", 3, 1, 8, [few], recompute=True, scale=False, seed=26))
    cs.append(_sparse_case("wide-a3", 3, 3, 256, [rng.choice(180, 50, replace=False).tolist() for _ in range(3)], cls="wide", seed=30))
    cs.append(_sparse_case("wide-a9", 9, 1, 8, [rng.choice(540, 8, replace=False).tolist()], cls="wide", seed=31))
    return {c["name"]: c for c in cs}
