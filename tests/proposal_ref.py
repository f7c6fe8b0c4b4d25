"""NumPy references of proposal selection, NMS and the RoIAlign forward (csrc/rpn_select.hip, csrc/nms.hip, csrc/roi_align.hip), written
from the torchvision / detectron2 definitions and the operation order documented at the top of the three files and in
include/ampis_hip.h, and the case tables tests/test_proposal_ref.py (CPU, against the oracle) and tests/test_proposal_gpu.py (the
kernels) share.  Nothing here imports oracle/.

Every fp32 step is one np.float32 operation (numpy never fuses a product into a sum), so roi_align_ref, nms_ref, topk_ref, the split
row format and sortkey_ref compare bit for bit.  Two steps are not exactly reproducible and are treated as such: log2f of the level
rule (level_ref reports where a 1-ulp change of it changes the level) and expf of the decode (decode_ref is float64 and reports every
box's margin to the validity decision)."""
import math

import numpy as np

F32 = np.float32
STRIDES = (4, 8, 16, 32)
SCALE_CLAMP = math.log(1000.0 / 16.0)
LEVEL_SIDES = (56, 112, 224, 448, 896)
LEVEL_BOUNDS = (112, 224, 448)            # sqrt(area) at which the level changes: p2 | p3 | p4 | p5
SWEEP_ULPS = 8


# ------------------------------------------------------------------------------------------------------------------ level rule
def _level_of(l):
    """clamp(floor(4 + l), 2, 5) - 2 in float32; NaN -> p2 (fmaxf(NaN, 2) = 2)."""
    with np.errstate(invalid="ignore"):
        v = np.floor(F32(4) + l.astype(F32))
        v = np.fmin(np.fmax(v, F32(2)), F32(5))
    return v.astype(np.int64) - 2


def level_ref(rois):
    """detectron2 poolers.py assign_boxes_to_levels, fp32: level = clamp(floor(4 + log2(sqrt(area) / 224 + 1e-8)), 2, 5) - 2.
    area, sqrt, / 224 and + 1e-8 are correctly rounded fp32 operations (the same on every IEEE machine); log2 is taken in float64 and
    rounded to fp32.  Returns (level [R], decided [R]): decided = the fp32 logarithm and both of its fp32 neighbours give the same
    level, so any log2f good to 1 ulp must report it."""
    r = np.asarray(rois, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
        x = np.sqrt(area) / F32(224) + F32(1e-8)
        assert x.dtype == F32
        l = np.log2(x.astype(np.float64)).astype(F32)
    lv = _level_of(l)
    decided = (_level_of(np.nextafter(l, F32(-np.inf))) == lv) & (_level_of(np.nextafter(l, F32(np.inf))) == lv)
    return lv, decided


def level_candidates(rois):
    """Per RoI the set of levels a log2f good to 1 ulp may report."""
    r = np.asarray(rois, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
        l = np.log2((np.sqrt(area) / F32(224) + F32(1e-8)).astype(np.float64)).astype(F32)
    c = np.stack([_level_of(np.nextafter(l, F32(-np.inf))), _level_of(l), _level_of(np.nextafter(l, F32(np.inf)))], 1)
    return [sorted(set(row.tolist())) for row in c]


# ------------------------------------------------------------------------------------------------------------------ RoIAlign
def roi_samples(roi, P, stride, H, W):
    """Sample coordinates of one RoI on a map of H x W cells: (ys [P, gh], xs [P, gw]) float32, or (None, None) for an empty grid.
    roi * (1 / stride) - 0.5, bin = roi_size / P, grid = ceil(roi_size / P), sample = (start + p * bin) + ((i + 0.5) * bin) / grid."""
    r = np.asarray(roi, F32)
    sc = F32(1) / F32(stride)
    sw, sh, ew, eh = (r[0] * sc - F32(0.5), r[1] * sc - F32(0.5), r[2] * sc - F32(0.5), r[3] * sc - F32(0.5))
    rw, rh = ew - sw, eh - sh
    bw, bh = rw / F32(P), rh / F32(P)
    gh, gw = int(np.ceil(bh)), int(np.ceil(bw))
    if gh <= 0 or gw <= 0:
        return None, None
    p = np.arange(P, dtype=F32)[:, None]
    ys = (sh + p * bh) + ((np.arange(gh, dtype=F32)[None, :] + F32(0.5)) * bh) / F32(gh)
    xs = (sw + p * bw) + ((np.arange(gw, dtype=F32)[None, :] + F32(0.5)) * bw) / F32(gw)
    assert ys.dtype == F32 and xs.dtype == F32
    return ys, xs


def _edge_rules(v, size):
    """torchvision bilinear_interpolate on one axis: v < -1 or v > size -> outside; v <= 0 -> 0; lo >= size - 1 -> clamp."""
    bad = (v < F32(-1)) | (v > F32(size))
    v = np.where(v <= 0, F32(0), v)
    lo = np.where(bad, 0, v).astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    v = np.where(top, lo.astype(F32), v)
    l = (v - lo.astype(F32)).astype(F32)
    return bad, lo, hi, l, (F32(1) - l).astype(F32)


def roi_align_ref(maps, rois, batch_idx, P, levels):
    """torchvision roi_align (aligned=True, sampling_ratio=0) over maps = [p2..p5] NHWC float32, one RoI at the level the caller names.
    Per sample ((w1*v1 + w2*v2) + w3*v3) + w4*v4, summed with iy outer and ix inner, then / max(gh * gw, 1).  Returns [R, P, P, C]."""
    rois = np.asarray(rois, F32).reshape(-1, 4)
    C = maps[0].shape[-1]
    out = np.zeros((len(rois), P, P, C), F32)
    for r in range(len(rois)):
        lv = int(levels[r])
        fe = maps[lv][int(batch_idx[r])]
        H, W = fe.shape[:2]
        ys, xs = roi_samples(rois[r], P, STRIDES[lv], H, W)
        if ys is None:
            continue
        gh, gw = ys.shape[1], xs.shape[1]
        ybad, ylo, yhi, ly, hy = _edge_rules(ys, H)
        xbad, xlo, xhi, lx, hx = _edge_rules(xs, W)
        acc = np.zeros((P, P, C), F32)
        for iy in range(gh):
            if ybad[:, iy].all():
                continue
            rows_lo, rows_hi = fe[ylo[:, iy]], fe[yhi[:, iy]]            # [P, W, C]
            for ix in range(gw):
                if xbad[:, ix].all():
                    continue
                w1 = (hy[:, iy, None] * hx[None, :, ix])[..., None]
                w2 = (hy[:, iy, None] * lx[None, :, ix])[..., None]
                w3 = (ly[:, iy, None] * hx[None, :, ix])[..., None]
                w4 = (ly[:, iy, None] * lx[None, :, ix])[..., None]
                v1, v2 = rows_lo[:, xlo[:, ix]], rows_lo[:, xhi[:, ix]]
                v3, v4 = rows_hi[:, xlo[:, ix]], rows_hi[:, xhi[:, ix]]
                val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4
                bad = (ybad[:, iy, None] | xbad[None, :, ix])[..., None]
                acc = np.where(bad, acc, acc + val)                     # a sample outside the map is skipped, not added as zero
        assert acc.dtype == F32
        out[r] = acc / F32(max(gh * gw, 1))
    return out


def roi_kernel_path(C, in_split, roi_lanes, roi_tab):
    """The kernel amp::roi_align_run launches (the dispatch at the end of csrc/roi_align.hip restated)."""
    if roi_lanes == 3 and C == 256:
        return "roi_align_rows_kernel<%s>" % ("true" if in_split else "false")
    if in_split and C == 256:
        return "roi_align_split_tab_kernel" if roi_tab else "roi_align_split_kernel"
    if in_split:
        return "roi_align_kernel<true>"
    return "roi_align_lanes_kernel" if roi_lanes else "roi_align_kernel<false>"


ROI_KERNELS = ("roi_align_kernel<false>", "roi_align_kernel<true>", "roi_align_lanes_kernel", "roi_align_rows_kernel<false>",
               "roi_align_rows_kernel<true>", "roi_align_split_kernel", "roi_align_split_tab_kernel")


def roi_grid_trips(R, P, C, in_split, xcd_order, roi_lanes=1):
    """(work units, workgroups launched x units per workgroup trip): the grid-stride loop takes a second trip when units exceed them."""
    nbins = R * P * P
    if roi_lanes == 3 and C == 256:
        return R * P, min(R * P, 16384)
    if in_split and C == 256:
        if xcd_order:
            per_x = ((R // 8 + 33) * P * P + 7) // 8
            return ((R + 7) // 8 * P * P + 1) // 2, min(per_x, 8192) * 4      # bin pairs of the longest XCD list against its workgroups x 4 waves
        return (nbins + 1) // 2, min((nbins + 7) // 8, 65536) * 4
    return nbins, min((nbins + 3) // 4, 65536) * 4


# ------------------------------------------------------------------------------------------------------------------ split rows
def split_rows_ref(x):
    """fp32 [..., C] (C % 32 == 0) -> the same bytes as split rows: per 32 channels 64 B of hi = f16(x) and 64 B of
    lo' = f16((x - hi) * 2048), returned as float32 of the same shape."""
    x = np.ascontiguousarray(x, F32)
    C = x.shape[-1]
    assert C % 32 == 0
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(F32)) * F32(2048)).astype(np.float16)
    g = np.stack([hi.reshape(-1, C // 32, 32), lo.reshape(-1, C // 32, 32)], 2)         # [rows, groups, hi | lo, 32]
    return np.ascontiguousarray(g).view(F32).reshape(x.shape)


def unsplit_rows_ref(s):
    """The inverse: hi + lo' / 2048 (exact in fp32)."""
    s = np.ascontiguousarray(s, F32)
    C = s.shape[-1]
    g = s.reshape(-1, C // 32, 32).view(np.float16).reshape(-1, C // 32, 2, 32)
    x = g[:, :, 0].astype(F32) + g[:, :, 1].astype(F32) * F32(1.0 / 2048.0)
    return x.reshape(s.shape)


# ------------------------------------------------------------------------------------------------------------------ NMS
def iou_ref(a, b):
    """torchvision nms_kernel IoU of box a against boxes b [n, 4], fp32: inter / ((area_a + area_b) - inter)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32).reshape(-1, 4)
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), F32(0))
    h = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), F32(0))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / ((area_a + area_b) - inter)
    assert iou.dtype == F32
    return iou


def nms_ref(boxes, cats, thresh, max_keep):
    """Greedy NMS over boxes already in descending-score order: a kept box suppresses every later box of its category with
    IoU > float32(thresh) (strict; a NaN IoU, 0/0, never suppresses); stops when max_keep boxes are kept.  Returns kept positions."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    cats = np.asarray(cats)
    n = len(boxes)
    th = F32(thresh)
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) >= max_keep:
            break
        if i + 1 < n:
            alive[i + 1:] &= ~((iou_ref(boxes[i], boxes[i + 1:]) > th) & (cats[i + 1:] == cats[i]))
    return np.asarray(keep, np.int64)


# ------------------------------------------------------------------------------------------------------------------ top-k, decode, sort
def topk_ref(logits, k):
    """The first k of (logit descending, -0.0 == +0.0, ties by ascending anchor index): (indices, logits as the kernel returns them:
    a zero of either sign comes back as +0.0)."""
    s = np.asarray(logits, F32)
    order = np.argsort(-s, kind="stable")[:min(k, len(s))]
    return order.astype(np.int64), (s[order] + F32(0)).astype(F32)


def grid_anchors_ref(h, w, stride, cell):
    """Anchors of an h x w map in (H, W, A) order: shift (x * stride, y * stride) + cell anchor, fp32."""
    sx = (np.arange(w) * stride).astype(F32)
    sy = (np.arange(h) * stride).astype(F32)
    shifts = np.stack(np.broadcast_arrays(sx[None, :], sy[:, None], sx[None, :], sy[:, None]), -1).reshape(-1, 1, 4)
    return (shifts + np.asarray(cell, F32)[None]).reshape(-1, 4).astype(F32)


def decode_ref(anchors, deltas, logits, img_h, img_w):
    """Box2BoxTransform.apply_deltas (weights 1, dw / dh clamped to float32(ln(1000/16))), Boxes.clip, and the validity of
    find_top_rpn_proposals (finite box and logit, clipped w > 0 and h > 0), in float64 from the fp32 inputs; a coordinate beyond the fp32
    range counts as infinite, as it is for the kernel.  Returns (clipped boxes [n, 4] float64, valid [n], margin [n], extent [n]):
    margin is the distance in px of the emptiness decision from its border -- min over both axes of (x2, W - x1, x2 - x1) of the
    unclipped box, positive exactly for a non-empty box -- and 0 for a non-finite one; extent is the largest coordinate involved
    (anchor, centre, size, unclipped box), the scale of the fp32 rounding errors."""
    a = np.asarray(anchors, F32).astype(np.float64)
    d = np.asarray(deltas, F32).astype(np.float64)
    lg = np.asarray(logits, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx, cy = a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h
        clamp = float(F32(SCALE_CLAMP))
        dw, dh = np.minimum(d[:, 2], clamp), np.minimum(d[:, 3], clamp)
        dw, dh = np.where(np.isnan(d[:, 2]), np.nan, dw), np.where(np.isnan(d[:, 3]), np.nan, dh)
        pcx, pcy = d[:, 0] * w + cx, d[:, 1] * h + cy
        pw, ph = np.exp(dw) * w, np.exp(dh) * h
        box = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)
        f32max = float(np.finfo(F32).max)
        parts = np.stack([d[:, 0] * w, d[:, 1] * h, pcx, pcy, pw, ph], 1)
        finite = np.isfinite(box).all(1) & (np.abs(box) <= f32max).all(1) & (np.abs(parts) <= f32max).all(1) & np.isfinite(lg)
        mx = np.minimum(np.minimum(box[:, 2], img_w - box[:, 0]), box[:, 2] - box[:, 0])
        my = np.minimum(np.minimum(box[:, 3], img_h - box[:, 1]), box[:, 3] - box[:, 1])
        margin = np.where(finite, np.minimum(mx, my), 0.0)
        clipped = np.stack([np.clip(box[:, 0], 0, img_w), np.clip(box[:, 1], 0, img_h), np.clip(box[:, 2], 0, img_w),
                            np.clip(box[:, 3], 0, img_h)], 1)
        extent = np.nanmax(np.where(np.isfinite(box), np.abs(box), 0), 1)
        extent = np.maximum(np.maximum(extent, np.abs(a).max(1)), np.where(np.isfinite(parts), np.abs(parts), 0).max(1))
    valid = finite & (margin > 0)
    return clipped, valid, margin, extent


def f2ord_ref(score):
    """common.h f2ord: the order-preserving uint32 image of a float; -0.0 ties with +0.0."""
    u = np.ascontiguousarray(score, F32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000)).astype(np.uint64)


def sortkey_ref(score, pos, cat):
    """common.h make_sortkey: (ordered score << 32) | (0xffffff - position) << 8 | category, as int64 bits; never 0 in the high word."""
    o = f2ord_ref(score)
    k = (o << np.uint64(32)) | ((np.uint64(0xffffff) - np.asarray(pos).astype(np.uint64)) << np.uint64(8)) | \
        (np.asarray(cat).astype(np.uint64) & np.uint64(0xff))
    k = np.where((k >> np.uint64(32)) == 0, k | (np.uint64(1) << np.uint64(32)), k).astype(np.uint64)
    return k.view(np.int64)


def rpn_nms_levels_ref(boxes, keys, sel_count, k, thresh, max_keep):
    """amp_rpn_nms_levels for one image: boxes [cap, 4], keys [cap] int64 sort words (0 = invalid), level l at [off, off + sel_count[l]).
    nms_ref per level over the valid candidates in slot order, survivors merged by descending sort word, first max_keep.
    Returns the kept slots in output order."""
    keys_u = np.asarray(keys).view(np.uint64)
    kept, off = [], 0
    for l, n in enumerate(sel_count):
        n = min(int(n), k)
        slots = off + np.nonzero(keys_u[off:off + n] != 0)[0]
        kp = nms_ref(boxes[slots], np.zeros(len(slots), np.int64), thresh, max_keep)
        kept.extend(slots[kp].tolist())
        off += int(sel_count[l])
    kept = np.asarray(kept, np.int64)
    order = np.argsort(~keys_u[kept], kind="stable")          # descending sort word (words are unique)
    return kept[order][:max_keep]


# ------------------------------------------------------------------------------------------------------------------ case tables
def _step(v, n):
    """v moved n float32 steps (n < 0: down)."""
    v = F32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F32(np.inf if n > 0 else -np.inf))
    return v


def _level_sweep():
    names, rois = [], []
    for s in LEVEL_SIDES:
        for o in (0.0, 0.25, 100.5, 333.3):
            for n in range(-SWEEP_ULPS, SWEEP_ULPS + 1):
                side = _step(s, n)
                for kind in ("square", "one-side"):
                    w, h = side, (side if kind == "square" else F32(s))
                    names.append("side%d%+d-%s-at%g" % (s, n, kind, o))
                    rois.append([F32(o), F32(o), F32(o) + w, F32(o) + h])
        for (w, h, tag) in ((s / 2, 2 * s, "half-by-double"), (s / 4, 4 * s, "quarter-by-quadruple"), (2 * s, s / 2, "double-by-half")):
            names.append("side%d-%s" % (s, tag))
            rois.append([F32(0), F32(0), F32(w), F32(h)])
    names += ["zero-area", "x2-below-x1", "both-sides-negative"]
    rois += [[30, 40, 30, 90], [50, 20, 30, 60], [90, 80, 40, 20]]
    return names, np.asarray(rois, F32)


LEVEL_SWEEP_IDS, LEVEL_SWEEP = _level_sweep()

MAP_HW = ((40, 48), (20, 24), (10, 12), (5, 6))       # p2..p5 of a 160 x 192 image
ROI_P = 7                                              # ROI_EDGE is built for P = 7
# the other side of an edge RoI, in cells, and the side of an edge RoI on both axes: sqrt(area) stays inside the level
_FILL_CELLS = 56
_BOTH_CELLS = (7, 21, 21, 21)


def _edge_span(target, bin_p, n_cells, stride, first_sample):
    """(lo, hi) in px of a RoI side of n_cells cells (k = n_cells / 7 samples per bin, bin = k cells) one of whose samples lands exactly on
    `target` cells: sample (bin_p, i = 0 or k - 1), or -- where that start is no fp32 number -- the very first sample.  Checked here
    with the kernel's own fp32 steps."""
    k = n_cells // ROI_P
    sc = F32(1) / F32(stride)
    for p, i in ((bin_p, 0 if first_sample else k - 1), (0, 0)):
        start = np.float64(target) - (k * p + i)                 # roi_lo / stride: the sample (p, i) sits at start + k p + i
        lo = F32(start * stride)
        if np.float64(lo) != start * stride:
            continue
        for dn in (0, 1, -1, 2, -2, 3, -3, 4, -4):               # the end: any value whose fp32 span is n_cells exactly
            hi = _step(F32((start + n_cells) * stride), dn)
            s_lo = lo * sc - F32(0.5)
            span = (hi * sc - F32(0.5)) - s_lo
            b = span / F32(ROI_P)
            if span == F32(n_cells) and (s_lo + F32(p) * b) + ((F32(i) + F32(0.5)) * b) / F32(k) == F32(target):
                return lo, hi
    raise AssertionError(("no exact span", target, bin_p, n_cells, stride))


def _roi_edge():
    names, rois, targets = [], [], []
    for lv, ((H, W), stride) in enumerate(zip(MAP_HW, STRIDES)):
        for axis, size in (("y", H), ("x", W)):
            tl = [("m1", F32(-1), 0), ("zero", F32(0), 0), ("below-m1", _step(-1, -1), 0), ("m1-last", F32(-1), ROI_P - 1),
                  ("top-1", F32(size - 1), ROI_P - 1), ("top", F32(size), ROI_P - 1), ("above-top", _step(size, 1), ROI_P - 1),
                  ("top-first", F32(size), 0)]
            for tag, t, p in tl:
                lo, hi = _edge_span(t, p, ROI_P, stride, True)
                flo, fhi = F32(-2.0 * stride), F32((-2.0 + _FILL_CELLS) * stride)
                names.append("p%d-%s-%s" % (lv + 2, axis, tag))
                rois.append([flo, lo, fhi, hi] if axis == "y" else [lo, flo, hi, fhi])
                targets.append((lv, axis, tag))
        n = _BOTH_CELLS[lv]
        for tag, ty, tx, p, first in (("m1", F32(-1), F32(-1), 0, True), ("zero", F32(0), F32(0), 0, True),
                                      ("below-m1", _step(-1, -1), _step(-1, -1), 0, True),
                                      ("top-1", F32(H - 1), F32(W - 1), ROI_P - 1, False), ("top", F32(H), F32(W), ROI_P - 1, False),
                                      ("above-top", _step(H, 1), _step(W, 1), ROI_P - 1, False)):
            ylo, yhi = _edge_span(ty, p, n, stride, first)
            xlo, xhi = _edge_span(tx, p, n, stride, first)
            names.append("p%d-both-%s" % (lv + 2, tag))
            rois.append([xlo, ylo, xhi, yhi])
            targets.append((lv, "both", tag))
    names += ["outside-above-left", "outside-below-right", "whole-image", "grid-65-columns", "grid-65-rows"]
    rois += [[-300, -200, -100, -50], [400, 300, 520, 420], [0, 0, 192, 160], [0, 64, 65 * 7 * 32, 96], [64, 0, 96, 65 * 7 * 32]]
    targets += [None] * 5
    return names, np.asarray(rois, F32), targets


ROI_EDGE_IDS, ROI_EDGE, ROI_EDGE_TARGETS = _roi_edge()
ROI_EDGE_BATCH = (np.arange(len(ROI_EDGE)) % 2).astype(np.int32)


def roi_edge_target_value(lv, axis, tag):
    """The cell coordinate the case's name promises, for the axis 'y' or 'x'."""
    size = MAP_HW[lv][0 if axis == "y" else 1]
    return {"m1": F32(-1), "m1-last": F32(-1), "zero": F32(0), "below-m1": _step(-1, -1), "top-1": F32(size - 1), "top": F32(size),
            "top-first": F32(size), "above-top": _step(size, 1)}[tag]


def _box(x, y, w, h):
    return [x, y, x + w, y + h]


def _nms_edge():
    """(name, boxes [n, 4] in score order, cats [n], thresh, expected kept positions or None, on_threshold pair or None)."""
    cases = []
    # A = [0,0,10,15], B = [0,5,10,20]: inter 100, union 150 + 150 - 100 = 200
    cases.append(("iou-exactly-half", [[0, 0, 10, 15], [0, 5, 10, 20]], [0, 0], 0.5, [0, 1], (0, 1)))
    # A = 10 x 10, B = 10 x 7 inside it: inter 70, union 100 -> 70 / 100, which rounds to float32(0.7)
    cases.append(("iou-70-of-100", [[0, 0, 10, 10], [0, 0, 10, 7]], [0, 0], 0.7, [0, 1], (0, 1)))
    # B inside A, IoU = area_B / area_A: the integer pairs (found by search) whose fp32 quotient is the next float above the threshold
    cases.append(("next-above-half", [[0, 0, 2597, 2597], [0, 0, 1649, 2045]], [0, 0], 0.5, [0], (0, 1)))
    cases.append(("next-above-0.7", [[0, 0, 1872, 1872], [0, 0, 1409, 1741]], [0, 0], 0.7, [0], (0, 1)))
    cases.append(("duplicates", [_box(5, 5, 20, 30)] * 3 + [_box(100, 5, 20, 30)] * 2, [0] * 5, 0.5, [0, 3], None))
    cases.append(("zero-area-alone", [_box(5, 5, 0, 30), _box(50, 5, 20, 0), _box(90, 90, 0, 0)], [0] * 3, 0.5, [0, 1, 2], None))
    cases.append(("zero-area-inside", [_box(0, 0, 40, 40), _box(10, 10, 0, 20), _box(10, 10, 20, 0), _box(20, 20, 0, 0)], [0] * 4, 0.5,
                  [0, 1, 2, 3], None))
    cases.append(("zero-area-duplicates", [_box(7, 9, 0, 0), _box(7, 9, 0, 0), _box(7, 9, 0, 5), _box(7, 9, 0, 5)], [0] * 4, 0.5,
                  [0, 1, 2, 3], None))
    cases.append(("same-box-other-category", [_box(5, 5, 20, 30)] * 4, [0, 1, 0, 2], 0.5, [0, 1, 3], None))
    # a > b > c: a suppresses b (IoU 30 / 50 = 0.6), b would suppress c (0.6), a and c overlap by 20 / 60 only: c survives, and so does d
    cases.append(("chain", [_box(0, 0, 40, 10), _box(10, 0, 40, 10), _box(20, 0, 40, 10), _box(40, 0, 40, 10)], [0] * 4, 0.5,
                  None, None))
    disjoint = [_box(30 * (i % 8), 30 * (i // 8), 20, 20) for i in range(64)]
    cases.append(("chunk-all-disjoint", disjoint, [0] * 64, 0.5, list(range(64)), None))
    one = [list(b) for b in disjoint]
    one[41] = _box(30 * (17 % 8) + 2, 30 * (17 // 8), 20, 20)              # overlaps box 17: inter 18 x 20, IoU 360 / 440
    cases.append(("chunk-one-overlap", one, [0] * 64, 0.5, [i for i in range(64) if i != 41], None))
    return cases


def nms_edge_cases():
    """NMS_EDGE as arrays: list of (name, boxes float32 [n, 4], cats int32 [n], thresh, expected kept positions or None, pair)."""
    return [(name, np.asarray(boxes, F32), np.asarray(cats, np.int32), th, exp, pair) for name, boxes, cats, th, exp, pair in _nms_edge()]


NMS_EDGE = nms_edge_cases()
NMS_EDGE_IDS = [c[0] for c in NMS_EDGE]
NMS_ON_THRESHOLD = ("iou-exactly-half", "iou-70-of-100")
NMS_ABOVE_THRESHOLD = ("next-above-half", "next-above-0.7")


def nms_edge_list():
    """All NMS_EDGE cases as ONE score-ordered list: case i is moved 10000 i px in x, far from the others, and its categories are shifted
    by 4 i, so the cases do not meet.  Integer coordinates below 2^24: the shift is exact and every IoU is that of the unshifted boxes.
    Returns (boxes, cats, [(name, slice)])."""
    boxes, cats, slices, n = [], [], [], 0
    for i, (name, b, c, th, exp, pair) in enumerate(NMS_EDGE):
        boxes.append(b + np.asarray([10000 * i, 0, 10000 * i, 0], F32))
        cats.append(c + 4 * i)
        slices.append((name, slice(n, n + len(b))))
        n += len(b)
    return np.concatenate(boxes).astype(F32), np.concatenate(cats).astype(np.int32), slices


def clustered_boxes(n, seed, spread=6.0, size=40.0, centres=24):
    """n boxes of about size px around a few centres: long suppression chains, a few dozen survivors."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0, 2000, (centres, 2))[rng.integers(0, centres, n)] + rng.normal(0, spread, (n, 2))
    wh = size * np.exp(rng.normal(0, 0.08, (n, 2)))
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F32)


def decode_cases():
    """RPN outputs for the decode edges on a two-level pyramid (maps 8 x 8 stride 4 and 4 x 4 stride 8, sizes 32 / 64, A = 3, ld = 16):
    dict name -> (level, pixel, anchor, logit, (dx, dy, dw, dh), exact).  `exact`: built to sit on the validity border (dw = dh = 0)."""
    clamp = F32(SCALE_CLAMP)
    big = F32(3e38)
    return {
        "plain": (0, 27, 1, 3.0, (0.1, -0.2, 0.3, 0.1), False),
        "dw-on-clamp": (0, 28, 1, 2.9, (0.0, 0.0, clamp, 0.0), False),
        "dw-step-above-clamp": (0, 29, 1, 2.8, (0.0, 0.0, _step(clamp, 1), 0.0), False),
        "dw-10x-clamp": (0, 30, 1, 2.7, (0.0, 0.0, F32(10) * clamp, F32(10) * clamp), False),
        "dx-overflows": (0, 35, 1, 2.6, (big, 0.0, 0.0, 0.0), False),
        "dw-inf": (0, 36, 1, 2.5, (0.0, 0.0, F32(np.inf), 0.0), False),
        "dy-nan": (0, 37, 1, 2.4, (0.0, F32(np.nan), 0.0, 0.0), False),
        "dw-nan": (0, 39, 1, 2.35, (0.0, 0.0, F32(np.nan), 0.0), False),          # torch.clamp(max=) keeps the NaN: invalid
        "logit-plus-inf": (0, 38, 1, np.inf, (0.0, 0.0, 0.0, 0.0), False),
        "logit-minus-inf": (1, 5, 1, -np.inf, (0.0, 0.0, 0.0, 0.0), False),
        # pixel 0 of level 0, ratio-1 anchor [-16, -16, 16, 16]: dx = -0.5 puts x2 on 0 exactly (clipped to zero width), one step less
        # leaves 2^-20 px of width
        "zero-width-at-left-border": (0, 0, 1, 2.3, (-0.5, 0.0, 0.0, 0.0), True),
        "one-step-of-width": (0, 8, 1, 2.2, (_step(-0.5, 1), 0.0, 0.0, 0.0), True),
        # pixel 7 of level 0 (x = 28): x1 = 12 with dx = 0, = the width of image 1 -> zero width there, 12 px wide in image 0
        "zero-width-at-image-1-border": (0, 7, 1, 2.1, (0.0, 0.0, 0.0, 0.0), True),
        "level-1-plain": (1, 6, 0, 2.0, (0.05, 0.1, -0.2, 0.2), False),
    }


DECODE_SHAPES = ((8, 8), (4, 4))
DECODE_IMG_HW = ((32, 32), (24, 12))
DECODE_K = 64                # above the 48 anchors of the second level: the -inf logit, the last of its level, is selected too
DECODE_SIZES = (32, 64)
DECODE_STRIDES = (4, 8)
ANCHOR_RATIOS = (0.5, 1.0, 2.0)


def cell_anchors_ref(size, ratios=ANCHOR_RATIOS):
    """detectron2 anchor_generator.py generate_cell_anchors for one size: double arithmetic, stored as fp32."""
    rows = []
    for r in ratios:
        w = math.sqrt(float(size) ** 2 / r)
        h = r * w
        rows.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return np.asarray(rows, F32)


def decode_case_preds(B=2):
    """The RPN predictor outputs of decode_cases(): per level [B, h * w, 16] float32 (logits in columns 0..2, deltas of anchor a in
    3 + 4a .. 6 + 4a, column 15 a pad), the same for every image.  Every anchor no case names has zero deltas (its box is its anchor:
    exact without expf) and a low logit of its own."""
    preds = []
    for l, (h, w) in enumerate(DECODE_SHAPES):
        p = np.zeros((B, h * w, 16), F32)
        p[:, :, :3] = (-1.0 - l - 1e-3 * np.arange(h * w * 3)).reshape(1, h * w, 3)
        preds.append(p)
    for name, (l, pix, an, logit, d, exact) in decode_cases().items():
        preds[l][:, pix, an] = logit
        preds[l][:, pix, 3 + 4 * an:7 + 4 * an] = np.asarray(d, F32)
    return preds


def decode_case_slots():
    """name -> (level, anchor index inside the level)."""
    return {name: (l, pix * 3 + an) for name, (l, pix, an, logit, d, exact) in decode_cases().items()}


def decode_pipeline_ref(preds, shapes, k, img_hw, sizes, strides):
    """topk_ref + decode_ref for every image and level of RPN outputs `preds` ([B, h*w, ld] per level, A = 3): per image a list over
    levels of dict(idx, logit, boxes float64 clipped, valid, margin, dw_dh_zero)."""
    B = preds[0].shape[0]
    out = []
    for b in range(B):
        per_level = []
        for l, (p, (h, w)) in enumerate(zip(preds, shapes)):
            logits = p[b, :, :3].reshape(-1)
            deltas = p[b, :, 3:15].reshape(-1, 4)
            idx, lg = topk_ref(logits, k)
            anchors = grid_anchors_ref(h, w, strides[l], cell_anchors_ref(sizes[l]))
            boxes, valid, margin, extent = decode_ref(anchors[idx], deltas[idx], lg, img_hw[b][0], img_hw[b][1])
            per_level.append(dict(idx=idx, logit=lg, boxes=boxes, valid=valid, margin=margin, extent=extent, deltas=deltas[idx],
                                  exact=(deltas[idx][:, 2] == 0) & (deltas[idx][:, 3] == 0)))
        out.append(per_level)
    return out


# ------------------------------------------------------------------------------------------------------------------ seeded inputs
IMG_HW = (160, 192)


def seeded_rois(n, seed, max_side=300.0):
    """n boxes of 3 .. max_side px (log-uniform sides) around the 160 x 192 image, some partly outside it; (rois, batch_idx of B = 2)."""
    rng = np.random.default_rng(seed)
    rng.random((n, 2))                                             # (unused draw: part of the stream the recorded boxes come from)
    ctr = rng.uniform(0, 1, (n, 2)) * np.array([IMG_HW[1] + 20, IMG_HW[0] + 20]) - 10
    size = np.exp(rng.uniform(np.log(3), np.log(max_side), (n, 2)))
    rois = np.concatenate([ctr - size / 2, ctr + size / 2], 1).astype(F32)
    return rois, rng.integers(0, 2, n).astype(np.int32)


def seeded_maps(C, seed, B=2):
    """[p2..p5] NHWC float32 maps of MAP_HW."""
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1, (B, h, w, C)).astype(F32) for h, w in MAP_HW]


def one_sample_rois(n, seed):
    """n boxes of 8 .. 28 px inside the image: p2, at most 7 cells, one sample per bin at P = 14."""
    rng = np.random.default_rng(seed)
    size = rng.uniform(8, 28, (n, 2))
    tl = rng.uniform(0, 1, (n, 2)) * (np.array([IMG_HW[1], IMG_HW[0]]) - size)
    return np.concatenate([tl, tl + size], 1).astype(F32), rng.integers(0, 2, n).astype(np.int32)
