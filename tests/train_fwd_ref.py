"""NumPy references of the training-forward kernels (csrc/train_fwd.hip, the top-k selection of csrc/select.h), written from the kernels'
header comments and from the detectron2 / fvcore / pycocotools semantics they name.  Nothing here imports oracle/ or the package: the
references are checked AGAINST oracle/train.py in tests/test_train_fwd_ref.py and held against the kernels in
tests/test_label_sample_exact_gpu.py and tests/test_loss_exact_gpu.py.

Two kinds of result.
* Decisions and everything free of expf / logf / log1pf / powf are reproduced bit for bit: every __f*_rn operation of a kernel is one
  correctly rounded fp32 NumPy operation (fp contraction is off in the build).  Anchor labels, both samplers, the polygon mask targets, the
  structure of every gradient map, L1 gradients and the q = 0, 1 delta gradients are of this kind.
* Values behind a transcendental get a float64 value and a PER-ELEMENT error bound (class E below): the rule
      bound = (fp32 roundings on the path + sum of the ulp limits of the math functions on it) * 2^-24 * sum |terms|
  applied node by node: every node adds (its roundings or ulp limit) * 2^-24 * |its value| (+ 2^-126, one flushed denormal) and passes the
  bounds of its inputs on through the operation's derivative, which is what "terms" means once a term is scaled on its way to the element.
  Ulp limits (ULP): OpenCL full profile, which the device library is built to (exp 3, log 3, log1p 2, pow 16); the ROCm install carries no
  HIP math table.  A comparison whose sides are closer than their bounds is recorded in E.unsafe: a case asserts that it has none.

Two facts about the sampling hash decide which cases can exist.
* hash32's finaliser is a bijection of uint32 and the index multiplier 0x27D4EB2F is odd, so two DIFFERENT indices of one (seed, image,
  stream) never share a key.  "Ties by ascending index" is reachable only through amp_roi_sample with repeated prop_anchor identities.
* For any (image, stream, index) exactly one seed makes the hash 0xffffffff, where the key takes its floor value 1: floor_key_seed
  inverts the finaliser and the (odd) seed multiplier.  A floor-key candidate is still a candidate and sorts last.

GIoU subgradient (pinned, giou_ref): a predicted corner EQUAL to the GT corner fails both one-sided tests (x1 > x1g and x1 < x1g), so that
corner gets neither the intersection term nor the enclosing-box term.  No claim about autograd, which splits ties.

Seeded defects (*_DEFECTS): named mutants of each reference; tests/test_train_fwd_ref.py asserts which case catches which."""
import math

import numpy as np

F32 = np.float32
M32 = 0xFFFFFFFF
U = 2.0 ** -24
TINY = 2.0 ** -126
ULP = {"exp": 3, "log": 3, "log1p": 2, "pow": 16}
SCALE_CLAMP = F32(4.135166556742356)          # log(1000 / 16) as the fp32 constant of the kernels
SAMPLE_CHUNK = 49152
SELECT_MAX_K = 2048
MS = 28

LABEL_DEFECTS = ("last_max_wins", "thresholds_strict", "lowq_skips_zero_best", "second_gt_tile_dropped", "lane_chunk_63_dropped")
RPN_SAMPLE_DEFECTS = ("key_floor_missing", "neg_quota_ignores_npos", "chunk_boundary_off_by_one")
ROI_SAMPLE_DEFECTS = ("ties_by_descending_index", "gt_not_appended", "iou_thresh_strict", "prop_count_not_clamped")
LOSS_DEFECTS = ("unused_rows_not_zeroed", "deltas_of_class_0", "beta_edge_inclusive")
MASK_DEFECTS = ("ratio_in_other_precision", "bits_row_major")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- hash, keys, selection
_C_SEED, _C_IMG, _C_STREAM, _C_IDX, _C1, _C2 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x85EBCA6B, 0xC2B2AE35


def hash32(seed, image, stream, idx):
    x = (np.uint64(seed & M32) * np.uint64(_C_SEED) + np.uint64(image) * np.uint64(_C_IMG) + np.uint64(stream) * np.uint64(_C_STREAM)
         + (np.asarray(idx).astype(np.int64).astype(np.uint64) & np.uint64(M32)) * np.uint64(_C_IDX)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(_C1)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(_C2)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def floor_key_seed(image, stream, idx):
    """the one seed with hash32(seed, image, stream, idx) == 0xffffffff (key = its floor 1)"""
    inv = lambda c: pow(c, -1, 1 << 32)
    x = M32
    x ^= x >> 16
    x = (x * inv(_C2)) & M32
    x ^= (x >> 13) ^ (x >> 26)
    x = (x * inv(_C1)) & M32
    x ^= x >> 16
    rest = (image * _C_IMG + stream * _C_STREAM + (idx & M32) * _C_IDX) & M32
    return ((x - rest) * inv(_C_SEED)) & M32


def sample_keys_ref(seed, image, stream, ident, defect=None):
    """uint32 keys of the identities: max(0xffffffff - hash, 1); 0 is reserved for "not a candidate" """
    k = np.uint32(M32) - hash32(seed, image, stream, ident)
    return k if defect == "key_floor_missing" else np.maximum(k, np.uint32(1))


def select_ref(keys, k, defect=None):
    """indices of the min(k, #candidates) largest non-zero keys, ordered by key descending, then index ascending"""
    keys = np.asarray(keys, np.uint32)
    cand = np.flatnonzero(keys)
    idx = -cand if defect == "ties_by_descending_index" else cand
    order = np.lexsort((idx, -keys[cand].astype(np.int64)))
    return cand[order[:max(k, 0)]]


# ---------------------------------------------------------------------------------------------------------------- anchors, IoU, labels
def cell_anchors_ref(sizes, ratios):
    """detectron2 generate_cell_anchors in double, stored as fp32: sizes outer, ratios inner"""
    out = []
    for s in sizes:
        for r in ratios:
            w = math.sqrt(float(s) * float(s) / r)
            h = r * w
            out.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return np.asarray(out, np.float64).astype(F32)


def default_cells(sizes=(32, 64, 128, 256, 512), ratios=(0.5, 1.0, 2.0)):
    return [cell_anchors_ref(s if hasattr(s, "__len__") else [s], ratios) for s in sizes]


def level_offsets(levels, A):
    return np.concatenate([[0], np.cumsum([h * w * A for h, w, _ in levels])]).astype(np.int64)


def anchors_ref(levels, cells):
    """[total, 4] fp32 in (level, y, x, anchor) order: fp32(px * stride) + cell, one rounding each.  levels: (h, w, stride)"""
    out = []
    for (h, w, stride), cell in zip(levels, cells):
        py, px = np.divmod(np.arange(h * w), w)
        sx, sy = (px * stride).astype(F32), (py * stride).astype(F32)
        shift = np.stack([sx, sy, sx, sy], 1)
        out.append((shift[:, None, :] + np.asarray(cell, F32)[None, :, :]).reshape(-1, 4))
    return np.concatenate(out).astype(F32)


def iou_ref(gt, box):
    """detectron2 pairwise_iou(gt, box) in the kernels' fp32 operation order -> [G, N] fp32, 0 where the intersection is empty"""
    gt, box = np.asarray(gt, F32).reshape(-1, 4), np.asarray(box, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ga = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        ba = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        w = np.maximum(np.minimum(gt[:, None, 2], box[None, :, 2]) - np.maximum(gt[:, None, 0], box[None, :, 0]), F32(0))
        h = np.maximum(np.minimum(gt[:, None, 3], box[None, :, 3]) - np.maximum(gt[:, None, 1], box[None, :, 1]), F32(0))
        inter = w * h
        v = inter / ((ga[:, None] + ba[None, :]) - inter)
    return np.where(inter > 0, v, F32(0)).astype(F32)


RULES = ("low", "lo_eq", "mid", "hi_eq", "hi")          # which threshold rule a match value falls under (before the low-quality rule)


def anchor_labels_ref(levels, cells, gt_per_image, lo, hi, defect=None):
    """-> dict(match_val [B,N] f32, match_idx [B,N] i32, gt_best [sum G] u32 (fp32 bits), label [B,N] i8, rule [B,N] index into RULES,
    lowq [B,N] bool: the low-quality rule set the label, zero_best [B] bool: a GT box with best IoU 0 marked the whole image)"""
    anc = anchors_ref(levels, cells)
    N, B = len(anc), len(gt_per_image)
    lo, hi = F32(lo), F32(hi)
    mv, mi = np.zeros((B, N), F32), np.zeros((B, N), np.int32)
    label, rule = np.zeros((B, N), np.int8), np.zeros((B, N), np.int8)
    lowq, zero_best, best_all = np.zeros((B, N), bool), np.zeros(B, bool), []
    for b, gt in enumerate(gt_per_image):
        gt = np.asarray(gt, F32).reshape(-1, 4)
        G = len(gt)
        if G == 0:
            continue
        q = iou_ref(gt, anc)
        seen = np.ones(G, bool)
        if defect == "second_gt_tile_dropped":
            seen[256:] = False
        if defect == "lane_chunk_63_dropped":
            seen[63::64] = False
        q[~seen] = 0
        if defect == "last_max_wins":
            mi[b] = G - 1 - np.argmax(q[::-1], axis=0)
        else:
            mi[b] = np.argmax(q, axis=0)          # the first maximum; all-zero columns -> 0
        mv[b] = q[mi[b], np.arange(N)]
        best = q.max(axis=1)
        best_all.append(best)
        v = mv[b]
        rule[b] = np.where(v > hi, 4, np.where(v == hi, 3, np.where(v > lo, 2, np.where(v == lo, 1, 0))))
        if defect == "thresholds_strict":
            label[b] = np.where(v > hi, 1, np.where(v > lo, -1, 0))
        else:
            label[b] = np.where(v >= hi, 1, np.where(v >= lo, -1, 0))
        zb = seen & (best == 0)
        if defect == "lowq_skips_zero_best":
            zb[:] = False
        zero_best[b] = zb.any()
        lq = ((q == best[:, None]) & (best[:, None] > 0) & seen[:, None]).any(axis=0) | zero_best[b]
        lowq[b] = lq
        label[b][lq] = 1
    gt_best = bits(np.concatenate(best_all).astype(F32)) if best_all else np.zeros(0, np.uint32)
    return dict(match_val=mv, match_idx=mi, gt_best=gt_best, label=label, rule=rule, lowq=lowq, zero_best=zero_best)


def wave_coverage(anc, gt):
    """per GT box: (waves of 64 anchors whose bounding box it overlaps, waves with an anchor it intersects); lanes past the last anchor hold
    an empty box at the origin, as in the kernels"""
    anc, gt = np.asarray(anc, F32), np.asarray(gt, F32).reshape(-1, 4)
    nw = -(-len(anc) // 64)
    pad = np.zeros((nw * 64, 4), F32)
    pad[:len(anc)] = anc
    wv = pad.reshape(nw, 64, 4)
    bb = np.stack([wv[:, :, 0].min(1), wv[:, :, 1].min(1), wv[:, :, 2].max(1), wv[:, :, 3].max(1)], 1)
    q = iou_ref(gt, pad).reshape(len(gt), nw, 64)
    out = []
    for j, g in enumerate(gt):
        hit = (g[0] < bb[:, 2]) & (g[2] > bb[:, 0]) & (g[1] < bb[:, 3]) & (g[3] > bb[:, 1])
        out.append((set(np.flatnonzero(hit).tolist()), set(np.flatnonzero((q[j] > 0).any(1)).tolist())))
    return out


# ---------------------------------------------------------------------------------------------------------------- RPN sampler
def rpn_sample_path_ref(total, B, batch):
    """('chunked' | 'one_wg', number of chunks): the host's dispatch rule of amp_rpn_sample_loss"""
    nch = -(-total // SAMPLE_CHUNK)
    need = B * 2 * nch * batch * 8 + B * 2 * nch * 4
    return ("chunked" if nch * batch <= SELECT_MAX_K and need <= B * total * 4 else "one_wg"), nch


def rpn_sample_ref(label, seed, batch, pos_max, defect=None):
    """-> (sampled [B, batch] i32: positives then negatives, -1 behind the counted prefix; counts [B, 2])"""
    label = np.asarray(label, np.int8)
    B, N = label.shape
    sampled, counts = np.full((B, batch), -1, np.int32), np.zeros((B, 2), np.int32)
    idx = np.arange(N)
    seen = np.ones(N, bool)
    if defect == "chunk_boundary_off_by_one":          # the first anchor of every later chunk belongs to no chunk
        seen[SAMPLE_CHUNK::SAMPLE_CHUNK] = False
    for b in range(B):
        kp = np.where((label[b] == 1) & seen, sample_keys_ref(seed, b, 0, idx, defect), np.uint32(0))
        pos = select_ref(kp, pos_max)
        kn = np.where((label[b] == 0) & seen, sample_keys_ref(seed, b, 1, idx, defect), np.uint32(0))
        neg = select_ref(kn, batch - (pos_max if defect == "neg_quota_ignores_npos" else len(pos)))
        neg = neg[:batch - len(pos)]
        sampled[b, :len(pos)] = pos
        sampled[b, len(pos):len(pos) + len(neg)] = neg
        counts[b] = len(pos), len(neg)
    return sampled, counts


# ---------------------------------------------------------------------------------------------------------------- RoI sampler
def roi_sample_ref(prop_boxes, prop_count, prop_anchor, gt_per_image, cls_per_image, K, batch, fg_max, iou_thresh, seed, num_anchors,
                   defect=None):
    """label_and_sample_proposals: proposals clamped to Pcap, GT appended, first maximum over GT, foreground iff IoU >= iou_thresh, identities
    prop_anchor[i] / num_anchors + j, foreground (stream 2) then background (stream 3).
    -> rois [B,batch,4] f32, roi_cls [B,batch] (K background, -1 unused), roi_gti [B,batch] (-1 where the kernel writes nothing), counts [B,2]"""
    prop_boxes, prop_anchor = np.asarray(prop_boxes, F32), np.asarray(prop_anchor, np.int64)
    B, Pcap = prop_boxes.shape[:2]
    flat_boxes = np.concatenate([prop_boxes.reshape(-1, 4), np.zeros((max(int(np.max(prop_count)), Pcap), 4), F32)])
    flat_ident = np.concatenate([prop_anchor.reshape(-1), np.zeros(max(int(np.max(prop_count)), Pcap), np.int64)])
    rois, roi_cls = np.zeros((B, batch, 4), F32), np.full((B, batch), -1, np.int32)
    roi_gti, counts = np.full((B, batch), -1, np.int32), np.zeros((B, 2), np.int32)
    thr = F32(iou_thresh)
    for b in range(B):
        P = int(prop_count[b]) if defect == "prop_count_not_clamped" else min(int(prop_count[b]), Pcap)
        gt = np.asarray(gt_per_image[b], F32).reshape(-1, 4)
        G = len(gt)
        app = 0 if defect == "gt_not_appended" else G
        boxes = np.concatenate([flat_boxes[b * Pcap:b * Pcap + P], gt[:app]])
        ident = np.concatenate([flat_ident[b * Pcap:b * Pcap + P], num_anchors + np.arange(app)])
        n = len(boxes)
        if G:
            q = iou_ref(gt, boxes)
            gti = np.argmax(q, axis=0).astype(np.int32)
            best = q[gti, np.arange(n)]
            fg = best > thr if defect == "iou_thresh_strict" else best >= thr
            cls = np.where(fg, np.asarray(cls_per_image[b], np.int32)[gti], K)
        else:
            gti, cls = np.zeros(n, np.int32), np.full(n, K, np.int32)
        kf = np.where(cls != K, sample_keys_ref(seed, b, 2, ident), np.uint32(0)) if n else np.zeros(0, np.uint32)
        sf = select_ref(kf, fg_max, defect)
        kb = np.where(cls == K, sample_keys_ref(seed, b, 3, ident), np.uint32(0)) if n else np.zeros(0, np.uint32)
        sb = select_ref(kb, batch - len(sf), defect)
        sel = np.concatenate([sf, sb]).astype(np.int64)
        m = len(sel)
        rois[b, :m] = boxes[sel]
        roi_cls[b, :m] = np.concatenate([cls[sf], np.full(len(sb), K, np.int32)])
        roi_gti[b, :m] = gti[sel]
        counts[b] = len(sf), len(sb)
    return rois, roi_cls, roi_gti, counts


# ---------------------------------------------------------------------------------------------------------------- mask targets
def fr_poly_ref(xy, h, w):
    """pycocotools rleFrPoly of a polygon already in the h x w frame -> bool [h, w] (the decoded runs)"""
    k = len(xy) // 2
    x = [int(5.0 * float(xy[2 * j]) + 0.5) for j in range(k)]          # C's (int): truncation toward zero, as Python's int()
    y = [int(5.0 * float(xy[2 * j + 1]) + 0.5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        s = ((ye - ys) / dx if dx else 0.0) if dx >= dy else (xe - xs) / dy
        for d in range(max(dx, dy) + 1):
            t = (max(dx, dy) - d) if flip else d
            if dx >= dy:
                u.append(t + xs)
                v.append(int(ys + s * t + 0.5))
            else:
                v.append(t + ys)
                u.append(int(xs + s * t + 0.5))
    tog = np.zeros(h * w + 1, np.int64)
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = (float(u[j] if u[j] < u[j - 1] else u[j] - 1) + 0.5) / 5.0 - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = (float(v[j] if v[j] < v[j - 1] else v[j - 1]) + 0.5) / 5.0 - 0.5
        yd = math.ceil(min(max(yd, 0.0), float(h)))
        tog[int(xd) * h + int(yd)] ^= 1          # a run boundary; runs alternate, zero-length runs merge: parity
    return (np.cumsum(tog)[:h * w] & 1).astype(bool).reshape(w, h).T


def mask_ratio(side32, precision):
    """28 / max(side, 0.1): 'double' -- the oracle and detectron2 under NumPy 1.x (PINNED) -- or 'float' -- detectron2 under NumPy 2"""
    if precision == "double":
        return 28.0 / max(float(side32), 0.1)
    return float(F32(MS) / max(F32(side32), F32(0.1)))


def mask_target_ref(polys, box, precision="double", defect=None):
    """rasterize_polygons_within_box: box sides as fp32 differences, the ratio in `precision`, the polygon arithmetic in double, rleFrPoly per
    polygon, union -> bool [28, 28] (row-major: [y, x])"""
    box = np.asarray(box, F32)
    if defect == "ratio_in_other_precision":
        precision = "float" if precision == "double" else "double"
    rw, rh = mask_ratio(box[2] - box[0], precision), mask_ratio(box[3] - box[1], precision)
    out = np.zeros((MS, MS), bool)
    for p in polys:
        p = np.asarray(p, np.float64)
        q = np.empty_like(p)
        q[0::2] = (p[0::2] - float(box[0])) * rw
        q[1::2] = (p[1::2] - float(box[1])) * rh
        out |= fr_poly_ref(q, MS, MS)
    return out.T.copy() if defect == "bits_row_major" else out


# ---------------------------------------------------------------------------------------------------------------- error-tracked fp32
class E:
    """An fp32 quantity of a kernel: v the value in float64 arithmetic from the fp32 inputs, e a bound on |kernel - v|, f the fp32 value by
    correctly rounded NumPy operations, x True where f is what the kernel holds bit for bit (no transcendental on the path)."""
    unsafe = []          # (what, count) of comparisons decided inside the error bounds since the last reset
    __array_ufunc__ = None          # NumPy scalars and arrays defer to the reflected operators

    def __init__(self, v, e=None, f=None, x=None):
        self.v = np.asarray(v, np.float64)
        self.f = np.asarray(v, F32) if f is None else np.asarray(f, F32)
        self.e = np.zeros(self.v.shape) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape)
        self.x = np.ones(self.v.shape, bool) if x is None else np.broadcast_to(np.asarray(x, bool), self.v.shape)

    @staticmethod
    def of(a):
        return a if isinstance(a, E) else E(np.asarray(a, F32).astype(np.float64), f=np.asarray(a, F32))

    def _round(self, v, e, f, x, n=1.0):
        return E(v, e + n * U * np.abs(v) + TINY, f, x)

    def __add__(a, b):
        b = E.of(b)
        with np.errstate(all="ignore"):
            return a._round(a.v + b.v, a.e + b.e, a.f + b.f, a.x & b.x)

    def __sub__(a, b):
        b = E.of(b)
        with np.errstate(all="ignore"):
            return a._round(a.v - b.v, a.e + b.e, a.f - b.f, a.x & b.x)

    def __rsub__(a, b):
        return E.of(b) - a

    def __radd__(a, b):
        return E.of(b) + a

    def __mul__(a, b):
        b = E.of(b)
        with np.errstate(all="ignore"):
            return a._round(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e, a.f * b.f, a.x & b.x)

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = E.of(b)
        with np.errstate(all="ignore"):
            v = a.v / b.v
            return a._round(v, a.e / np.abs(b.v) + np.abs(v) * b.e / np.abs(b.v), a.f / b.f, a.x & b.x)

    def __rtruediv__(a, b):
        return E.of(b) / a

    def __neg__(a):
        return E(-a.v, a.e, -a.f, a.x)

    def abs(a):
        return E(np.abs(a.v), a.e, np.abs(a.f), a.x)

    def half(a):          # x 0.5: exact
        return E(0.5 * a.v, 0.5 * a.e, F32(0.5) * a.f, a.x)

    def _fn(a, name, v, dv):
        with np.errstate(all="ignore"):
            return E(v, dv * a.e + ULP[name] * U * np.abs(v) + TINY, v.astype(F32), False)

    def exp(a):          # expf(0) = 1 and logf(1) = 0 exactly
        with np.errstate(all="ignore"):
            v = np.exp(a.v)
        return E.where(a.x & (a.f == 0), E.of(np.ones_like(a.f)), a._fn("exp", v, v))

    def log(a):
        with np.errstate(all="ignore"):
            return E.where(a.x & (a.f == 1), E.of(np.zeros_like(a.f)), a._fn("log", np.log(a.v), 1.0 / np.abs(a.v)))

    def log1p(a):
        with np.errstate(all="ignore"):
            return a._fn("log1p", np.log1p(a.v), 1.0 / np.abs(1.0 + a.v))

    def pow(a, g):
        g = float(g)
        with np.errstate(all="ignore"):
            dv = np.zeros(a.v.shape) if g == 0 else (np.ones(a.v.shape) if g == 1 else g * np.power(a.v, g - 1))
            return a._fn("pow", np.power(a.v, g), dv)

    def val(a):
        """the side of a comparison: the kernel's own bits where they are known"""
        return np.where(a.x, a.f.astype(np.float64), a.v)

    @staticmethod
    def less(a, b, what):
        """a < b as the kernel decides it; a decision inside the bounds of inexact sides is recorded as unsafe"""
        a, b = E.of(a), E.of(b)
        r = a.val() < b.val()
        near = ~(a.x & b.x) & (np.abs(a.v - b.v) <= a.e + b.e)
        if near.any():
            E.unsafe.append((what, int(near.sum())))
        return r

    @staticmethod
    def where(c, a, b):
        a, b = E.of(a), E.of(b)
        return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e), np.where(c, a.f, b.f), np.where(c, a.x, b.x))

    @staticmethod
    def fmin(a, b, what):
        return E.where(E.less(a, b, what), a, b)

    @staticmethod
    def fmax(a, b, what):
        return E.where(E.less(a, b, what), b, a)

    def __getitem__(a, i):
        return E(a.v[i], a.e[i], a.f[i], a.x[i])


def tree_sum(el, width):
    """the kernels' reduction: s[t] += s[t + o] for o = width / 2 ... 1 over `width` slots (missing slots are 0)"""
    pad = lambda z, fill: np.concatenate([z.reshape(-1), np.full(width - z.size, fill, z.dtype)])
    s = E(pad(el.v, 0.0), pad(el.e, 0.0), pad(el.f, F32(0)), pad(el.x, True))
    o = width // 2
    while o:
        s = s[:o] + s[o:2 * o]
        o //= 2
    return s[0]


def bce_ref(x, y):
    """binary_cross_entropy_with_logits and d/dx (before the scale): max(x,0) - x y + log1p(exp(-|x|)); sigmoid(x) - y"""
    x, y = E.of(x), E.of(y)
    relu = E.where(x.f > 0, x, E.of(np.zeros_like(x.f)))
    loss = (relu - x * y) + (-x.abs()).exp().log1p()
    grad = 1.0 / (1.0 + (-x).exp()) - y
    return loss, grad


def deltas_ref(src, gt, w):
    """Box2BoxTransform.get_deltas in the kernels' operation order -> four E (q = 0, 1 exact)"""
    s, g = [E.of(src[:, i]) for i in range(4)], [E.of(gt[:, i]) for i in range(4)]
    sw, sh = s[2] - s[0], s[3] - s[1]
    sx, sy = s[0] + sw.half(), s[1] + sh.half()
    tw, th = g[2] - g[0], g[3] - g[1]
    tx, ty = g[0] + tw.half(), g[1] + th.half()
    return [(F32(w[0]) * (tx - sx)) / sw, (F32(w[1]) * (ty - sy)) / sh, F32(w[2]) * (tw / sw).log(), F32(w[3]) * (th / sh).log()]


def smooth_l1_ref(d, beta, mode, defect=None):
    """(loss, d loss / d d) of the differences d.  mode 'l1': |d|, sign(d) (0 at 0); 'smooth_l1': fvcore, quadratic for |d| < beta (strict)"""
    zero = E.of(np.zeros_like(d.f))
    pos, neg = E.less(zero, d, "sign of d"), E.less(d, zero, "sign of d")
    sign = E.of(np.where(pos, 1.0, -1.0).astype(F32))
    if mode == "l1":
        return d.abs(), E.of(np.where(pos, 1.0, np.where(neg, -1.0, 0.0)).astype(F32))
    b = E.of(np.full_like(d.f, F32(beta)))
    quad = E.less(d.abs(), b, "|d| < beta")
    if defect == "beta_edge_inclusive":
        quad = quad | (d.abs().val() == b.val())
    return E.where(quad, (d * d).half() / b, d.abs() - b.half()), E.where(quad, d / b, sign)


def giou_ref(p, src, w, gb):
    """fvcore giou_loss(apply_deltas(p, src, w), gb, eps 1e-7) per box and its gradient w.r.t. the four deltas, in the kernel's operation
    order.  p: four E / fp32 arrays.  A corner equal to the GT corner gets neither the I-term nor the C-term (the pinned subgradient)."""
    p = [E.of(q) for q in p]
    s, g = [E.of(src[:, i]) for i in range(4)], [E.of(gb[:, i]) for i in range(4)]
    eps = F32(1e-7)
    sw, sh = s[2] - s[0], s[3] - s[1]
    sx, sy = s[0] + sw.half(), s[1] + sh.half()
    dx, dy, dw, dh = p[0] / F32(w[0]), p[1] / F32(w[1]), p[2] / F32(w[2]), p[3] / F32(w[3])
    clamp = E.of(np.full_like(dw.f, SCALE_CLAMP))
    cw, ch = E.less(clamp, dw, "dw > clamp"), E.less(clamp, dh, "dh > clamp")
    dw, dh = E.where(cw, clamp, dw), E.where(ch, clamp, dh)
    pcx, pcy = dx * sw + sx, dy * sh + sy
    pw, ph = dw.exp() * sw, dh.exp() * sh
    x1, y1, x2, y2 = pcx - pw.half(), pcy - ph.half(), pcx + pw.half(), pcy + ph.half()
    x1g, y1g, x2g, y2g = g
    bw, bh = x2 - x1, y2 - y1
    iw = E.fmin(x2, x2g, "x2 : x2g") - E.fmax(x1, x1g, "x1 : x1g")
    ih = E.fmin(y2, y2g, "y2 : y2g") - E.fmax(y1, y1g, "y1 : y1g")
    zero = E.of(np.zeros_like(iw.f))
    hit = E.less(zero, iw, "iw > 0") & E.less(zero, ih, "ih > 0")
    I = E.where(hit, iw * ih, zero)
    Uu = (bw * bh + (x2g - x1g) * (y2g - y1g)) - I
    Ue = Uu + eps
    ew = E.fmax(x2, x2g, "x2 : x2g") - E.fmin(x1, x1g, "x1 : x1g")
    eh = E.fmax(y2, y2g, "y2 : y2g") - E.fmin(y1, y1g, "y1 : y1g")
    Cc = ew * eh
    Ce = Cc + eps
    iou = I / Ue
    loss = 1.0 - (iou - (Cc - Uu) / Ce)
    gU = iou / Ue - 1.0 / Ce
    gI = -1.0 / Ue - gU
    gC = Ue / (Ce * Ce)
    gx1, gx2, gy1, gy2 = gU * (-bh), gU * bh, gU * (-bw), gU * bw
    gx1 = E.where(hit & E.less(x1g, x1, "x1 : x1g"), gx1 - gI * ih, gx1)
    gx2 = E.where(hit & E.less(x2, x2g, "x2 : x2g"), gx2 + gI * ih, gx2)
    gy1 = E.where(hit & E.less(y1g, y1, "y1 : y1g"), gy1 - gI * iw, gy1)
    gy2 = E.where(hit & E.less(y2, y2g, "y2 : y2g"), gy2 + gI * iw, gy2)
    gx1 = E.where(E.less(x1, x1g, "x1 : x1g"), gx1 - gC * eh, gx1)
    gx2 = E.where(E.less(x2g, x2, "x2 : x2g"), gx2 + gC * eh, gx2)
    gy1 = E.where(E.less(y1, y1g, "y1 : y1g"), gy1 - gC * ew, gy1)
    gy2 = E.where(E.less(y2g, y2, "y2 : y2g"), gy2 + gC * ew, gy2)
    zg = E.of(np.zeros_like(iw.f))
    grad = [((gx1 + gx2) * sw) / F32(w[0]), ((gy1 + gy2) * sh) / F32(w[1]),
            E.where(cw, zg, (((gx2 - gx1).half()) * pw) / F32(w[2])), E.where(ch, zg, (((gy2 - gy1).half()) * ph) / F32(w[3]))]
    kind = np.where(~hit, "disjoint", np.where((E.less(x1, x1g, "") & E.less(y1, y1g, "") & E.less(x2g, x2, "") & E.less(y2g, y2, ""))
                                               | (E.less(x1g, x1, "") & E.less(y1g, y1, "") & E.less(x2, x2g, "") & E.less(y2, y2g, "")),
                                               "nested", "partial"))
    return loss, grad, dict(clamped_w=cw, clamped_h=ch, kind=kind, corners=(x1, y1, x2, y2))


def reg_ref(mode, beta, p, src, gt, w, defect=None):
    """(the loss terms a thread adds in order -- four E for L1 / smooth-L1, one for GIoU --, four gradient E) of the predicted deltas p (four
    fp32 arrays) of boxes src against gt"""
    if mode == "giou":
        loss, grad, _ = giou_ref(p, src, w, gt)
        return [loss], grad
    t = deltas_ref(src, gt, w)
    terms, grad = [], []
    for q in range(4):
        l, g = smooth_l1_ref(E.of(p[q]) - t[q], beta, mode, defect)
        terms.append(l)
        grad.append(g)
    return terms, grad


def reg_mode(loss_type, beta):
    """which instantiation of the loss kernels the host launches: fvcore's smooth_l1_loss is |d| below beta = 1e-5"""
    return "giou" if loss_type == "giou" else ("l1" if F32(beta) < F32(1e-5) else "smooth_l1")


def _scatter(el, idx, n):
    """an E of n zeros (exact) with el at idx"""
    v, e, f, x = np.zeros(n), np.zeros(n), np.zeros(n, F32), np.ones(n, bool)
    v[idx], e[idx], f[idx], x[idx] = el.v, el.e, el.f, el.x
    return E(v, e, f, x)


def _acc(acc, el):
    """acc + el where a thread adds (el may be shorter than acc: the other threads add nothing); 0 + el is exact"""
    n = el.v.size
    first = (acc.f[:n] == 0) & acc.x[:n] & (acc.e[:n] == 0)
    s = E.where(first, el, acc[:n] + el)
    return E(np.concatenate([s.v, acc.v[n:]]), np.concatenate([s.e, acc.e[n:]]), np.concatenate([s.f, acc.f[n:]]), np.concatenate([s.x, acc.x[n:]]))


class GradMap:
    """a gradient map: float64 values, bounds, the cells whose bits are known, the cells the kernel writes (all others must keep their preset)"""
    def __init__(self, shape):
        self.v, self.e = np.zeros(shape), np.zeros(shape)
        self.f, self.x, self.written = np.zeros(shape, F32), np.ones(shape, bool), np.zeros(shape, bool)

    def put(self, idx, el):
        self.v[idx], self.e[idx], self.f[idx], self.x[idx], self.written[idx] = el.v, el.e, el.f, el.x, True

    def as_e(self):
        return E(self.v, self.e, self.f, self.x)


def rpn_loss_ref(levels, cells, preds, gt_per_image, match_idx, sampled, counts, mode, beta, cls_scale, loc_scale, defect=None):
    """amp_rpn_sample_loss_ex behind the sampler.  preds: per level [B, h*w, ld] fp32; cls_scale / loc_scale: the fp32 scales the host forms.
    -> (per image (sum BCE, sum regression loss) as E, a GradMap per level: the caller zero-fills, the kernel writes the listed cells)"""
    A = len(cells[0])
    anc, off = anchors_ref(levels, cells), level_offsets(levels, A)
    maps = [GradMap(p.shape) for p in preds]
    partial = []
    for b in range(len(gt_per_image)):
        npos, nneg = int(counts[b, 0]), int(counts[b, 1])
        an = np.asarray(sampled[b, :npos + nneg], np.int64)
        n = len(an)
        zero = E.of(np.zeros(1024, F32))
        if n == 0:
            partial.append((zero[0], zero[0]))
            continue
        lvl = np.searchsorted(off, an, side="right") - 1
        local = an - off[lvl]
        pix, k = local // A, local % A
        row = np.stack([preds[l][b, px] for l, px in zip(lvl, pix)])          # [n, ld]
        bce, g = bce_ref(row[np.arange(n), k], (np.arange(n) < npos).astype(F32))
        g = g * F32(cls_scale)
        loc = zero
        if npos:
            gt = np.asarray(gt_per_image[b], F32).reshape(-1, 4)[np.asarray(match_idx[b], np.int64)[an[:npos]]]
            p = [row[np.arange(npos), A + 4 * k[:npos] + q] for q in range(4)]
            terms, gl = reg_ref(mode, beta, p, anc[an[:npos]], gt, (1.0, 1.0, 1.0, 1.0), defect)
            for t in terms:
                loc = _acc(loc, t)
            gl = [q * F32(loc_scale) for q in gl]
        for l in set(lvl.tolist()):
            m = lvl == l
            maps[l].put((b, pix[m], k[m]), g[m])
            mp = m[:npos]
            for q in range(4 if npos else 0):
                maps[l].put((b, pix[:npos][mp], A + 4 * k[:npos][mp] + q), gl[q][mp])
        partial.append((tree_sum(bce, 1024), tree_sum(loc, 1024)))
    return partial, maps


def box_loss_ref(pred, K, rois, roi_cls, roi_gti, gt_per_image, batch, w, mode, beta, inv_total, reg_scale, defect=None):
    """amp_box_loss_ex.  pred [B*batch, ld] fp32, rois [B, batch, 4], roi_cls / roi_gti [B, batch].
    -> (per image (sum CE, sum regression loss) as E, GradMap [B*batch, ld]: the kernel writes every cell of every row)"""
    pred = np.asarray(pred, F32)
    gm = GradMap(pred.shape)
    partial = []
    for b in range(len(gt_per_image)):
        rows = np.arange(b * batch, (b + 1) * batch)
        c = np.asarray(roi_cls[b], np.int64)
        used = c >= 0
        if defect != "unused_rows_not_zeroed":
            gm.written[rows[~used]] = True
        ce, reg = E.of(np.zeros(batch, F32)), [E.of(np.zeros(batch, F32))]
        if used.any():
            ru, cu = rows[used], c[used]
            P = pred[ru]
            lg = E.of(P[:, :K + 1])
            mx = P[:, :K + 1].max(axis=1)
            ex = [(lg[:, k] - mx).exp() for k in range(K + 1)]
            s = ex[0]
            for t in ex[1:]:
                s = s + t
            ce = _scatter((mx + s.log()) - E.of(P[np.arange(len(ru)), cu]), np.flatnonzero(used), batch)
            gm.written[ru] = True          # the columns behind the K + 1 logits and the GT-class deltas: zeros
            for k in range(K + 1):
                gm.put((ru, k), (ex[k] / s - (cu == k).astype(F32)) * F32(inv_total))
            fg = cu < K
            if fg.any():
                rf, cf = ru[fg], cu[fg]
                col = K + 1 + 4 * (np.zeros_like(cf) if defect == "deltas_of_class_0" else cf)
                gt = np.asarray(gt_per_image[b], F32).reshape(-1, 4)[np.asarray(roi_gti[b], np.int64)[used][fg]]
                terms, gl = reg_ref(mode, beta, [pred[rf, col + q] for q in range(4)], np.asarray(rois[b], F32)[used][fg], gt, w, defect)
                for q in range(4):
                    gm.put((rf, col + q), gl[q] * F32(reg_scale))
                reg = [_scatter(t, np.flatnonzero(used)[fg], batch) for t in terms]
        # thread t adds its rows t, t + 512, ... in order, the terms of a row in order; then the 512-slot tree
        acc_ce, acc_reg = E.of(np.zeros(512, F32)), E.of(np.zeros(512, F32))
        for r0 in range(0, batch, 512):
            acc_ce = _acc(acc_ce, ce[r0:min(r0 + 512, batch)])
            for t in reg:
                acc_reg = _acc(acc_reg, t[r0:min(r0 + 512, batch)])
        partial.append((tree_sum(acc_ce, 512), tree_sum(acc_reg, 512)))
    return partial, gm


def focal_ref(x, labels, K, alpha, gamma, scale):
    """fvcore sigmoid_focal_loss per element: (loss E [N, K] before the scale, gradient E [N, K] scaled); rows with label < 0 are exact zeros"""
    x = np.asarray(x, F32).reshape(-1, K)
    labels = np.asarray(labels, np.int64)
    t = (labels[:, None] == np.arange(K)[None, :]).astype(F32)
    X, T = E.of(x), E.of(t)
    p = 1.0 / (1.0 + (-X).exp())
    relu = E.where(x > 0, X, E.of(np.zeros_like(x)))
    ce = (relu - X * T) + (-X.abs()).exp().log1p()
    omp, omt = 1.0 - p, E.of(F32(1) - t)
    pt = p * T + omp * omt
    q = 1.0 - pt
    one = E.of(np.ones_like(x))
    mod = one if gamma == 0 else q.pow(gamma)
    a32 = F32(alpha)
    at = E.of((a32 * t + (F32(1) - a32) * (F32(1) - t)).astype(F32)) if alpha >= 0 else one
    loss = (at * ce) * mod
    dpt = (p * omp) * E.of(F32(2) * t - F32(1))
    dmod = E.of(np.zeros_like(x)) if gamma == 0 else (F32(-gamma) * q.pow(gamma - 1.0)) * dpt
    g = (at * ((p - T) * mod + ce * dmod)) * F32(scale)
    live = (labels >= 0)[:, None] & np.ones((1, K), bool)
    z = E.of(np.zeros_like(x))
    return E.where(live, loss, z), E.where(live, g, z)


def check_bound(got, el, what):
    """got (fp32 array) against an E: bits where they are known, |got - v| <= e elsewhere.  -> the worst error / bound (0 where exact)"""
    got = np.asarray(got, F32).reshape(el.v.shape)
    bad = el.x & (bits(got) != bits(el.f))          # the sign of a zero included
    assert not bad.any(), (what, f"{int(bad.sum())} exact cells differ", np.argwhere(bad)[:4].tolist())
    assert np.isfinite(got).all(), (what, "a non-finite value")
    err = np.abs(got.astype(np.float64) - el.v)
    with np.errstate(all="ignore"):
        ratio = np.where(el.x | (err == 0), 0.0, err / el.e)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst < 1.0, (what, f"error / bound {worst:.3f}", np.argwhere(ratio >= 1)[:4].tolist())
    return worst
