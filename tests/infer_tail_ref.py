"""NumPy references of the inference tail (csrc/mask_paste.hip, csrc/box_infer.hip), written from the documented operation order
(include/ampis_hip.h and the comments at the top of the two files), and the cases tests/test_infer_tail_ref.py (CPU, against the
oracle) and tests/test_infer_tail_gpu.py (the kernels) share.

paste_ref is exact: every step is one float32 operation, in the order the kernel documents (it rounds each product and sum on its
own, __f*_rn), so run lists are compared without a tolerance.  The other references are float64 or plain indexing."""
import math

import numpy as np

F32 = np.float32
MS = 28                          # side of the mask-head output
MAX_UNITS = 4096                 # (column, segment) work units a workgroup of paste_rle_seg_kernel holds
SCALE_CLAMP = math.log(1000.0 / 16.0)


# ------------------------------------------------------------------------------------------------------------------ paste
def _axis(lo_i, hi_i, lo, hi):
    """Source coordinate of the output pixels [lo_i, hi_i) of a box side [lo, hi): (i0 = floor(c), w1 = c - i0), float32 step by step."""
    pix = np.arange(lo_i, hi_i).astype(F32)
    g = ((pix + F32(0.5) - lo) / (hi - lo)) * F32(2) - F32(1)
    c = ((g + F32(1)) * F32(MS) - F32(1)) / F32(2)
    f = np.floor(c)
    assert g.dtype == F32 and c.dtype == F32
    return f.astype(np.int64), c - f


def _tap(prob, iy, ix):
    """prob[iy, ix] with zero padding; iy [ny, 1], ix [1, nx]."""
    ok = (iy >= 0) & (iy < MS) & (ix >= 0) & (ix < MS)
    return np.where(ok, prob[np.clip(iy, 0, MS - 1), np.clip(ix, 0, MS - 1)], F32(0))


def paste_region(det_box, out_hw, in_hw):
    """detector_postprocess's box and _do_paste_mask's region: (out_box float32 [4], valid, (x0i, y0i, x1i, y1i) or None)."""
    H, W = int(out_hw[0]), int(out_hw[1])
    sx, sy = F32(float(W) / float(in_hw[1])), F32(float(H) / float(in_hw[0]))
    db = np.asarray(det_box, F32)
    x0, y0, x1, y1 = db[0] * sx, db[1] * sy, db[2] * sx, db[3] * sy
    x0, x1 = (np.minimum(np.maximum(v, F32(0)), F32(W)) for v in (x0, x1))
    y0, y1 = (np.minimum(np.maximum(v, F32(0)), F32(H)) for v in (y0, y1))
    out_box = np.array([x0, y0, x1, y1], F32)
    valid = bool((x1 - x0) > 0) and bool((y1 - y0) > 0)
    if not valid:
        return out_box, False, None
    x0i, y0i = max(int(np.floor(x0)) - 1, 0), max(int(np.floor(y0)) - 1, 0)
    x1i, y1i = min(int(np.ceil(x1)) + 1, W), min(int(np.ceil(y1)) + 1, H)
    return out_box, True, (x0i, y0i, x1i, y1i)


def paste_ref(prob, det_box, out_hw, in_hw, thr):
    """One detection: prob [28, 28] float32, det_box in network-input coordinates -> (out_box [4] float32, valid, mask [H, W] bool).
    The run lengths of the mask are oracle.rle.encode_counts(mask)."""
    H, W = int(out_hw[0]), int(out_hw[1])
    prob = np.ascontiguousarray(prob, F32)
    out_box, valid, reg = paste_region(det_box, out_hw, in_hw)
    mask = np.zeros((H, W), bool)
    if not valid:
        return out_box, False, mask
    x0i, y0i, x1i, y1i = reg
    x0, y0, x1, y1 = out_box
    ix, wx = _axis(x0i, x1i, x0, x1)
    iy, wy = _axis(y0i, y1i, y0, y1)
    ix, iy = ix[None, :], iy[:, None]
    w, n = wx[None, :], wy[:, None]
    e, s = F32(1) - w, F32(1) - n
    v = _tap(prob, iy, ix) * (s * e)
    v = v + _tap(prob, iy, ix + 1) * (s * w)
    v = v + _tap(prob, iy + 1, ix) * (n * e)
    v = v + _tap(prob, iy + 1, ix + 1) * (n * w)
    assert v.dtype == F32
    mask[y0i:y1i, x0i:x1i] = v >= F32(thr)
    return out_box, True, mask


def paste_path(nx, ny):
    """How paste_rle_seg_kernel cuts an nx x ny region: dict(SEG rows per segment, nseg segments per column, units, keep_bits,
    path 'a' | 'b' | 'c' | 'd' as the issue's table names them)."""
    nseg = (ny + 31) // 32
    if nseg * nx > MAX_UNITS:
        nseg = max(MAX_UNITS // nx, 1)
    seg = (ny + nseg - 1) // nseg
    nseg = (ny + seg - 1) // seg
    units = nx * nseg
    keep = seg <= 64 and units <= MAX_UNITS
    if nx > MAX_UNITS:
        path = "d"
    elif seg <= 32:
        path = "a"
    elif seg <= 64:
        path = "b"
    else:
        path = "c"
    return dict(SEG=seg, nseg=nseg, units=units, keep_bits=keep, path=path)


def _smooth(rng):
    yy, xx = np.mgrid[0:MS, 0:MS]
    cy, cx, r = rng.uniform(10, 18), rng.uniform(10, 18), rng.uniform(6, 11)
    return (1 / (1 + np.exp(((yy - cy) ** 2 + (xx - cx) ** 2 - r * r) / 8))).astype(F32)


def two_probs(seed):
    """[2, 28, 28] float32: one smooth blob, one mask of uniform noise (many runs)."""
    rng = np.random.default_rng(seed)
    return np.stack([_smooth(rng), rng.uniform(0, 1, (MS, MS)).astype(F32)])


# name, out (H, W), box in output pixels, threshold, (nx, ny) of the region, path ('-' = no region)
PASTE_CASES = [
    ("small", (160, 208), (30.3, 20.6, 120.2, 140.9), 0.5, (93, 123), "a"),
    ("b", (520, 320), (10.5, 8.25, 305.5, 505.75), 0.5, (298, 500), "b"),
    ("b_wrap", (500, 320), (10.5, -3, 305.5, 600), 0.5, (298, 500), "b"),
    ("c", (540, 540), (9.5, 11.25, 525.5, 527.75), 0.5, (519, 519), "c"),
    ("c_wrap", (530, 540), (9.5, 0, 525.5, 530), 0.5, (519, 530), "c"),
    ("d", (24, 4200), (2.5, 3.25, 4190.5, 20.75), 0.5, (4191, 20), "d"),
    ("d_wrap", (24, 4200), (0, 0, 4200, 24), 0.5, (4200, 24), "d"),
    ("tall", (4200, 24), (3.25, 2.5, 20.75, 4190.5), 0.5, (20, 4191), "a"),
    ("bottom", (160, 208), (40.5, 30.25, 100.5, 160), 0.5, (63, 131), "a"),     # bottom on H, top > 1: closing transition at (x+1)*H
    ("bottom_b", (520, 320), (10.5, 8.25, 305.5, 520), 0.5, (298, 513), "b"),
    ("bottom_c", (540, 540), (9.5, 11.25, 525.5, 540), 0.5, (519, 530), "c"),
    ("right", (160, 208), (197.7, 20.7, 213, 70.2), 0.5, (12, 53), "a"),          # touches the right border
    ("corner", (160, 208), (150.5, 100.5, 208, 160), 0.5, (59, 61), "a"),         # right border and bottom: no closing transition
    ("pixel", (160, 208), (50.3, 60.3, 50.7, 60.7), 0.5, (3, 3), "a"),            # inside one pixel
    ("empty", (160, 208), (50, 60, 50, 90), 0.5, None, "-"),                       # empty after the clip
    ("thr03", (160, 208), (30.3, 20.6, 120.2, 140.9), 0.3, (93, 123), "a"),
    ("thr0", (160, 208), (30.3, 20.6, 120.2, 140.9), 0.0, (93, 123), "a"),         # the whole region is ones
    ("thr0_all", (160, 208), (-5, -5, 300, 300), 0.0, (208, 160), "a"),            # counts [0, H*W]
    ("thr15", (160, 208), (30.3, 20.6, 120.2, 140.9), 1.5, (93, 123), "a"),        # counts [H*W]
    ("thr15_all", (160, 208), (-5, -5, 300, 300), 1.5, (208, 160), "a"),
]
PASTE_IDS = [c[0] for c in PASTE_CASES]


def paste_case_inputs(i):
    """Case i of PASTE_CASES as a launch: (prob [2,28,28], boxes [2,4] float32 (the box twice), (H, W), thr)."""
    _, hw, box, thr, _, _ = PASTE_CASES[i]
    return two_probs(100 + i), np.tile(np.asarray(box, F32), (2, 1)), hw, thr


def multi_image_case():
    """Detections of three images with different output sizes and non-dyadic scales in one launch:
    dict(prob [N,28,28], boxes [N,4] in network-input coordinates, batch [N], out_hw [3,2], in_hw [3,2], in_common (h, w))."""
    rng = np.random.default_rng(77)
    out_hw = np.array([[150, 203], [97, 64], [200, 131]], np.int32)
    in_hw = np.array([[256, 320], [224, 160], [192, 136]], np.int32)
    per, boxes, batch = 5, [], []
    for b in range(3):
        h, w = in_hw[b]
        ctr = rng.uniform(0.2, 0.8, (per, 2)) * np.array([w, h])
        size = np.exp(rng.uniform(np.log(6), np.log(0.9 * min(h, w)), (per, 2)))
        bb = np.concatenate([ctr - size / 2, ctr + size / 2], 1)
        bb[0] = [-3, -2, w + 10, h + 9]                # the whole image
        bb[1] = [w * 0.25, 0, w * 0.5, h]              # full-height columns
        if b == 1:
            bb[2] = [w + 2, 10, w + 30, 40]            # empty after the clip
        boxes.append(bb)
        batch += [b] * per
    boxes, batch = np.concatenate(boxes).astype(F32), np.array(batch, np.int32)
    order = rng.permutation(len(batch))                # detections of the images interleaved
    boxes, batch = boxes[order], batch[order]
    prob = np.stack([two_probs(500 + i)[i % 2] for i in range(len(batch))])
    return dict(prob=prob, boxes=boxes, batch=batch, out_hw=out_hw, in_hw=in_hw, in_common=(256, 320))


def paste_many_ref(prob, boxes, batch, out_hw, in_hw, thr):
    """paste_ref per detection; in_hw [B, 2] or one (h, w) for every image.  Returns (out_boxes [N,4], valid [N] bool, masks list)."""
    in_hw = np.asarray(in_hw)
    obs, vs, ms = [], [], []
    for i in range(len(prob)):
        b = int(batch[i])
        ob, v, m = paste_ref(prob[i], boxes[i], out_hw[b], in_hw[b] if in_hw.ndim == 2 else in_hw, thr)
        obs.append(ob), vs.append(v), ms.append(m)
    return np.stack(obs), np.array(vs), ms


# ------------------------------------------------------------------------------------------------------------------ detection tail
def mask_prob_ref(logits, classes):
    """logits [N, 28, 28, K], classes [N] -> float64 sigmoid of channel classes[n]; a class outside [0, K) reads channel 0."""
    logits = np.asarray(logits, np.float64)
    N, K = logits.shape[0], logits.shape[-1]
    c = np.asarray(classes).astype(np.int64)
    c = np.where((c >= 0) & (c < K), c, 0)
    x = logits[np.arange(N), :, :, c]
    return 1.0 / (1.0 + np.exp(-x))


def box_candidates_ref(pred, proposals, prop_count, K, score_thresh, img_hw, weights=(10., 10., 5., 5.)):
    """pred [B, Rcap, ld] (columns [0, K] class logits with the background last, then 4 K deltas), proposals [B, Rcap, 4],
    img_hw [B, 2].  float64.  Per image: dict(boxes [Rcap, K, 4] decoded and clipped (rows >= prop_count are NaN), finite [Rcap] bool
    (a row with a non-finite probability or box is no candidate in any class), probs [Rcap, K], cand = sorted list of (r*K + k, k))."""
    pred, proposals = np.asarray(pred, np.float64), np.asarray(proposals, np.float64)
    B, Rcap = proposals.shape[:2]
    out = []
    with np.errstate(all="ignore"):
        for b in range(B):
            n = int(prop_count[b])
            logit, delta = pred[b, :, :K + 1], pred[b, :, K + 1:K + 1 + 4 * K].reshape(Rcap, K, 4)
            ex = np.exp(logit - logit.max(1, keepdims=True))
            probs = ex / ex.sum(1, keepdims=True)
            p = proposals[b]
            w, h = (p[:, 2] - p[:, 0])[:, None], (p[:, 3] - p[:, 1])[:, None]
            cx, cy = p[:, 0:1] + 0.5 * w, p[:, 1:2] + 0.5 * h
            dx, dy = delta[..., 0] / weights[0], delta[..., 1] / weights[1]
            dw, dh = np.minimum(delta[..., 2] / weights[2], SCALE_CLAMP), np.minimum(delta[..., 3] / weights[3], SCALE_CLAMP)
            pcx, pcy, pw, ph = dx * w + cx, dy * h + cy, np.exp(dw) * w, np.exp(dh) * h
            raw = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)
            finite = np.isfinite(raw).all((1, 2)) & np.isfinite(probs).all(1)
            H, W = float(img_hw[b][0]), float(img_hw[b][1])
            boxes = np.stack([np.clip(raw[..., 0], 0, W), np.clip(raw[..., 1], 0, H), np.clip(raw[..., 2], 0, W),
                              np.clip(raw[..., 3], 0, H)], -1)
            live = np.arange(Rcap) < n
            boxes[~live] = np.nan
            take = (probs[:, :K] > score_thresh) & (finite & live)[:, None]
            rr, kk = np.nonzero(take)
            out.append(dict(boxes=boxes, finite=finite & live, probs=probs[:, :K], cand=[(int(r) * K + int(k), int(k)) for r, k in zip(rr, kk)]))
    return out


def decode_sortkeys(keys):
    """csrc/common.h make_sortkey backwards (make_sortkeys in tests/test_rpn_nms_levels_gpu.py is the forward direction):
    64-bit words -> (score float32, position, category, used), used = the word is not 0."""
    k = np.ascontiguousarray(keys).view(np.uint64)
    o = (k >> np.uint64(32)).astype(np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o).astype(np.uint32)
    pos = (np.uint64(0xffffff) - ((k >> np.uint64(8)) & np.uint64(0xffffff))).astype(np.int64)
    return u.view(F32), pos, (k & np.uint64(0xff)).astype(np.int64), k != 0


def gather_dets_ref(sboxes, sscores, scats, keep_idx, keep_count, D, payload=None):
    """Rows keep_idx[b, :keep_count[b]] of the sorted candidates; the rows from keep_count[b] on are zeros, class and payload -1.
    Returns (boxes [B,D,4], scores [B,D], classes [B,D], payload [B,D] or None) with the source's bits."""
    B = sboxes.shape[0]
    ob, os_ = np.zeros((B, D, 4), sboxes.dtype), np.zeros((B, D), sscores.dtype)
    oc = np.full((B, D), -1, np.int32)
    op = np.full((B, D), -1, np.int32) if payload is not None else None
    for b in range(B):
        idx = keep_idx[b, :keep_count[b]]
        ob[b, :len(idx)], os_[b, :len(idx)], oc[b, :len(idx)] = sboxes[b, idx], sscores[b, idx], scats[b, idx]
        if payload is not None:
            op[b, :len(idx)] = payload[b, idx]
    return ob, os_, oc, op


def compact_dets_ref(det_count, det_boxes, det_scores, det_classes):
    """The first min(det_count[b], D) detections of every image, in image order: (boxes [T,4], scores [T], classes [T], batch [T])."""
    B, D = det_scores.shape
    n = np.minimum(np.asarray(det_count), D)
    sel = [(b, i) for b in range(B) for i in range(int(n[b]))]
    bi, ii = np.array([s[0] for s in sel], np.int64), np.array([s[1] for s in sel], np.int64)
    return det_boxes[bi, ii], det_scores[bi, ii], det_classes[bi, ii], bi.astype(np.int32)


def box_inputs(seed, B, Rcap, K, ld, H, W, counts):
    """Box-head outputs and proposals for box_candidates: (pred [B, Rcap, ld] float32, proposals [B, Rcap, 4] float32, counts int32)."""
    rng = np.random.default_rng(seed)
    pred = rng.normal(0, 1.5, (B, Rcap, ld)).astype(F32)
    pred[:, :, K + 1:] *= 0.5
    ctr = rng.uniform(0, 1, (B, Rcap, 2)) * np.array([W, H])
    size = rng.uniform(8, 120, (B, Rcap, 2))
    props = np.clip(np.concatenate([ctr - size / 2, ctr + size / 2], 2), 0, [W, H, W, H]).astype(F32)
    return pred, props, np.asarray(counts, np.int32)


# name -> (seed, B, Rcap, K, ld, (H, W) common clip size, per-image clip sizes or None, prop counts, score threshold).  The seeds are
# chosen so that no reference score lies within 1e-5 of the threshold (tests/test_infer_tail_ref.py asserts it): membership in the
# candidate set is then no rounding question.  Rcap is no multiple of 64, so waves straddle images.
BOX_CASES = {
    "k3": (11, 3, 100, 3, 16, (300, 400), None, (100, 0, 63), 0.05),                  # prop_count 0, a ragged count
    "k1_wide_ld": (12, 2, 67, 1, 8, (300, 400), None, (67, 41), 0.5),               # ld wider than 5K + 1
    "k80": (25, 1, 130, 80, 401, (300, 400), None, (130,), 0.02),
    "sized": (14, 3, 100, 3, 16, (300, 400), ((300, 400), (150, 210), (77, 390)), (100, 100, 90), 0.05),
}


def box_case(name):
    """-> dict(pred, props, counts, K, thr, hw (common), img_hw [B,2] the clip size of each image, sized (img_hw is per image))."""
    seed, B, Rcap, K, ld, hw, sized, counts, thr = BOX_CASES[name]
    pred, props, counts = box_inputs(seed, B, Rcap, K, ld, hw[0], hw[1], counts)
    img_hw = np.array(sized if sized else [hw] * B, np.int32)
    return dict(pred=pred, props=props, counts=counts, K=K, thr=thr, hw=hw, img_hw=img_hw, sized=sized is not None)


def nonfinite_case():
    """k3's shape with rows the finite filter must drop for all K classes: (case dict, bad rows as (image, row))."""
    c = box_case("k3")
    c["counts"] = np.array([100, 100, 63], np.int32)
    K = c["K"]
    c["pred"][:, :, :K] += 1.0                              # most rows have a class above the threshold
    c["pred"][0, 5, 1] = np.nan                             # NaN logit
    c["pred"][0, 64, K] = np.inf                            # +inf logit (the wave after row 63)
    c["pred"][1, 27, K + 1 + 4 * 2] = np.inf                # inf dx of class 2: the whole row goes
    c["props"][2, 36, 2] = np.nan                           # NaN proposal
    c["pred"][2, 70, 0] = np.nan                            # beyond prop_count anyway
    return c, [(0, 5), (0, 64), (1, 27), (2, 36)]


def overflow_case():
    """ccap = 64 with a low threshold: image 0 has several hundred candidates, image 1 fewer than 64."""
    pred, props, counts = box_inputs(21, 2, 200, 3, 16, 300, 400, (200, 15))
    return dict(pred=pred, props=props, counts=counts, K=3, thr=0.01, hw=(300, 400), img_hw=np.array([[300, 400]] * 2, np.int32),
                sized=False, ccap=64)
