"""COCO RLE codec on the C ABI (amp_rle_* of libampis_hip.so, host C++): the drop-in for the pycocotools.mask
calls AMPIS makes around the hot path (ampis/data_utils.py:275; ampis/analyze.py:108,158,315-321;
ampis/structures.py:465-468,568,752).  RLE dicts are pycocotools' compressed form {'size':[h,w], 'counts': bytes}."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def _vp(a):
    """A numpy array as the void pointer of a C call."""
    return a.ctypes.data_as(C.c_void_p)


def _handle(ctx):
    """The amp_ctx of a _lib.Context, NULL for None (the host path)."""
    return ctx.handle if ctx is not None else None


def counts_to_string(cnts):
    cnts = np.ascontiguousarray(cnts, dtype=np.uint32)
    cap = 7 * len(cnts) + 8
    buf = C.create_string_buffer(cap)
    n = C.c_size_t()
    check(lib().amp_rle_to_string(cnts.ctypes.data_as(C.c_void_p), len(cnts), buf, cap, C.byref(n)), "amp_rle_to_string")
    return buf.raw[: n.value]


def counts_to_strings(pool, off, ln):
    """RLE strings of many masks in one call: mask i = pool[off[i] : off[i] + ln[i]] (uint32 run lengths)."""
    n = len(off)
    if n == 0:
        return []
    pool = np.ascontiguousarray(pool, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ln = np.ascontiguousarray(ln, dtype=np.int32)
    cap = 7 * int(ln.sum()) + 8 * n + 8
    buf = C.create_string_buffer(cap)
    so = np.zeros(n + 1, dtype=np.uintp)
    check(lib().amp_rle_to_strings(pool.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), n,
                                   buf, cap, so.ctypes.data_as(C.c_void_p)), "amp_rle_to_strings")
    raw = buf.raw
    so = so.tolist()
    return [raw[so[i]: so[i + 1]] for i in range(n)]


def string_to_counts(s):
    if isinstance(s, str):
        s = s.encode("ascii")
    out = np.empty(len(s) + 1, dtype=np.uint32)
    m = C.c_int()
    check(lib().amp_rle_from_string(C.c_char_p(s), len(s), out.ctypes.data_as(C.c_void_p), len(out), C.byref(m)),
          "amp_rle_from_string")
    return out[: m.value].copy()


def _counts(r):
    c = r["counts"]
    return string_to_counts(c) if isinstance(c, (bytes, str)) else np.ascontiguousarray(c, dtype=np.uint32)


def encode(mask):
    """mask: [H,W] (or [H,W,N]) bool/uint8 -> RLE dict (or list), like pycocotools.mask.encode."""
    mask = np.asarray(mask)
    if mask.ndim == 3:
        return [encode(mask[:, :, i]) for i in range(mask.shape[2])]
    h, w = mask.shape
    f = np.asfortranarray(mask.astype(np.uint8))
    cap = h * w + 2
    out = np.empty(cap, dtype=np.uint32)
    m = C.c_int()
    check(lib().amp_rle_encode(f.ctypes.data_as(C.c_void_p), h, w, out.ctypes.data_as(C.c_void_p), cap, C.byref(m)),
          "amp_rle_encode")
    return {"size": [h, w], "counts": counts_to_string(out[: m.value])}


def decode(r):
    if isinstance(r, (list, tuple)):
        return np.stack([decode(x) for x in r], axis=2)
    h, w = r["size"]
    c = _counts(r)
    out = np.empty((h, w), dtype=np.uint8, order="F")
    check(lib().amp_rle_decode(c.ctypes.data_as(C.c_void_p), len(c), h, w, out.ctypes.data_as(C.c_void_p)), "amp_rle_decode")
    return out


def area(r):
    if isinstance(r, (list, tuple)):
        return np.array([area(x) for x in r], dtype=np.uint32)
    c = _counts(r)
    a = C.c_ulonglong()
    check(lib().amp_rle_area(c.ctypes.data_as(C.c_void_p), len(c), C.byref(a)), "amp_rle_area")
    return int(a.value)


def _pool(counts_list):
    off = np.zeros(len(counts_list), dtype=np.uint64)
    ln = np.asarray([len(c) for c in counts_list], dtype=np.int32)
    if len(counts_list):
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    pool = np.ascontiguousarray(np.concatenate(counts_list) if len(counts_list) else np.zeros(1, np.uint32), dtype=np.uint32)
    return pool, off, ln


def iou(dt, gt, iscrowd):
    """len(dt) x len(gt) float64 matrix, like pycocotools.mask.iou on RLE lists (one C call: amp_rle_iou_matrix)."""
    out = np.zeros((len(dt), len(gt)), dtype=np.float64)
    if len(dt) == 0 or len(gt) == 0:
        return out
    dp, do, dl = _pool([_counts(x) for x in dt])
    gp, go, gl = _pool([_counts(x) for x in gt])
    crowd = np.ascontiguousarray([int(bool(c)) for c in iscrowd], dtype=np.uint8) if len(iscrowd) else None
    assert crowd is None or len(crowd) == len(gt)
    h = int(dt[0]["size"][0]) if isinstance(dt[0], dict) and "size" in dt[0] else 0
    check(lib().amp_rle_iou_matrix(_vp(dp), _vp(do), _vp(dl), len(dt), _vp(gp), _vp(go), _vp(gl), len(gt),
                                   _vp(crowd) if crowd is not None else None, h, _vp(out)), "amp_rle_iou_matrix")
    return out


def resize_nearest(r, new_h, new_w, flip=False):
    """RLE of flip(PIL.Image.resize(decode(r), (new_w, new_h), NEAREST)) computed on the runs (amp_rle_resize_nearest): what detectron2 does to a
    bitmask annotation under ResizeShortestEdge + RandomFlip, without decoding."""
    h, w = int(r["size"][0]), int(r["size"][1])
    c = _counts(r)
    fn = lambda out, cap, m: lib().amp_rle_resize_nearest(c.ctypes.data_as(C.c_void_p), len(c), h, w, int(new_h), int(new_w), int(bool(flip)),
                                                          out.ctypes.data_as(C.c_void_p), cap, C.byref(m))
    return _resized(fn, "amp_rle_resize_nearest", len(c), w, int(new_h), int(new_w))


def _resized(fn, name, runs, src_w, new_h, new_w):
    cap = 2 * new_w + 2 * runs * max(1, -(-new_w // max(src_w, 1))) + 8      # every source transition repeats for each output column that reads its column
    while True:
        out = np.empty(cap, dtype=np.uint32)
        m = C.c_int()
        st = fn(out, cap, m)
        if st == 0:
            return {"size": [new_h, new_w], "counts": counts_to_string(out[: m.value])}
        if cap >= new_h * new_w + 2:
            check(st, name)
        cap = min(cap * 4, new_h * new_w + 2)


def crop_resize_nearest(r, crop, new_h, new_w, hflip=False, vflip=False):
    """RLE of flips(PIL.Image.resize(decode(r)[y0:y0+ch, x0:x0+cw], (new_w, new_h), NEAREST)) computed on the runs
    (amp_rle_crop_resize_nearest): a bitmask annotation under RandomCrop + ResizeShortestEdge + RandomFlip.  crop = (y0, x0, ch, cw)."""
    h, w = int(r["size"][0]), int(r["size"][1])
    y0, x0, ch, cw = (int(v) for v in crop)
    c = _counts(r)
    fn = lambda out, cap, m: lib().amp_rle_crop_resize_nearest(c.ctypes.data_as(C.c_void_p), len(c), h, w, y0, x0, ch, cw, int(new_h), int(new_w),
                                                               int(bool(hflip)) | 2 * int(bool(vflip)), out.ctypes.data_as(C.c_void_p), cap, C.byref(m))
    return _resized(fn, "amp_rle_crop_resize_nearest", len(c), cw, int(new_h), int(new_w))


def bbox(r):
    """(x0, y0, x1, y1) of the set pixels of a mask, x1 / y1 one past the last (detectron2 BitMasks.get_bounding_boxes); None when empty."""
    h = int(r["size"][0])
    c = _counts(r).astype(np.int64)
    end = np.cumsum(c)
    ln, end = c[1::2], end[1::2]
    keep = ln > 0
    if h <= 0 or not keep.any():
        return None
    a, b = (end - ln)[keep], end[keep] - 1          # first and last pixel of every run of ones, column-major
    xa, xb = a // h, b // h
    one = xa == xb                                  # a run that crosses a column border covers rows 0 and h - 1
    ya = np.where(one, a % h, 0).min()
    yb = np.where(one, b % h, h - 1).max()
    return int(xa.min()), int(ya), int(xb.max()) + 1, int(yb) + 1


def clip_polygons(flat, off, sel, x0, y0, x1, y1):
    """Polygons sel[j] of a pool (polygon i = flat[off[i] : off[i + 1]], flat x,y values) clipped against the rectangle [x0, x1] x [y0, y1]
    in one call (amp_polygon_clip_rect: Sutherland-Hodgman in float64, untranslated).  Returns (out, out_off): result j = out[out_off[j] :
    out_off[j + 1]], empty when nothing with an area is left."""
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    n = len(sel)
    out_off = np.zeros(n + 1, dtype=np.int64)
    if n == 0:
        return np.zeros(0, np.float64), out_off
    assert sel.min() >= 0 and sel.max() < len(off) - 1 and int(off[-1]) <= len(flat)
    cap = int(6 * (off[sel + 1] - off[sel]).sum() + 16 * n)
    out = np.empty(cap, dtype=np.float64)
    check(lib().amp_polygon_clip_rect(_vp(flat), _vp(off), _vp(sel), n, float(x0), float(y0), float(x1), float(y1), _vp(out), cap, _vp(out_off)),
          "amp_polygon_clip_rect")
    return out[: int(out_off[-1])], out_off


def pair_overlap(a, b, pairs):
    """For index pairs (i, j): |a[i] AND b[j]|, |a[i] minus b[j]|, |b[j] minus a[i]| as three int64 arrays, one C call
    (amp_rle_pair_overlap)."""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = len(pairs)
    out = [np.zeros(n, dtype=np.uint64) for _ in range(3)]
    if n:
        ap, ao, al = _pool([_counts(x) for x in a])
        bp, bo, bl = _pool([_counts(x) for x in b])
        assert pairs[:, 0].max() < len(a) and pairs[:, 1].max() < len(b) and pairs.min() >= 0
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        check(lib().amp_rle_pair_overlap(_vp(ap), _vp(ao), _vp(al), _vp(bp), _vp(bo), _vp(bl), _vp(pa), _vp(pb), n, _vp(out[0]), _vp(out[1]), _vp(out[2])),
              "amp_rle_pair_overlap")
    return tuple(o.astype(np.int64) for o in out)


def edge_distance(gt, pred, pairs, boxes, ctx=None):
    """mask_edge_distance on run lists, one C call (amp_mask_edge_distance): for index pairs (g, p) and one merged index box [r1, r2, c1, c2]
    per pair (the crop [r1:r2, c1:c2]), two lists of uint32 arrays -- for every crop pixel of pred[p] & ~gt[g] in row-major order the SQUARED
    distance to the nearest crop pixel of gt[g], and for every pixel of gt[g] & ~pred[p] to the nearest of pred[p].  ctx: a _lib.Context
    (computed on its device) or None (on the host).  ValueError when a pair has such pixels and the other mask has none in the crop."""
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
    n = len(pairs)
    assert len(boxes) == n, "one box per pair"
    if n == 0:
        return [], []
    assert pairs.min() >= 0 and pairs[:, 0].max() < len(gt) and pairs[:, 1].max() < len(pred)
    h, w = (int(v) for v in gt[int(pairs[0, 0])]["size"])
    gc, pc = [_counts(x) for x in gt], [_counts(x) for x in pred]
    gp, go, gl = _pool(gc)
    pp, po, pl = _pool(pc)
    pg, pq = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    ga = np.array([int(c[1::2].sum(dtype=np.uint64)) for c in gc], dtype=np.uint64)       # amp_rle_area of every mask
    pa = np.array([int(c[1::2].sum(dtype=np.uint64)) for c in pc], dtype=np.uint64)
    fp_cap, fn_cap = int(pa[pq].sum()), int(ga[pg].sum())                                 # a pair has no more queries than its mask has pixels
    fp, fn = np.empty(max(fp_cap, 1), dtype=np.uint32), np.empty(max(fn_cap, 1), dtype=np.uint32)
    fpo, fno = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    check(lib().amp_mask_edge_distance(_handle(ctx), _vp(gp), _vp(go), _vp(gl), len(gc), _vp(pp), _vp(po), _vp(pl), len(pc),
                                       _vp(pg), _vp(pq), _vp(boxes), n, h, w, _vp(fp), fp_cap, _vp(fpo), _vp(fn), fn_cap, _vp(fno)), "amp_mask_edge_distance")
    out = ([fp[int(fpo[i]): int(fpo[i + 1])].copy() for i in range(n)], [fn[int(fno[i]): int(fno[i + 1])].copy() for i in range(n)])
    for name, lst in (("ground-truth", out[0]), ("predicted", out[1])):
        for i, d in enumerate(lst):
            if len(d) and d[0] == 0xFFFFFFFF:
                raise ValueError(f"mask_edge_distance: pair {i} (gt {int(pg[i])}, pred {int(pq[i])}) has no {name} pixel inside its box "
                                 f"{boxes[i].tolist()} to measure a distance to")
    return out


def region_props(masks, ctx=None):
    """Region properties of RLE dicts of one image size, one C call (amp_mask_region_props): (bbox, vals) = int64 [n, 4] boxes (rmin, cmin,
    rmax + 1, cmax + 1) and uint64 [n, 13] exact integers {N, sum r, sum c, sum r^2, sum r c, sum c^2, P1, P2, P3, convex area, 0, 0, 0}; all
    zero for an empty mask.  ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    n = len(masks)
    bbox, vals = np.zeros((n, 4), dtype=np.int64), np.zeros((n, 13), dtype=np.uint64)
    h, w = (int(v) for v in masks[0]["size"]) if n else (1, 1)
    pool, off, ln = _pool([_counts(x) for x in masks])
    check(lib().amp_mask_region_props(_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, _vp(bbox), _vp(vals)),
          "amp_mask_region_props")
    return bbox, vals


def overlap_groups(a_groups, b_groups, ctx=None):
    """All-pairs intersection inside groups, one C call (amp_rle_overlap_groups): a_groups, b_groups are equally long lists of lists of RLE
    dicts, group g = the masks of one image.  Returns (inters, areas_a, areas_b): lists of int64 arrays, inters[g][i, j] = the pixels of
    a_groups[g][i] AND b_groups[g][j] ([na_g, nb_g]), areas_a[g][i] / areas_b[g][j] the pixels of each mask.  Pairs across groups are never
    formed; a group without masks on one side has no image size of its own and gives empty arrays.  ctx: a _lib.Context (computed on its
    device) or None (on the host): the same bytes."""
    assert len(a_groups) == len(b_groups), "one list of B masks per list of A masks"
    ng = len(a_groups)
    na, nb = [len(x) for x in a_groups], [len(x) for x in b_groups]
    gh, gw = np.ones(max(ng, 1), dtype=np.int32), np.ones(max(ng, 1), dtype=np.int32)
    for g in range(ng):
        sizes = {tuple(int(v) for v in r["size"]) for r in list(a_groups[g]) + list(b_groups[g])}
        if len(sizes) > 1:
            raise ValueError(f"overlap_groups: group {g} holds masks of different sizes {sorted(sizes)}")
        if sizes:
            gh[g], gw[g] = sizes.pop()
    af, bf = np.zeros(ng + 1, dtype=np.int32), np.zeros(ng + 1, dtype=np.int32)
    af[1:], bf[1:] = np.cumsum(na), np.cumsum(nb)
    ap, ao, al = _pool([_counts(x) for grp in a_groups for x in grp])
    bp, bo, bl = _pool([_counts(x) for grp in b_groups for x in grp])
    first = np.zeros(ng + 1, dtype=np.int64)
    first[1:] = np.cumsum(np.asarray(na, dtype=np.int64) * np.asarray(nb, dtype=np.int64))
    total = int(first[-1])
    inter = np.zeros(max(total, 1), dtype=np.uint32)
    area_a, area_b = np.zeros(max(int(af[-1]), 1), dtype=np.uint64), np.zeros(max(int(bf[-1]), 1), dtype=np.uint64)
    check(lib().amp_rle_overlap_groups(_handle(ctx), _vp(ap), _vp(ao), _vp(al), _vp(bp), _vp(bo), _vp(bl), _vp(af), _vp(bf),
                                       _vp(gh), _vp(gw), ng, _vp(inter), total, _vp(area_a), _vp(area_b)), "amp_rle_overlap_groups")
    inters = [inter[int(first[g]): int(first[g + 1])].astype(np.int64).reshape(na[g], nb[g]) for g in range(ng)]
    return (inters, [area_a[int(af[g]): int(af[g + 1])].astype(np.int64) for g in range(ng)],
            [area_b[int(bf[g]): int(bf[g + 1])].astype(np.int64) for g in range(ng)])


def seg_class_map(gt, pred, pairs, mode, ctx=None, size=None):
    """Pixel classes of one image from matched pairs, one C call (amp_seg_class_map): for index pairs (g, p), TP = OR (gt[g] & pred[p]),
    FN = OR (gt[g] & ~pred[p]), FP = OR (~gt[g] & pred[p]) and code = TP + 2 FN + 4 FP.  mode 'all' (or 1): the 7 classes code == 1 .. 7;
    'reduced' (or 0): the 4 classes code == 1, 2, 4 and code in {3, 5, 6, 7}.  Returns (class_counts, pixel_counts): a list of K uint32 run lists
    over the whole image (column-major, COCO order) and an int64 [8] array of the pixels of every code.  size=(h, w): the image size when there
    is no pair to take it from.  ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    m = {"reduced": 0, "all": 1, 0: 0, 1: 1}.get(mode if not isinstance(mode, str) else mode.lower())
    if m is None:
        raise ValueError(f"seg_class_map: mode = {mode!r} ('reduced' or 'all')")
    K = 7 if m else 4
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n = len(pairs)
    if n:
        assert pairs.min() >= 0 and pairs[:, 0].max() < len(gt) and pairs[:, 1].max() < len(pred)
        h, w = (int(v) for v in gt[int(pairs[0, 0])]["size"])
    else:
        assert size is not None, "size=(height, width) is required when there is no pair"
        h, w = (int(v) for v in size)
    named_g, named_p = sorted(set(pairs[:, 0].tolist())), sorted(set(pairs[:, 1].tolist()))
    empty = np.zeros(0, np.uint32)                                  # masks no pair names are never read: they need not even be decoded
    gc = [empty] * len(gt)
    pc = [empty] * len(pred)
    for i in named_g:
        gc[i] = _counts(gt[i])
    for i in named_p:
        pc[i] = _counts(pred[i])
    gp, go, gl = _pool(gc)
    pp, po, pl = _pool(pc)
    pg, pq = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    cap = K * (1 + sum(len(gc[i]) - 1 for i in named_g) + sum(len(pc[i]) - 1 for i in named_p))      # what amp_seg_class_map asks for
    counts = np.empty(max(cap, K), dtype=np.uint32)
    coff, pixels = np.zeros(K + 1, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    check(lib().amp_seg_class_map(_handle(ctx), _vp(gp), _vp(go), _vp(gl), len(gc), _vp(pp), _vp(po), _vp(pl), len(pc),
                                  _vp(pg), _vp(pq), n, h, w, m, _vp(counts), len(counts), _vp(coff), _vp(pixels)), "amp_seg_class_map")
    return [counts[int(coff[k]): int(coff[k + 1])].copy() for k in range(K)], pixels.astype(np.int64)


def render_instances(image, masks, tables, edge_rgb, boxes, box_rgb, lw, ctx=None):
    """Instance overlays of one image, one C call (amp_render_instances): image uint8 [h, w, 3]; per instance in draw order masks[i] (RLE dicts
    of the image's size; None: no masks), tables[i] uint8 [256, 3] (a mask pixel holding v in channel c becomes tables[i][v][c]), edge_rgb[i]
    uint8 [3] for the mask's edge pixels (None: no edges), boxes[i] int (x0, y0, x1, y1) inside the image (None: no boxes) framed lw pixels wide
    in box_rgb[i].  Returns the drawn uint8 [h, w, 3] array; the image is not written.  ctx: a _lib.Context (drawn on its device) or None (on
    the host): the same bytes."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3, f"an [h, w, 3] image is required, got shape {img.shape}"
    h, w = img.shape[:2]
    n = len(masks) if masks is not None else (len(boxes) if boxes is not None else 0)
    pool = off = ln = tab = edge = bx = brgb = None
    if masks is not None:
        for i, r in enumerate(masks):
            if tuple(int(v) for v in r["size"]) != (h, w):
                raise ValueError(f"render_instances: mask {i} has size {list(r['size'])}, the image {[h, w]}")
        pool, off, ln = _pool([_counts(x) for x in masks])
        tab = np.ascontiguousarray(tables, dtype=np.uint8).reshape(-1, 256, 3)
        assert len(tab) == n, "one fill table per mask"
        if edge_rgb is not None:
            edge = np.ascontiguousarray(edge_rgb, dtype=np.uint8).reshape(-1, 3)
            assert len(edge) == n, "one edge colour per mask"
    if boxes is not None:
        bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        brgb = np.ascontiguousarray(box_rgb, dtype=np.uint8).reshape(-1, 3)
        assert len(bx) == n and len(brgb) == n, "one box and one box colour per instance"
    out = np.empty_like(img)
    opt = lambda a: _vp(a) if a is not None else None
    check(lib().amp_render_instances(_handle(ctx), _vp(img), h, w, opt(pool), opt(off), opt(ln), n, opt(tab), opt(edge), opt(bx), opt(brgb),
                                     int(lw), _vp(out)), "amp_render_instances")
    return out


LABEL_KINDS = {"binary": 0, "label": 1}


def label_runs(image, kind, connectivity=2, zero_is_background=True, ctx=None, return_labels=False):
    """The instances of an annotation image as run lists, at most two C calls (amp_label_runs: the first reports the capacities when the guess
    was too small).  image: 2-D; kind 'binary' (uint8, nonzero is foreground: the connected components, connectivity 1 = 4 neighbours, 2 = 8,
    numbered by the row-major position of their first pixel) or 'label' (int32 ids: one instance per distinct id in ascending order, id 0 skipped
    when zero_is_background).  Returns (ids int32 [N], boxes int32 [N, 4] {r0, c0, r1, c1} ends exclusive, areas uint32 [N], pool, off, len) --
    instance i's COCO counts are pool[off[i] : off[i] + len[i]] -- and the int32 label image (instance number, 0 elsewhere) when return_labels.
    ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    k = LABEL_KINDS.get(kind if not isinstance(kind, str) else kind.lower())
    if k is None:
        raise ValueError(f"label_runs: kind = {kind!r} ('binary' or 'label')")
    img = np.ascontiguousarray(image, dtype=np.int32 if k else np.uint8)
    if img.ndim != 2:
        raise ValueError(f"label_runs: a 2-D image is required, got shape {img.shape}")
    h, w = img.shape
    labels = np.empty((h, w), dtype=np.int32) if return_labels else None
    need = np.zeros(2, dtype=np.uint64)
    icap, ccap = 1024, 4 * (h + w) + 4096
    for attempt in range(2):
        ids, boxes, areas = np.empty(icap, np.int32), np.empty((icap, 4), np.int32), np.empty(icap, np.uint32)
        pool, off, ln = np.empty(ccap, np.uint32), np.empty(icap, np.uint64), np.empty(icap, np.int32)
        st = lib().amp_label_runs(_handle(ctx), _vp(img), h, w, k, int(connectivity), int(bool(zero_is_background)), _vp(ids), _vp(boxes),
                                  _vp(areas), _vp(pool), _vp(off), _vp(ln), icap, ccap, _vp(labels) if return_labels else None, _vp(need))
        if st != -3 or attempt:                                     # AMP_ERR_NOMEM the first time: the needs are known now
            check(st, "amp_label_runs")
            break
        icap, ccap = max(int(need[0]), 1), max(int(need[1]), 1)
    n, total = int(need[0]), int(need[1])
    out = (ids[:n], boxes[:n], areas[:n], pool[:total], off[:n], ln[:n])
    return out + (labels,) if return_labels else out


def polygons_to_rle(instances, h, w, ctx=None, return_boxes=False):
    """The polygon instances of one image as RLE dicts, one C call (amp_polygons_to_rle; a second one when the first reports that the capacity
    guess was too small) and one counts_to_strings: instances[i] is the list of instance i's polygons, a polygon flat [x0, y0, x1, y1, ...].
    Instance i's mask is what merge(frPyObjects(instances[i], h, w)) gives, byte for byte.  return_boxes: also the int32 [n, 4] tight boxes
    {r0, c0, r1, c1} (ends exclusive, zeros for an empty mask) and the uint32 [n] areas of those masks.  A coordinate that is not finite or
    exceeds 10^6 in magnitude is refused (AmpError), like every other malformed argument.  ctx: a _lib.Context (computed on its device) or
    None (on the host): the same bytes."""
    h, w = int(h), int(w)
    n = len(instances)
    flat = [np.asarray(p, dtype=np.float64).reshape(-1) for inst in instances for p in inst]
    first = np.zeros(n + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(inst) for inst in instances], dtype=np.int64)
    poff = np.zeros(len(flat) + 1, dtype=np.uint64)
    poff[1:] = np.cumsum([len(p) for p in flat], dtype=np.uint64)
    xy = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(1, np.float64), dtype=np.float64)
    boxes, areas = np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.uint32)
    off, ln = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32)
    need = np.zeros(1, dtype=np.uint64)
    cap = 2 * n + len(xy) + 4096                                    # a guess: two boundaries for every vertex
    for attempt in range(2):
        pool = np.empty(cap, dtype=np.uint32)
        st = lib().amp_polygons_to_rle(_handle(ctx), _vp(xy), _vp(poff), _vp(first), n, h, w, _vp(pool), cap, _vp(off), _vp(ln), _vp(boxes),
                                       _vp(areas), _vp(need))
        if st != -3 or attempt:                                     # AMP_ERR_NOMEM the first time: the need is known now
            check(st, "amp_polygons_to_rle")
            break
        cap = max(int(need[0]), 1)
    strings = counts_to_strings(pool[: int(need[0])], off[:n], ln[:n])
    out = [{"size": [h, w], "counts": c} for c in strings]
    return (out, boxes, areas) if return_boxes else out


MASK_PARTS_ALL = 0xFFFFFFFF


def mask_parts(masks, colour, connectivity=2, threshold=0, keep_largest=False, ctx=None, emit=True):
    """Connected components per mask for RLE dicts of one image size, one C call (amp_mask_parts; a second one when the first reports that the
    capacity was too small).  colour 1: the parts -- components of the ones, connectivity 1 = 4 neighbours, 2 = 8; with keep_largest every part
    but the largest (ties: the first in column-major order) and then every part of area < threshold is removed.  colour 0: the holes --
    components of the zeros under the dual neighbourhood that do not touch the border of the mask's tight box; every hole of area < threshold
    is filled, threshold None fills all.  Returns (stats, counts): stats int64 [n, 4] = {components, their pixels, the largest component's
    pixels, the pixels flipped} and the list of the results' canonical uint32 counts arrays (None when emit is false: statistics only).
    ValueError for masks of different sizes.  ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    n = len(masks)
    sizes = {tuple(int(v) for v in r["size"]) for r in masks}
    if len(sizes) > 1:
        raise ValueError(f"mask_parts: masks of different sizes {sorted(sizes)}")
    stats = np.zeros((n, 4), dtype=np.uint64)
    if n == 0:
        return stats.astype(np.int64), ([] if emit else None)
    h, w = sizes.pop()
    thr = MASK_PARTS_ALL if threshold is None else min(int(threshold), MASK_PARTS_ALL)
    pool, off, ln = _pool([_counts(x) for x in masks])
    args = (_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, int(colour), int(connectivity), thr, int(bool(keep_largest)), _vp(stats))
    if not emit:
        check(lib().amp_mask_parts(*args, None, 0, None, None, None), "amp_mask_parts")
        return stats.astype(np.int64), None
    out_off, out_len, need = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32), np.zeros(1, dtype=np.uint64)
    cap = int(ln.sum()) + n * (w + 1)                               # always enough: a tight box is no wider than the image
    for attempt in range(2):
        out = np.empty(cap, dtype=np.uint32)
        st = lib().amp_mask_parts(*args, _vp(out), cap, _vp(out_off), _vp(out_len), _vp(need))
        if st != -3 or attempt:                                     # AMP_ERR_NOMEM the first time: the need is known now
            check(st, "amp_mask_parts")
            break
        cap = max(int(need[0]), 1)
    return stats.astype(np.int64), [out[int(o): int(o) + int(k)].copy() for o, k in zip(out_off, out_len)]


def flatten_instances(masks, rank=None, ctx=None, emit=True, return_labels=False, size=None):
    """Which instance a pixel belongs to, for RLE dicts of one image size that may overlap, in ONE C call (amp_flatten_instances; the capacity
    2 x the input counts always suffices).  The owner of a pixel is the covering instance of smallest rank[i], among equals of smallest index;
    rank None is index order, any uint32 values are valid.  Returns (stats, boxes, pixels, counts) and, with return_labels, the int32 [h, w]
    label image of owner + 1 (0: no owner): stats int64 [n, 2] = {area of the input mask, pixels owned}, boxes int64 [n, 4] = {r0, c0, r1, c1}
    of the owned pixels with exclusive ends (zeros when nothing is owned), pixels int64 [3] = the pixels covered by no instance, by one, by two
    or more, counts the list of the visible masks' canonical uint32 counts arrays -- what encode(labels == i + 1) gives; [h * w] for an
    instance that owns nothing -- or None when emit is false.  size=(h, w) is needed only when there is no mask.  ValueError for masks of
    different sizes, a rank of another length or outside uint32.  ctx: a _lib.Context (computed on its device) or None (on the host): the same
    bytes."""
    n = len(masks)
    sizes = {tuple(int(v) for v in r["size"]) for r in masks}
    if size is not None:
        sizes.add((int(size[0]), int(size[1])))
    if len(sizes) > 1:
        raise ValueError(f"flatten_instances: masks of different sizes {sorted(sizes)}")
    if not sizes:
        raise ValueError("flatten_instances: size=(height, width) is required when there is no mask to take it from")
    h, w = sizes.pop()
    rk = None
    if rank is not None:
        r = np.asarray(rank)
        if r.shape != (n,) or not (n == 0 or np.issubdtype(r.dtype, np.integer)):
            raise ValueError(f"flatten_instances: rank must be {n} integers, got shape {r.shape} {r.dtype}")
        if n and (int(r.min()) < 0 or int(r.max()) > 0xFFFFFFFF):
            raise ValueError(f"flatten_instances: ranks {int(r.min())} .. {int(r.max())} do not fit uint32")
        rk = np.ascontiguousarray(r, dtype=np.uint32)
    pool, off, ln = _pool([_counts(x) for x in masks])
    stats, boxes, pixels = np.zeros((n, 2), dtype=np.uint64), np.zeros((n, 4), dtype=np.int32), np.zeros(3, dtype=np.uint64)
    labels = np.empty((h, w), dtype=np.int32) if return_labels else None
    cap = 2 * int(ln.sum()) if emit else 0
    out = np.empty(max(cap, 1), dtype=np.uint32) if emit else None
    out_off, out_len, need = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32), np.zeros(1, dtype=np.uint64)
    opt = lambda a: _vp(a) if a is not None else None
    check(lib().amp_flatten_instances(_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, opt(rk), opt(labels), opt(out), cap, _vp(out_off),
                                      _vp(out_len), _vp(stats), _vp(boxes), _vp(pixels), _vp(need)), "amp_flatten_instances")
    counts = [out[int(o): int(o) + int(k)].copy() for o, k in zip(out_off[:n], out_len[:n])] if emit else None
    res = (stats.astype(np.int64), boxes.astype(np.int64), pixels.astype(np.int64), counts)
    return res + (labels,) if return_labels else res


def mask_contours(masks, connectivity=2, ctx=None, size=None):
    """The boundary rings of RLE dicts of one image size as flat arrays, one C call (amp_mask_contours; a second one when the first reports
    that the capacity guess was too small).  Vertices are integer pixel corners (x, y) -- pixel (r, c) is the square [c, c + 1] x [r, r + 1],
    the coordinates of polygons_to_rle --, a ring is its corners only, the one on its right hand (outer rings clockwise on screen), starting
    at its smallest corner by x, then y; connectivity 2 joins diagonal ones into one ring, 1 keeps them apart.  Returns (ring_first, ring_off,
    ring_len, ring_area2, ring_length, xy): the rings of mask i are ring_first[i] .. ring_first[i + 1] - 1 (int64 [n + 1]), ring r's corners
    are xy[ring_off[r] : ring_off[r] + ring_len[r]] (xy int32 [vertices, 2]), ring_area2 int64 is the signed shoelace sum (positive: outer ring,
    twice the enclosed pixels; negative: hole), ring_length int64 the crack length.  size=(h, w) is needed only when there is no mask.
    ValueError for masks of different sizes.  ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    n = len(masks)
    sizes = {tuple(int(v) for v in r["size"]) for r in masks}
    if size is not None:
        sizes.add((int(size[0]), int(size[1])))
    if len(sizes) > 1:
        raise ValueError(f"mask_contours: masks of different sizes {sorted(sizes)}")
    if not sizes:
        raise ValueError("mask_contours: size=(height, width) is required when there is no mask to take it from")
    h, w = sizes.pop()
    pool, off, ln = _pool([_counts(x) for x in masks])
    first, need = np.zeros(n + 1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    vcap, rcap = 4 * int(ln.sum()) + 64, int(ln.sum()) + 16        # a guess: a run of ones that stays in its column is one piece
    for attempt in range(2):
        xy = np.empty((vcap, 2), dtype=np.int32)
        r_off, r_len = np.empty(rcap, dtype=np.uint64), np.empty(rcap, dtype=np.int32)
        r_a2, r_length = np.empty(rcap, dtype=np.int64), np.empty(rcap, dtype=np.int64)
        st = lib().amp_mask_contours(_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, int(connectivity), _vp(first), _vp(r_off), _vp(r_len),
                                     _vp(r_a2), _vp(r_length), rcap, _vp(xy), vcap, _vp(need))
        if st != -3 or attempt:                                     # AMP_ERR_NOMEM the first time: the need is known now
            check(st, "amp_mask_contours")
            break
        vcap, rcap = max(int(need[0]), 1), max(int(need[1]), 1)
    nv, nr = int(need[0]), int(need[1])
    return (first.astype(np.int64), r_off[:nr].astype(np.int64), r_len[:nr].astype(np.int64), r_a2[:nr].copy(), r_length[:nr].copy(),
            xy[:nv].copy())


MORPH_OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3, "band_in": 4, "band_out": 5}
MORPH_SHAPES = {"square": 0, "diamond": 1, "disk": 2}
MORPH_MAX_RADIUS = 1024


def morphology(masks, op, shape='disk', radius=1, border_value=0, ctx=None, size=None, return_stats=False):
    """Mask morphology on RLE dicts of one image size, one C call (amp_mask_morphology; a second one when the first reports that the capacity
    guess was too small).  op: 'dilate', 'erode', 'open' (the dilation of the erosion), 'close' (the erosion of the dilation), 'band_in' (the
    mask minus its erosion) or 'band_out' (its dilation minus the mask); shape: 'square' (Chebyshev distance), 'diamond' (city-block) or 'disk'
    (Euclidean, dx^2 + dy^2 <= radius^2); radius: an integer 0 .. 1024; border_value: what an erosion takes the outside of the image for, 0
    (scipy's default: a mask erodes from the image's sides) or 1 (cv2's default).  Returns the list of RLE dicts in canonical form -- what
    encode gives for the dense result --, length and order unchanged; with return_stats also the int64 [n, 4] tight boxes {r0, c0, r1, c1}
    (ends exclusive, zeros for an empty result) and the int64 [n] areas of the results.  radius 0 gives the canonical form of the input (empty
    masks for the bands).  size=(h, w) is needed only when there is no mask.  ValueError for an unknown op or shape, a radius or border value
    out of range and masks of different sizes.  ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    if op not in MORPH_OPS:
        raise ValueError(f"morphology: op = {op!r} (one of {sorted(MORPH_OPS)})")
    if shape not in MORPH_SHAPES:
        raise ValueError(f"morphology: shape = {shape!r} (one of {sorted(MORPH_SHAPES)})")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= MORPH_MAX_RADIUS:
        raise ValueError(f"morphology: radius = {radius!r} (an integer 0 .. {MORPH_MAX_RADIUS})")
    if isinstance(border_value, bool) or border_value not in (0, 1):
        raise ValueError(f"morphology: border_value = {border_value!r} (0 or 1)")
    n = len(masks)
    sizes = {tuple(int(v) for v in r["size"]) for r in masks}
    if size is not None:
        sizes.add((int(size[0]), int(size[1])))
    if len(sizes) > 1:
        raise ValueError(f"morphology: masks of different sizes {sorted(sizes)}")
    boxes, areas = np.zeros((n, 4), dtype=np.int64), np.zeros(n, dtype=np.uint64)
    if n == 0:
        return ([], boxes, areas.astype(np.int64)) if return_stats else []
    h, w = sizes.pop()
    pool, off, ln = _pool([_counts(x) for x in masks])
    out_off, out_len, need = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32), np.zeros(1, dtype=np.uint64)
    cap = 2 * int(ln.sum()) + 64                                    # a guess: a result has about as many runs as its input
    for attempt in range(2):
        out = np.empty(cap, dtype=np.uint32)
        st = lib().amp_mask_morphology(_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, MORPH_OPS[op], MORPH_SHAPES[shape], int(radius),
                                       int(border_value), _vp(out), cap, _vp(out_off), _vp(out_len), _vp(boxes), _vp(areas), _vp(need))
        if st != -3 or attempt:                                     # AMP_ERR_NOMEM the first time: the need is known now
            check(st, "amp_mask_morphology")
            break
        cap = max(int(need[0]), 1)
    res = [{"size": [h, w], "counts": c} for c in counts_to_strings(out[: int(need[0])], out_off, out_len)]
    return (res, boxes, areas.astype(np.int64)) if return_stats else res


DIST_NONE = 0xFFFFFFFF                                              # AMP_DIST_NONE: the squared distance of a pixel of a mask without background
DIST_MAX_CURVE = MORPH_MAX_RADIUS + 1


def mask_distance(masks, border_value=0, ncurve=0, want_map=False, ctx=None, size=None):
    """Exact squared distance maps of RLE dicts of one image size (amp_mask_distance; with want_map a first call that only asks for the
    capacity, which the check answers on the host).  For every pixel of a mask the squared Euclidean distance to the nearest pixel outside it
    -- scipy.ndimage.distance_transform_edt, squared --; border_value 0 counts the pixels just outside the image as background, 1 does not
    (scipy on the undecorated array).  Returns (stats, boxes, curve, maps): stats int64 [n, 4] = {d2_max, pos, sum_d2, area} with pos = col *
    h + row of the first pixel in column-major order that attains d2_max (zeros for an empty mask, {DIST_NONE, 0, 0, h * w} for a mask
    without background); boxes int64 [n, 4] = the tight boxes {r0, c0, r1, c1}, ends exclusive; curve int64 [n, ncurve] = the pixels with
    d2 > r^2 for r = 0 .. ncurve - 1 (ncurve 0 .. 1025); maps = per mask the uint32 [r1 - r0, c1 - c0] squared distances on its box, 0
    outside the mask, or None without want_map.  size=(h, w) is needed only when there is no mask.  ValueError for a bad border value or
    ncurve and masks of different sizes.  ctx: a _lib.Context (computed on its device) or None (on the host): the same bytes."""
    if isinstance(border_value, bool) or border_value not in (0, 1):
        raise ValueError(f"mask_distance: border_value = {border_value!r} (0 or 1)")
    if isinstance(ncurve, bool) or not isinstance(ncurve, (int, np.integer)) or not 0 <= int(ncurve) <= DIST_MAX_CURVE:
        raise ValueError(f"mask_distance: ncurve = {ncurve!r} (an integer 0 .. {DIST_MAX_CURVE})")
    n, ncurve = len(masks), int(ncurve)
    sizes = {tuple(int(v) for v in r["size"]) for r in masks}
    if size is not None:
        sizes.add((int(size[0]), int(size[1])))
    if len(sizes) > 1:
        raise ValueError(f"mask_distance: masks of different sizes {sorted(sizes)}")
    stats, boxes, curve = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.int64), np.zeros((n, ncurve), dtype=np.uint64)
    if n == 0:
        return stats.astype(np.int64), boxes, curve.astype(np.int64), ([] if want_map else None)
    h, w = sizes.pop()
    pool, off, ln = _pool([_counts(x) for x in masks])
    args = (_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, int(border_value), _vp(stats), _vp(boxes), _vp(curve) if ncurve else None, ncurve)
    if not want_map:
        check(lib().amp_mask_distance(*args, None, 0, None, None), "amp_mask_distance")
        return stats.astype(np.int64), boxes, curve.astype(np.int64), None
    map_off, need = np.zeros(n, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    buf = np.empty(1, dtype=np.uint32)
    st = lib().amp_mask_distance(*args, _vp(buf), 0, _vp(map_off), _vp(need))               # the need: refused before any evaluation
    if st == -3:
        buf = np.empty(int(need[0]), dtype=np.uint32)
        st = lib().amp_mask_distance(*args, _vp(buf), int(need[0]), _vp(map_off), _vp(need))
    check(st, "amp_mask_distance")
    maps = [buf[int(o): int(o) + int((b[2] - b[0]) * (b[3] - b[1]))].reshape(int(b[2] - b[0]), int(b[3] - b[1])).copy() for o, b in zip(map_off, boxes)]
    return stats.astype(np.int64), boxes, curve.astype(np.int64), maps


INTENSITY_NVALS = 8                                                 # AMP_INTENSITY_NVALS: {N, sum v, sum v^2, sum r v, sum c v, min, max, 0}
INTENSITY_MAX_BINS = 4096
INTENSITY_CHUNK = 2048                                              # the pixel ranks of one work item of the device path (csrc/mask_intensity.h)


def intensity_image(who, image):
    """The image of a mask_intensity call as the C-contiguous uint8 or uint16 array [h, w, C] the call reads; (array, depth).  bool is read as
    uint8.  ValueError naming the dtype for a float or signed image -- exactness is the point: quantise first -- and for a bad shape."""
    img = np.asarray(image)
    if img.dtype == np.bool_:
        img = img.view(np.uint8)
    if img.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise ValueError(f"{who}: an image of dtype {img.dtype} (uint8, uint16 or bool; quantise a float or signed image first)")
    if img.ndim not in (2, 3) or (img.ndim == 3 and not 1 <= img.shape[2] <= 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"{who}: an image of shape {img.shape} ([h, w] or [h, w, C] with 1 <= C <= 4)")
    return np.ascontiguousarray(img.reshape(img.shape[0], img.shape[1], -1)), 8 * img.dtype.itemsize


def mask_intensity(rles, image, hist_shift=None, ctx=None):
    """The grey levels of `image` under RLE dicts of its size, one C call (amp_mask_intensity): (vals, hist).  vals uint64 [n, C, 8] = per mask
    and channel the exact integers {N, sum v, sum v^2, sum r v, sum c v, min, max, 0} over the mask's pixels (r, c) (row and column in the full
    image), zeros for an empty mask; hist uint32 [n, C, nbins], the pixels with v >> hist_shift == b, nbins = 2^(depth - hist_shift) <= 4096,
    or None without hist_shift.  image: uint8, uint16 or bool (read as uint8), [h, w] or [h, w, C] with C <= 4.  ValueError for a float or
    signed image (naming the dtype), a bad hist_shift and an image whose size differs from the masks'.  ctx: a _lib.Context (computed on its
    device) or None (on the host): the same bytes."""
    img, depth = intensity_image("mask_intensity", image)
    h, w, ch = img.shape
    if hist_shift is not None and (isinstance(hist_shift, bool) or not isinstance(hist_shift, (int, np.integer)) or
                                   not max(depth - 12, 0) <= int(hist_shift) <= depth):
        raise ValueError(f"mask_intensity: hist_shift = {hist_shift!r} (None, or an integer {max(depth - 12, 0)} .. {depth} at depth {depth}: "
                         f"at most {INTENSITY_MAX_BINS} bins)")
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if sizes - {(h, w)}:
        raise ValueError(f"mask_intensity: masks of sizes {sorted(sizes)} on an image of size {(h, w)}")
    n = len(rles)
    shift = -1 if hist_shift is None else int(hist_shift)
    nbins = 0 if shift < 0 else 1 << (depth - shift)
    vals = np.zeros((n, ch, INTENSITY_NVALS), dtype=np.uint64)
    hist = None if shift < 0 else np.zeros((n, ch, nbins), dtype=np.uint32)
    if n == 0:
        return vals, hist
    pool, off, ln = _pool([_counts(x) for x in rles])
    need = np.zeros(1, dtype=np.uint64)
    check(lib().amp_mask_intensity(_handle(ctx), _vp(pool), _vp(off), _vp(ln), n, h, w, _vp(img), ch, depth, shift, _vp(vals),
                                   None if hist is None else _vp(hist), 0 if hist is None else hist.size, _vp(need)), "amp_mask_intensity")
    return vals, hist


def merge(rles, intersect=False):
    assert len(rles) >= 1
    h, w = rles[0]["size"]
    cur = _counts(rles[0])
    for r in rles[1:]:
        b = _counts(r)
        cap = len(cur) + len(b) + 2
        out = np.empty(cap, dtype=np.uint32)
        m = C.c_int()
        check(lib().amp_rle_merge2(cur.ctypes.data_as(C.c_void_p), len(cur), b.ctypes.data_as(C.c_void_p), len(b),
                                   int(bool(intersect)), out.ctypes.data_as(C.c_void_p), cap, C.byref(m)), "amp_rle_merge2")
        cur = out[: m.value].copy()
    return {"size": [h, w], "counts": counts_to_string(cur)}


def frPyObjects(polys, h, w):
    """Polygons -> RLE, like pycocotools.mask.frPyObjects for polygon input: `polys` is a list of flat [x0,y0,x1,y1,...]
    polygons (or one such flat list); returns a list of RLE dicts (or one dict)."""
    single = len(polys) > 0 and np.isscalar(polys[0])
    plist = [polys] if single else polys
    out = []
    for p in plist:
        xy = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
        k = len(xy) // 2
        cap = 2 * 5 * (4 * (h + w) + 8 * k) + 16
        buf = np.empty(cap, dtype=np.uint32)
        m = C.c_int()
        check(lib().amp_rle_from_polygon(xy.ctypes.data_as(C.c_void_p), k, int(h), int(w), buf.ctypes.data_as(C.c_void_p), cap, C.byref(m)),
              "amp_rle_from_polygon")
        out.append({"size": [int(h), int(w)], "counts": counts_to_string(buf[: m.value])})
    return out[0] if single else out
