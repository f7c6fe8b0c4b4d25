"""The middle of the inference path -- csrc/rpn_select.hip (top-k, decode, sort), csrc/nms.hip (amp_nms, amp_rpn_nms_levels) and the
forward half of csrc/roi_align.hip -- through the C entry points against the NumPy references of tests/proposal_ref.py, which
tests/test_proposal_ref.py proves against the oracle on the CPU.

RoIAlign: every kernel (proposal_ref.ROI_KERNELS) and launch path -- fp32 and split-row maps, split-row output, index and XCD-major
order, a device-side RoI count, the grid-stride second trip under each of the three grid caps -- bit for bit on proposal_ref.ROI_EDGE
(samples exactly on -1, 0, H - 1, H and one fp32 step outside) plus seeded boxes.  The level is held to level_ref wherever a 1-ulp
change of log2f cannot change it, and to one of the two candidates elsewhere.  NMS: both entry points on proposal_ref.NMS_EDGE (IoU on
and one step above the threshold, duplicates, 0/0), at chunk-boundary sizes, with every word of the scan's removed mask and every
super-block of the per-level scan in use.  Top-k, decode, sort: ties decided by index, signed zeros, infinities, chunk boundaries, the
scale clamp, boxes clipped to nothing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import proposal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
FMT_X, FMT_Y = 1, 2


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _switches(lanes=1, tab=1, xcd=1, share=1):
    from ampis_amd._lib import lib
    lib().amp_debug_set_roi_lanes(lanes)
    lib().amp_debug_set_roi_tab(tab)
    lib().amp_debug_set_roi_xcd(xcd)
    lib().amp_debug_set_roi_share(share)


def _roi_align(ctx, feats, rois, bidx, P, fmt=0, count=None, out=None, lvl=None, Rn=None):
    """amp_roi_align_fmt on device tensors; count: device int32 [1] or None; out / lvl: tensors to write into (sentinels kept);
    Rn: the R passed (default: all of rois)."""
    from ampis_amd import ops, _lib
    f = ops.make_fpn_feats(feats)
    Rn = rois.shape[0] if Rn is None else Rn
    if out is None:
        out = torch.empty((Rn, P, P, f.C), device=DEV)
    if lvl is None:
        lvl = torch.empty((Rn,), dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().amp_roi_align_fmt(ctx.handle, C.byref(f), _lib.ptr(rois), _lib.ptr(bidx), _lib.ptr(count) if count is not None else None,
                                            Rn, P, _lib.ptr(out), _lib.ptr(lvl), int(fmt)), "amp_roi_align_fmt")
    return out, lvl


# ------------------------------------------------------------------------------------------------------------------ RoIAlign inputs
@functools.lru_cache(maxsize=None)
def _maps():
    """p2..p5 of 40 x 48 ... 5 x 6 cells, B = 2, C = 512, every value a split-row number (hi + lo' / 2048): the fp32 kernels read them
    as they are and the split kernels read the same values from split rows.  A channel slice [..., :C] (C % 32 == 0) keeps that."""
    return tuple(R.unsplit_rows_ref(R.split_rows_ref(m)) for m in R.seeded_maps(512, 31))


@functools.lru_cache(maxsize=None)
def _dev_maps(C, split):
    return tuple(_dev(R.split_rows_ref(m[..., :C]) if split else m[..., :C]) for m in _maps())


@functools.lru_cache(maxsize=None)
def _main_rois():
    rnd, rb = R.seeded_rois(200, 17)
    rois = np.concatenate([R.ROI_EDGE, rnd])
    bidx = np.concatenate([R.ROI_EDGE_BATCH, rb])
    levels, decided = R.level_ref(rois)
    assert decided.all()                     # the main cases do not hang on log2f (LEVEL_SWEEP does: test_levels_...)
    return rois, bidx, levels


@functools.lru_cache(maxsize=None)
def _main_ref(P):
    """roi_align_ref of the main cases at C = 512, on the device ([R, P, P, 512] float32), and its split-row form per C."""
    rois, bidx, levels = _main_rois()
    return R.roi_align_ref(_maps(), rois, bidx, P, levels)


@functools.lru_cache(maxsize=None)
def _main_ref_dev(P, C, split_out):
    ref = np.ascontiguousarray(_main_ref(P)[..., :C])
    return _dev(R.split_rows_ref(ref) if split_out else ref)


def _assert_rows_equal(got, ref_dev, what):
    """Bit for bit, compared on the device; on a mismatch name the first RoIs that differ."""
    g, r = got.view(torch.int32), ref_dev.view(torch.int32)
    if not torch.equal(g, r):
        rows = torch.nonzero((g != r).reshape(g.shape[0], -1).any(1)).flatten()[:8].tolist()
        raise AssertionError("%s: %d RoIs differ from the reference, first %s" % (what, len(rows), rows))


# (C, split input, roi_lanes, roi_tab, roi_xcd)
ROI_VARIANTS = [(C_, False, lanes, 1, 1) for C_ in (4, 64, 256, 512) for lanes in (0, 1)] + [(256, False, 3, 1, 1)] + \
               [(256, True, 1, tab, xcd) for tab in (0, 1) for xcd in (0, 2)] + [(256, True, 3, 1, 1), (32, True, 1, 1, 1)]


def _variant_id(v):
    return "C%d-%s-lanes%d-tab%d-xcd%d" % (v[0], "split" if v[1] else "f32", v[2], v[3], v[4])


def test_the_variants_reach_every_roi_align_kernel():
    reached = {R.roi_kernel_path(C_, split, lanes, tab) for C_, split, lanes, tab, xcd in ROI_VARIANTS}
    assert reached == set(R.ROI_KERNELS) and len(R.ROI_KERNELS) == 7
    assert any(R.roi_kernel_path(*v[:4]) == "roi_align_split_kernel" and v[3] == 0 for v in ROI_VARIANTS)        # AMP_ROI_TAB=0


@pytest.mark.parametrize("variant", ROI_VARIANTS, ids=_variant_id)
def test_roi_align_equals_the_reference_on_every_path(gpu_ctx, variant):
    C_, split, lanes, tab, xcd = variant
    rois, bidx, levels = _main_rois()
    d_rois, d_b = _dev(rois), _dev(bidx)
    feats = _dev_maps(C_, split)
    assert xcd != 2 or len(rois) >= 64                                           # XCD-major order is taken from 64 RoIs on
    # roi_align_split_kernel runs with its taps shared along a sample row (the default) and without (AMP_ROI_SHARE=0)
    shares = (1, 0) if R.roi_kernel_path(C_, split, lanes, tab) == "roi_align_split_kernel" else (1,)
    try:
        for share in shares:
            _switches(lanes, tab, xcd, share)
            for P in (7, 14):
                for split_out in ((False, True) if C_ % 32 == 0 else (False,)):
                    out, lvl = _roi_align(gpu_ctx, feats, d_rois, d_b, P, fmt=(FMT_X if split else 0) | (FMT_Y if split_out else 0))
                    torch.cuda.synchronize()
                    assert np.array_equal(lvl.cpu().numpy(), levels), (P, np.nonzero(lvl.cpu().numpy() != levels)[0])
                    _assert_rows_equal(out, _main_ref_dev(P, C_, split_out),
                                       "%s share=%d P=%d split_out=%d" % (_variant_id(variant), share, P, split_out))
    finally:
        _switches()


LEVEL_VARIANTS = [(256, False, 0, 1, 1), (256, False, 1, 1, 1), (256, False, 3, 1, 1), (256, True, 1, 0, 0), (256, True, 1, 1, 0),
                  (256, True, 1, 0, 2), (256, True, 1, 1, 2), (256, True, 3, 1, 1), (32, True, 1, 1, 1)]


def test_levels_at_the_boundaries(gpu_ctx):
    """LEVEL_SWEEP: RoIs within 8 ulps of the sides at which the level changes.  Where level_ref is decided the device reports that
    level; elsewhere one of the two candidates, with the pooled rows of that level; every variant reports the same."""
    from oracle import maskrcnn as O
    rois = R.LEVEL_SWEEP
    bidx = (np.arange(len(rois)) % 2).astype(np.int32)
    ref_lv, decided = R.level_ref(rois)
    cands = R.level_candidates(rois)
    d_rois, d_b = _dev(rois), _dev(bidx)
    P = 7
    reports = []
    try:
        for C_, split, lanes, tab, xcd in LEVEL_VARIANTS:
            _switches(lanes, tab, xcd)
            out, lvl = _roi_align(gpu_ctx, _dev_maps(C_, split), d_rois, d_b, P, fmt=FMT_X if split else 0)
            torch.cuda.synchronize()
            lv = lvl.cpu().numpy()
            reports.append(lv)
            assert np.array_equal(lv[decided], ref_lv[decided]), np.nonzero((lv != ref_lv) & decided)[0]
            und = np.nonzero(~decided)[0]
            for i in und:
                assert int(lv[i]) in cands[i], (i, lv[i], cands[i])
            # the undecided RoIs and the three degenerate ones: pooled at the level the device reports
            sel = np.concatenate([und, np.arange(len(rois) - 3, len(rois))])
            ref = R.roi_align_ref([m[..., :C_] for m in _maps()], rois[sel], bidx[sel], P, lv[sel])
            assert np.array_equal(_bits(out[_dev(sel)]), _bits(ref)), _variant_id((C_, split, lanes, tab, xcd))
            assert not ref[-3:].any()
    finally:
        _switches()
    for lv in reports[1:]:
        assert np.array_equal(lv, reports[0])
    torch_lv = O.assign_levels(torch.from_numpy(rois)).numpy()
    n_und = int((~decided).sum())
    n_diff = int(((reports[0] != torch_lv) & ~decided).sum())
    print("LEVEL_SWEEP: %d of %d RoIs undecided; the device differs from torch CPU on %d of them (and from level_ref's own log2 on %d)"
          % (n_und, len(rois), n_diff, int(((reports[0] != ref_lv) & ~decided).sum())))
    assert not ((reports[0] != torch_lv) & decided).any()


COUNT_VARIANTS = [(64, False, 1, 1, 1), (256, False, 3, 1, 1), (256, True, 1, 1, 0), (256, True, 1, 0, 0), (256, True, 1, 1, 2), (256, True, 1, 0, 2)]


@pytest.mark.parametrize("variant", COUNT_VARIANTS, ids=_variant_id)
def test_roi_count_on_the_device_limits_the_rows_written(gpu_ctx, variant):
    """roi_count < R: rows and levels at and beyond the count keep what was there; roi_count > R: all R rows; R = 0: nothing."""
    C_, split, lanes, tab, xcd = variant
    rois, bidx, levels = _main_rois()
    n_edge = len(R.ROI_EDGE)
    rois, bidx, levels = rois[n_edge - 20:], bidx[n_edge - 20:], levels[n_edge - 20:]         # 20 edge cases + the 200 seeded boxes
    Rn, P, count = len(rois), 7, 97
    assert count < Rn and Rn >= 64
    ref = _main_ref_dev(P, C_, False)[n_edge - 20:]
    d_rois, d_b = _dev(rois), _dev(bidx)
    feats = _dev_maps(C_, split)
    SENT, LSENT = 0x7fc12345, -7
    try:
        _switches(lanes, tab, xcd)
        for cnt in (count, Rn + 1000):
            out = torch.full((Rn, P, P, C_), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
            lvl = torch.full((Rn,), LSENT, dtype=torch.int32, device=DEV)
            _roi_align(gpu_ctx, feats, d_rois, d_b, P, fmt=FMT_X if split else 0, count=torch.tensor([cnt], dtype=torch.int32, device=DEV),
                       out=out, lvl=lvl)
            torch.cuda.synchronize()
            n = min(cnt, Rn)
            _assert_rows_equal(out[:n], ref[:n], "count %d" % cnt)
            assert np.array_equal(lvl[:n].cpu().numpy(), levels[:n])
            assert bool((out[n:].view(torch.int32) == SENT).all()) and bool((lvl[n:] == LSENT).all())
        out = torch.full((1, P, P, C_), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
        lvl = torch.full((1,), LSENT, dtype=torch.int32, device=DEV)
        _roi_align(gpu_ctx, feats, d_rois, d_b, P, fmt=FMT_X if split else 0, out=out, lvl=lvl, Rn=0)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == SENT).all()) and int(lvl[0]) == LSENT
    finally:
        _switches()


@functools.lru_cache(maxsize=None)
def _trip_case():
    """2700 one-sample RoIs at P = 14 and their reference at C = 256 on the device (the fp32 case uses its first 1400, 4 channels)."""
    rois, bidx = R.one_sample_rois(2700, 41)
    levels, decided = R.level_ref(rois)
    assert decided.all() and not levels.any()
    for r in rois[::97]:
        ys, xs = R.roi_samples(r, 14, 4, *R.MAP_HW[0])
        assert ys.shape[1] == 1 and xs.shape[1] == 1
    ref = R.roi_align_ref([m[..., :256] for m in _maps()], rois, bidx, 14, levels)
    return rois, bidx, _dev(ref)


@pytest.mark.parametrize("C_,split,xcd,Rn", [(4, False, 1, 1400), (256, True, 0, 2700), (256, True, 2, 2700)], ids=["f32-C4", "split-index-order", "split-xcd-major"])
def test_roi_align_grid_stride_second_trip(gpu_ctx, C_, split, xcd, Rn):
    """More work than the capped grid holds in one trip (g > 65536, g2 > 65536, per_x > 8192): every RoI against the reference."""
    P = 14
    units, per_trip = R.roi_grid_trips(Rn, P, C_, split, xcd == 2)
    assert units > per_trip, (units, per_trip)                                    # the cap is exceeded: some workgroups loop again
    nbins = Rn * P * P
    if not split:
        assert (nbins + 3) // 4 > 65536
    elif xcd == 0:
        assert (nbins + 7) // 8 > 65536
    else:
        assert ((Rn // 8 + 33) * P * P + 7) // 8 > 8192 and 64 <= Rn <= 8192
    rois, bidx, ref = _trip_case()
    d_rois, d_b = _dev(rois[:Rn]), _dev(bidx[:Rn])
    try:
        _switches(1, 1, xcd)
        out, lvl = _roi_align(gpu_ctx, _dev_maps(C_, split), d_rois, d_b, P, fmt=FMT_X if split else 0)
        torch.cuda.synchronize()
    finally:
        _switches()
    assert not bool(lvl.any())
    _assert_rows_equal(out, ref[:Rn, :, :, :C_].contiguous(), "R=%d" % Rn)


# ------------------------------------------------------------------------------------------------------------------ NMS
def _nms(ctx, boxes, cats, counts, thresh, max_keep):
    """amp_nms on host arrays boxes [B, cap, 4], cats [B, cap], counts [B] -> list of kept positions per image."""
    from ampis_amd import ops
    keep, kc = ops.nms(ctx, _dev(boxes.astype(F32)), _dev(cats.astype(np.int32)), _dev(np.asarray(counts, np.int32)), thresh, max_keep)
    torch.cuda.synchronize()
    keep, kc = keep.cpu().numpy(), kc.cpu().numpy()
    return [keep[b, :kc[b]] for b in range(len(counts))]


@pytest.mark.parametrize("thresh", [0.5, 0.7])
def test_nms_edge_cases(gpu_ctx, thresh):
    """Every NMS_EDGE case as an image of its own, and all of them in one list."""
    cap = 64
    Bn = len(R.NMS_EDGE)
    boxes, cats = np.zeros((Bn, cap, 4), F32), np.full((Bn, cap), -1, np.int32)
    counts = []
    for i, (name, b, c, th, exp, pair) in enumerate(R.NMS_EDGE):
        boxes[i, :len(b)], cats[i, :len(b)] = b, c
        counts.append(len(b))
    got = _nms(gpu_ctx, boxes, cats, counts, thresh, 1000)
    for i, (name, b, c, th, exp, pair) in enumerate(R.NMS_EDGE):
        ref = R.nms_ref(b, c, thresh, 1000)
        assert np.array_equal(got[i], ref), (name, got[i], ref)
        if exp is not None and th == thresh:
            assert got[i].tolist() == exp, name
    lb, lc, _ = R.nms_edge_list()
    got = _nms(gpu_ctx, lb[None], lc[None], [len(lb)], thresh, 1000)[0]
    assert np.array_equal(got, R.nms_ref(lb, lc, thresh, 1000))


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_nms_at_chunk_boundaries(gpu_ctx, n):
    rng = np.random.default_rng(n)
    boxes = np.round(R.clustered_boxes(n, n, spread=10.0, size=30.0, centres=5))         # integer boxes: exact ties and duplicates happen
    cats = rng.integers(0, 2, n)
    for thresh in (0.5, 0.7):
        got = _nms(gpu_ctx, boxes[None], cats[None], [n], thresh, 1000)[0]
        ref = R.nms_ref(boxes, cats, thresh, 1000)
        assert np.array_equal(got, ref), (thresh, got, ref)
        assert 2 < len(ref) < n


def test_nms_uses_every_word_of_the_removed_mask(gpu_ctx):
    """n = 16384, one category, clustered: suppression reaches from the first chunk into chunks 192..255, whose removed bits are the
    fourth register of nms_scan_kernel, and the scan runs to the end (fewer than max_keep survive)."""
    n, max_keep, thresh = 16384, 1000, 0.5
    boxes = R.clustered_boxes(n, 77)
    boxes[16000] = [5000, 5000, 5040, 5040]                       # a late box nothing suppresses
    boxes[16383] = boxes[3]                                        # the last box: a duplicate of an early one
    ref = R.nms_ref(boxes, np.zeros(n, np.int64), thresh, max_keep)
    assert len(ref) < max_keep and ref[-1] >= 12288 and 16000 in ref and 16383 not in ref
    first = ref[ref < 64]
    late = boxes[12288:]
    assert any((R.iou_ref(boxes[i], late) > F32(thresh)).any() for i in first)        # chunk 0 removes boxes of chunks >= 192
    got = _nms(gpu_ctx, boxes[None], np.zeros((1, n), np.int32), [n], thresh, max_keep)[0]
    assert np.array_equal(got, ref)


def test_nms_stops_at_max_keep(gpu_ctx):
    """max_keep reached exactly at the end of a chunk, and one box later."""
    disjoint = R.NMS_EDGE[R.NMS_EDGE_IDS.index("chunk-all-disjoint")][1]
    boxes = np.concatenate([disjoint, R.clustered_boxes(300, 5) + F32(400)])
    n = len(boxes)
    cats = np.zeros(n, np.int64)
    full = R.nms_ref(boxes, cats, 0.5, 1000)
    assert full[:64].tolist() == list(range(64)) and len(full) > 66
    for max_keep in (64, 65):
        ref = R.nms_ref(boxes, cats, 0.5, max_keep)
        assert len(ref) == max_keep and np.array_equal(ref, full[:max_keep])
        got = _nms(gpu_ctx, boxes[None], cats[None], [n], 0.5, max_keep)[0]
        assert np.array_equal(got, ref), max_keep
    assert full[64] >= 64 and (full[63] == 63)                    # 64 kept when chunk 0 ends; the 65th is a box of a later chunk


def _levels_case(segments, k, cap):
    """segments: per level (boxes [n, 4], scores [n] descending, valid [n]) -> boxes [cap, 4], keys [cap] int64, sel_count [L]."""
    boxes, keys = np.zeros((cap, 4), F32), np.zeros(cap, np.int64)
    off = 0
    for l, (b, s, v) in enumerate(segments):
        n = len(b)
        assert n <= k and (np.diff(s) <= 0).all()
        boxes[off:off + n] = b
        kk = R.sortkey_ref(s, np.arange(off, off + n), np.full(n, l))
        keys[off:off + n] = np.where(v, kk, 0)
        off += n
    return boxes, keys, np.asarray([len(s[0]) for s in segments], np.int32)


def _check_levels(ctx, boxes, keys, sel, k, thresh, max_keep):
    """amp_rpn_nms_levels against rpn_nms_levels_ref and against the one-list chain (amp_sort_gather + amp_nms with the level as category)."""
    from ampis_amd import ops
    d_b, d_k, d_s = _dev(boxes[None]), _dev(keys[None]), _dev(sel[None])
    pb, ps, pl, pc, _ = ops.rpn_nms_levels(ctx, d_b, d_k, d_s, k, thresh, max_keep)
    sb, ss, scat, cnt, pos = ops.sort_gather(ctx, d_k, d_b)
    keep, kc = ops.nms(ctx, sb, scat, cnt, thresh, max_keep)
    torch.cuda.synchronize()
    slots = R.rpn_nms_levels_ref(boxes, keys, sel, k, thresh, max_keep)
    n = int(pc[0])
    assert n == len(slots), (n, len(slots))
    ku = keys.view(np.uint64)[slots]
    assert np.array_equal(_bits(pb[0, :n]), _bits(boxes[slots]))
    assert np.array_equal(_bits(ps[0, :n]).astype(np.uint64), np.where(ku >> np.uint64(63), (ku >> np.uint64(32)) & np.uint64(0x7fffffff),
                                                                     ~(ku >> np.uint64(32)) & np.uint64(0xffffffff)))        # ord2f of the word
    assert np.array_equal(pl[0, :n].cpu().numpy(), (ku & np.uint64(0xff)).astype(np.int32))
    assert not bool(pb[0, n:].any()) and not bool(ps[0, n:].any()) and bool((pl[0, n:] == -1).all())
    assert int(kc[0]) == n
    assert np.array_equal(pos[0][keep[0, :n].long()].cpu().numpy(), slots)            # the one-list chain keeps the same slots in the same order
    return slots


@pytest.mark.parametrize("thresh", [0.5, 0.7])
def test_rpn_nms_levels_edge_cases(gpu_ctx, thresh):
    """The NMS_EDGE boxes as level segments: the whole list, the list reversed with some invalid candidates and the same scores (ties
    between levels go by position), and a segment of exactly 64 candidates."""
    lb, _, _ = R.nms_edge_list()
    n = len(lb)
    scores = np.linspace(4, -4, n).astype(F32)
    valid1 = np.ones(n, bool)
    valid1[[0, 5, 70, n - 1]] = False
    one = R.NMS_EDGE[R.NMS_EDGE_IDS.index("chunk-one-overlap")][1]
    segs = [(lb, scores, np.ones(n, bool)), (lb[::-1], scores, valid1), (one, scores[:64], np.ones(64, bool))]
    k = n
    boxes, keys, sel = _levels_case(segs, k, 3 * k)
    assert sel[2] == 64
    for max_keep in (1000, 37):
        slots = _check_levels(gpu_ctx, boxes, keys, sel, k, thresh, max_keep)
        assert len(slots) == min(max_keep, len(_check_levels(gpu_ctx, boxes, keys, sel, k, thresh, 100000)))


@pytest.mark.parametrize("k,sel", [(4096, (4096, 4096)), (2049, (2049, 1000))], ids=["k4096-four-super-blocks", "k2049-three-super-blocks"])
def test_rpn_nms_levels_walks_every_super_block(gpu_ctx, k, sel):
    """lvl_scan_kernel folds the decisions of earlier super-blocks (1024 boxes) into later ones: clustered segments in which a box kept in
    the first super-block suppresses boxes of the last, and the last super-block keeps a box of its own."""
    thresh, max_keep = 0.7, 100000
    segs = []
    for l, n in enumerate(sel):
        b = R.clustered_boxes(n, 100 + l, spread=5.0)
        b[n - 1] = [7000 + 100 * l, 7000, 7040 + 100 * l, 7040]                  # the last candidate: kept, nothing near it
        segs.append((b, np.sort(np.random.default_rng(l).normal(0, 1, n).astype(F32))[::-1].copy(), np.ones(n, bool)))
    boxes, keys, sel_a = _levels_case(segs, k, len(sel) * k)
    slots = _check_levels(gpu_ctx, boxes, keys, sel_a, k, thresh, max_keep)
    nsb = (k + 1023) // 1024
    assert nsb == (4 if k == 4096 else 3)
    last0 = (nsb - 1) * 1024
    assert (k - 1) in slots and (k - 1) >= last0                                  # level 0's last super-block keeps its last box
    b0 = segs[0][0]
    kept0 = np.sort(slots[slots < k])
    assert len(kept0) < k // 4
    if k == 4096:
        assert any((R.iou_ref(b0[i], b0[last0:]) > F32(thresh)).any() for i in kept0[kept0 < 1024])        # super-block 1 reaches into super-block 4
        assert any((R.iou_ref(b0[i], b0[2048:3072]) > F32(thresh)).any() for i in kept0[kept0 < 1024])
    else:
        assert any((R.iou_ref(b0[i], b0[1024:2048]) > F32(thresh)).any() for i in kept0[kept0 < 1024])


# ------------------------------------------------------------------------------------------------------------------ top-k, decode, sort
@functools.lru_cache(maxsize=None)
def _topk_case():
    """Five levels, B = 2: all logits equal; zeros of both signs only; infinities among ties; exactly TOPK_CHUNK = 49 152 anchors
    (128 x 128 x 3, the largest single chunk); 49 155 anchors (1 x 16385 x 3, two chunks).  Image 1: the two large levels all equal, so
    the k-th place is decided by index alone, across the chunk boundary too."""
    rng = np.random.default_rng(3)
    shapes = [(8, 8), (4, 4), (4, 4), (128, 128), (1, 16385)]
    preds = []
    for l, (h, w) in enumerate(shapes):
        p = np.zeros((2, h * w, 16), F32)
        p[:, :, 3:15] = rng.normal(0, 0.1, (2, h * w, 12))
        lg = np.round(rng.normal(0, 1, (2, h * w, 3)) * 4) / 4                  # ties everywhere
        if l == 0:
            lg[:] = 0.25
        elif l == 1:
            lg = np.where(rng.integers(0, 2, lg.shape) == 1, -0.0, 0.0)
        elif l == 2:
            lg[0].reshape(-1)[[3, 17, 40]] = np.inf
            lg[0].reshape(-1)[[5, 6, 30]] = -np.inf
            lg[1].reshape(-1)[:] = -np.inf
            lg[1].reshape(-1)[[7, 8]] = np.inf
        else:
            lg[1] = -1.5
        p[:, :, :3] = lg
        preds.append(p)
    return shapes, preds


@pytest.mark.parametrize("k", [1, 100, 2048])
def test_topk_edges(gpu_ctx, k):
    from ampis_amd import ops
    shapes, preds = _topk_case()
    assert shapes[3][0] * shapes[3][1] * 3 == 49152 and shapes[4][0] * shapes[4][1] * 3 == 49155
    si, sl, sc = ops.rpn_topk(gpu_ctx, [_dev(p) for p in preds], shapes, 2, k)
    torch.cuda.synchronize()
    si, sl, sc = si.cpu().numpy(), sl.cpu().numpy(), sc.cpu().numpy()
    for b in range(2):
        for l, p in enumerate(preds):
            idx, lg = R.topk_ref(p[b, :, :3].reshape(-1), k)
            assert sc[b, l] == len(idx) == min(k, p.shape[1] * 3), (b, l)
            assert np.array_equal(si[b, l, :len(idx)], idx), (b, l)
            assert np.array_equal(_bits(sl[b, l, :len(idx)]), _bits(lg)), (b, l)
    assert k <= 48 or sc[0, 1] == 48                                             # k greater than the level's anchors


def _decode(ctx, preds, shapes, k, img_hw, per_image):
    """amp_rpn_topk + amp_rpn_decode(_sized) -> (sel_idx, sel_logit, sel_count, boxes [B, cap, 4], keys [B, cap]) on the host."""
    from ampis_amd import ops, _lib
    dp = [_dev(p) for p in preds]
    B, L = preds[0].shape[0], len(preds)
    si, sl, sc = ops.rpn_topk(ctx, dp, shapes, B, k)
    lv = ops.make_rpn_levels(dp, shapes)
    cap = L * k
    boxes = torch.empty((B, cap, 4), device=DEV)
    keys = torch.empty((B, cap), dtype=torch.int64, device=DEV)
    hw = torch.tensor(np.asarray(img_hw).tolist(), dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().amp_rpn_decode_sized(ctx.handle, C.byref(lv), B, k, _lib.ptr(si), _lib.ptr(sl), _lib.ptr(sc), int(img_hw[0][0]),
                                               int(img_hw[0][1]), _lib.ptr(hw) if per_image else None, cap, _lib.ptr(boxes), _lib.ptr(keys), None),
               "amp_rpn_decode_sized")
    sb, ss, scat, cnt, pos = ops.sort_gather(ctx, keys, boxes)
    torch.cuda.synchronize()
    return (si.cpu().numpy(), sl.cpu().numpy(), sc.cpu().numpy(), boxes.cpu().numpy(), keys.cpu().numpy(),
            ss.cpu().numpy(), scat.cpu().numpy(), cnt.cpu().numpy(), pos.cpu().numpy())


@pytest.mark.parametrize("per_image", [True, False], ids=["img_hw-per-image", "one-size"])
def test_decode_edges(gpu_ctx, per_image):
    """decode_cases(): deltas on, one step above and 10x above the scale clamp, overflowing and NaN deltas, infinite logits, boxes clipped
    to zero width and to one step of width, two images of different sizes.  Validity and order exact; boxes within 4 ulps of the largest
    coordinate involved, 1e-4 px at most."""
    preds, shapes, k = R.decode_case_preds(), R.DECODE_SHAPES, R.DECODE_K
    img_hw = R.DECODE_IMG_HW if per_image else (R.DECODE_IMG_HW[0],) * 2
    si, sl, sc, boxes, keys, ss, scat, cnt, pos = _decode(gpu_ctx, preds, shapes, k, img_hw, per_image)
    ref = R.decode_pipeline_ref(preds, shapes, k, img_hw, R.DECODE_SIZES, R.DECODE_STRIDES)
    slots = R.decode_case_slots()
    for b in range(2):
        off = 0
        order_ref = []
        for l, lv in enumerate(ref[b]):
            n = len(lv["idx"])
            assert sc[b, l] == n and np.array_equal(si[b, l, :n], lv["idx"]) and np.array_equal(_bits(sl[b, l, :n]), _bits(lv["logit"]))
            kk = keys[b, off:off + n]
            assert np.array_equal(kk != 0, lv["valid"]), (b, l, np.nonzero((kk != 0) != lv["valid"])[0], lv["idx"])
            want = R.sortkey_ref(lv["logit"], np.arange(off, off + n), np.full(n, l))
            assert np.array_equal(kk[lv["valid"]], want[lv["valid"]])
            fin = np.isfinite(lv["boxes"]).all(1) & (lv["extent"] < 3e38)           # (beyond fp32 the box is invalid: checked above)
            tol = np.minimum(1e-4, 4 * np.spacing(lv["extent"][fin].astype(F32)).astype(np.float64))
            err = np.abs(boxes[b, off:off + n][fin].astype(np.float64) - lv["boxes"][fin]).max(1)
            assert (err <= tol).all(), (b, l, err.max(), lv["idx"][fin][np.argmax(err - tol)])
            order_ref += [(-float(s) if s == s else 0.0, off + j) for j, s in enumerate(lv["logit"]) if lv["valid"][j]]
            off += n
        assert not keys[b, off:].any() and not boxes[b, off:].any()
        order_ref.sort()
        assert cnt[b] == len(order_ref) and pos[b, :cnt[b]].tolist() == [p for _, p in order_ref]
    # the cases the names promise, on the device
    def key_of(b, name):
        l, idx = slots[name]
        j = int(np.nonzero(ref[b][l]["idx"] == idx)[0][0])
        o = j + (0 if l == 0 else len(ref[b][0]["idx"]))
        return keys[b, o], boxes[b, o]
    assert key_of(0, "zero-width-at-left-border")[0] == 0 and key_of(0, "one-step-of-width")[0] != 0
    assert key_of(0, "one-step-of-width")[1][2] == F32(2.0 ** -20) and key_of(0, "one-step-of-width")[1][0] == 0
    assert key_of(0, "zero-width-at-image-1-border")[0] != 0
    assert (key_of(1, "zero-width-at-image-1-border")[0] == 0) == per_image
    for name in ("dx-overflows", "dy-nan", "dw-nan", "logit-plus-inf", "logit-minus-inf"):
        assert key_of(0, name)[0] == 0, name
    for name in ("dw-on-clamp", "dw-step-above-clamp", "dw-10x-clamp", "dw-inf"):
        assert key_of(0, name)[0] != 0, name
