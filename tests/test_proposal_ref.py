"""tests/proposal_ref.py against the oracle (CPU): the NumPy references of RoIAlign, NMS, top-k, decode and the level rule, written from
the definitions, must agree with oracle/maskrcnn.py's restatements on every case table and on seeded random inputs -- bit for bit
where the arithmetic is exactly reproducible -- and the tables must hold the cases their names promise, so that no GPU test can pass by
leaving one out."""
import numpy as np
import pytest
import torch

import proposal_ref as R
from oracle import maskrcnn as O

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ references
def _oracle_roi_align(maps, rois, bidx, P, levels):
    out = np.zeros((len(rois), P, P, maps[0].shape[-1]), F32)
    for l in range(4):
        for b in range(maps[0].shape[0]):
            sel = np.nonzero((levels == l) & (bidx == b))[0]
            if len(sel):
                f = torch.from_numpy(maps[l][b]).permute(2, 0, 1)
                out[sel] = O.roi_align(f, torch.from_numpy(rois[sel]), P, 1.0 / R.STRIDES[l]).permute(0, 2, 3, 1).numpy()
    return out


@pytest.mark.parametrize("P", [7, 14])
def test_roi_align_ref_equals_oracle_bit_for_bit(P):
    maps = R.seeded_maps(8, 3)
    rnd, rb = R.seeded_rois(200, 17)
    sweep = R.LEVEL_SWEEP[:-3]
    rois = np.concatenate([R.ROI_EDGE, R.LEVEL_SWEEP[-3:], sweep, rnd])
    bidx = np.concatenate([R.ROI_EDGE_BATCH, np.zeros(3 + len(sweep), np.int32), rb])
    levels, _ = R.level_ref(rois)
    ref = R.roi_align_ref(maps, rois, bidx, P, levels)
    orc = _oracle_roi_align(maps, rois, bidx, P, levels)
    assert np.array_equal(_bits(ref), _bits(orc)), np.nonzero((_bits(ref) != _bits(orc)).reshape(len(rois), -1).any(1))[0]
    assert np.abs(ref).max() > 0
    # the three degenerate boxes pool to zero
    n = len(R.ROI_EDGE)
    assert not ref[n:n + 3].any()
    # an undecided RoI pooled at either candidate level is still the oracle's value at that level
    _, dec = R.level_ref(R.LEVEL_SWEEP)
    und = R.LEVEL_SWEEP[~dec][:6]
    for lv_set, roi in zip(R.level_candidates(und), und):
        assert len(lv_set) == 2
        for lv in lv_set:
            a = R.roi_align_ref(maps, roi[None], [1], P, [lv])
            assert np.array_equal(_bits(a), _bits(_oracle_roi_align(maps, roi[None], np.array([1]), P, np.array([lv]))))


def test_split_rows_ref_round_trip_and_layout():
    rng = np.random.default_rng(2)
    x = (rng.normal(0, 1, (5, 3, 64)) * np.exp(rng.uniform(-8, 4, (5, 3, 64)))).astype(F32)
    x[0, 0, :4] = [0.0, -0.0, 1.0, -2.5]
    s = R.split_rows_ref(x)
    assert s.shape == x.shape and s.dtype == F32
    h = s.reshape(-1, 2, 32).view(np.float16).reshape(-1, 2, 2, 32)          # [rows, group, hi | lo, 32 channels]
    xr = x.reshape(-1, 2, 32)
    assert np.array_equal(h[:, :, 0], xr.astype(np.float16))
    assert np.array_equal(h[:, :, 1], ((xr - xr.astype(np.float16).astype(F32)) * F32(2048)).astype(np.float16))
    back = R.unsplit_rows_ref(s)
    assert np.abs(back - x).max() <= np.abs(x).max() * 2.0 ** -21              # hi + lo' / 2048 holds 22 bits
    assert np.array_equal(_bits(R.unsplit_rows_ref(R.split_rows_ref(back))), _bits(back))      # a decoded value splits exactly


def _nms_both(boxes, cats, thresh, max_keep):
    ref = R.nms_ref(boxes, cats, thresh, max_keep)
    orc = O.nms_sorted(torch.from_numpy(np.asarray(boxes, F32)), torch.from_numpy(np.asarray(cats).astype(np.int64)), thresh, max_keep=max_keep)
    assert np.array_equal(ref, orc.numpy()), (ref, orc)
    return ref


@pytest.mark.parametrize("i", range(len(R.NMS_EDGE)), ids=R.NMS_EDGE_IDS)
def test_nms_ref_equals_oracle_on_the_edge_cases(i):
    name, boxes, cats, thresh, expected, pair = R.NMS_EDGE[i]
    for th in (0.5, 0.7):
        kept = _nms_both(boxes, cats, th, 1000)
        if th == thresh and expected is not None:
            assert kept.tolist() == expected, (name, kept)
    if name == "chain":
        assert _nms_both(boxes, cats, 0.5, 1000).tolist() == [0, 2, 3]         # a suppresses b (0.6); b would suppress c (0.6) but is gone: c stays
    for mk in (1, 2):
        assert len(_nms_both(boxes, cats, thresh, mk)) == min(mk, len(_nms_both(boxes, cats, thresh, 1000)))


def test_nms_ref_equals_oracle_on_the_joined_list_and_random_boxes():
    boxes, cats, slices = R.nms_edge_list()
    for th in (0.5, 0.7):
        kept = _nms_both(boxes, cats, th, 10000)
        for (name, sl), case in zip(slices, R.NMS_EDGE):              # the cases do not meet: every case keeps what it keeps alone
            own = kept[(kept >= sl.start) & (kept < sl.stop)] - sl.start
            assert np.array_equal(own, R.nms_ref(case[1], case[2], th, 10000)), name
    rng = np.random.default_rng(8)
    for t in range(300):
        n = int(rng.integers(1, 90))
        c = rng.uniform(0, 60, (n, 2)); s = rng.integers(1, 30, (n, 2)) if t % 2 else rng.uniform(1, 30, (n, 2))
        b = np.concatenate([c - s / 2, c + s / 2], 1).astype(F32)
        if t % 3 == 0:
            b = np.round(b)                                                    # integer boxes: exact ties, duplicates, zero areas
        _nms_both(b, rng.integers(0, 3, n), float(rng.choice([0.3, 0.5, 0.7])), int(rng.choice([5, 1000])))
    cl = R.clustered_boxes(3000, 4)
    kept = _nms_both(cl, np.zeros(3000, np.int64), 0.5, 1000)
    assert 10 < len(kept) < 1000


def test_topk_ref_equals_oracle_order():
    rng = np.random.default_rng(6)
    for t in range(300):
        n = int(rng.integers(1, 400))
        s = rng.normal(0, 1, n).astype(F32)
        if t % 2:
            s = np.round(s * 2) / 2                                            # many ties
        if t % 3 == 0:
            s[rng.integers(0, n, 3)] = [0.0, -0.0, 0.0]
        if t % 5 == 0:
            s[rng.integers(0, n, 2)] = [np.inf, -np.inf]
        if t % 7 == 0:
            s[:] = s[0]                                                        # all equal: index order alone
        k = int(rng.integers(1, n + 20))
        idx, lg = R.topk_ref(s, k)
        order = O.sort_desc_stable(torch.from_numpy(s)).numpy()[:k]
        assert np.array_equal(idx, order)
        assert np.array_equal(lg, s[order]) and not np.signbit(lg[lg == 0]).any()
    idx, _ = R.topk_ref(np.asarray([-0.0, 0.0, -0.0, 1.0], F32), 3)
    assert idx.tolist() == [3, 0, 1]


def _oracle_proposals(preds, shapes, k, img_hw):
    """find_top_rpn_proposals without suppression (threshold 1: no IoU is above it) -> per image (boxes, logits) of the valid candidates."""
    cfg = O.Cfg(num_classes=2, pre_nms_topk=k, post_nms_topk=100000, rpn_nms_thresh=1.0)
    B = preds[0].shape[0]
    outs = [(torch.from_numpy(p[:, :, :3].reshape(B, -1)), torch.from_numpy(p[:, :, 3:15].reshape(B, -1, 4))) for p in preds]
    with np.errstate(all="ignore"):
        cands = O.rpn_select_candidates(outs, shapes, cfg)
        return [O.rpn_proposals_from_candidates(cands[b], img_hw[b], cfg) for b in range(B)]


def _ref_proposals(per_level):
    """The valid candidates of decode_pipeline_ref for one image in (logit descending, concatenated position ascending) order."""
    boxes = np.concatenate([lv["boxes"] for lv in per_level])
    logit = np.concatenate([lv["logit"] for lv in per_level])
    valid = np.concatenate([lv["valid"] for lv in per_level])
    order = np.argsort(-logit[valid], kind="stable")
    return boxes[valid][order], logit[valid][order]


def _check_decode_against_oracle(preds, shapes, k, img_hw):
    ref = R.decode_pipeline_ref(preds, shapes, k, img_hw, O.ANCHOR_SIZES, O.STRIDES)
    orc = _oracle_proposals(preds, shapes, k, img_hw)
    for b in range(preds[0].shape[0]):
        rb, rl = _ref_proposals(ref[b])
        ob, ol = orc[b]
        assert np.array_equal(rl, ol.numpy()), b                               # the same kept set in the same order
        assert len(rb) == 0 or np.abs(rb - ob.numpy()).max() < 1e-4
    return ref


def test_decode_ref_equals_oracle_on_the_cases():
    ref = _check_decode_against_oracle(R.decode_case_preds(), R.DECODE_SHAPES, R.DECODE_K, R.DECODE_IMG_HW)
    slots = R.decode_case_slots()
    want = {"plain": (True, True), "dw-on-clamp": (True, True), "dw-step-above-clamp": (True, True), "dw-10x-clamp": (True, True),
            "dx-overflows": (False, False), "dw-inf": (True, True), "dy-nan": (False, False), "dw-nan": (False, False), "logit-plus-inf": (False, False),
            "logit-minus-inf": (False, False), "zero-width-at-left-border": (False, False), "one-step-of-width": (True, True),
            "zero-width-at-image-1-border": (True, False), "level-1-plain": (True, True)}
    for name, (l, idx) in slots.items():
        for b in range(2):
            lv = ref[b][l]
            pos = np.nonzero(lv["idx"] == idx)[0]
            if name == "logit-minus-inf":
                assert pos.tolist() == [len(lv["idx"]) - 1] and len(lv["idx"]) == 48       # k exceeds the level: selected last, then dropped
            assert len(pos) == 1, (name, b)                                    # every named case is among the selected
            assert bool(lv["valid"][pos[0]]) == want[name][b], (name, b)
    lv = ref[0][0]
    assert lv["idx"][0] == slots["logit-plus-inf"][1] and np.isposinf(lv["logit"][0])      # +inf is selected first, then dropped


def test_decode_ref_equals_oracle_on_random_rpn_outputs():
    rng = np.random.default_rng(12)
    shapes = [(12, 16), (6, 8), (3, 4)]
    for t in range(6):
        preds = []
        for h, w in shapes:
            p = rng.normal(0, 2, (2, h * w, 16)).astype(F32)
            p[:, :, 3:15] *= 0.4
            p[:, :, 15] = 0
            p[0, rng.integers(0, h * w, 3), 3] = np.nan
            p[1, rng.integers(0, h * w, 3), 5] = 1e4
            preds.append(p)
        ref = _check_decode_against_oracle(preds, shapes, 60, ((48, 64), (40, 50)))
        # (boxes whose validity hangs on expf are rare: the kept sets above already agreed; report how close the closest one is)
        m = np.concatenate([np.abs(lv["margin"][np.isfinite(lv["margin"]) & (lv["margin"] != 0)]) for per in ref for lv in per])
        assert m.min() > 1e-4, m.min()


def test_level_ref_equals_oracle_where_decided():
    rnd, _ = R.seeded_rois(400, 23, max_side=1200.0)
    for rois in (R.LEVEL_SWEEP, R.ROI_EDGE, rnd):
        lv, dec = R.level_ref(rois)
        orc = O.assign_levels(torch.from_numpy(rois)).numpy()
        assert np.array_equal(lv[dec], orc[dec]), np.nonzero((lv != orc) & dec)[0]
        for i in np.nonzero(~dec)[0]:
            assert int(orc[i]) in R.level_candidates(rois[i:i + 1])[0]


def test_sortkey_ref_orders_like_the_scores():
    s = np.asarray([3.0, 0.0, -0.0, -1.5, np.inf, -np.inf, 1e-30, -1e-30], F32)
    k = R.sortkey_ref(s, np.arange(8), np.zeros(8, np.int64)).view(np.uint64)
    order = np.argsort(~k, kind="stable")
    assert order.tolist() == R.topk_ref(s, 8)[0].tolist()
    assert (k != 0).all() and ((k >> np.uint64(8)) & np.uint64(0xffffff)).tolist() == [0xffffff - i for i in range(8)]


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_level_sweep_is_mostly_decided_and_brackets_every_boundary():
    lv, dec = R.level_ref(R.LEVEL_SWEEP)
    n_und = int((~dec).sum())
    print("LEVEL_SWEEP: %d of %d RoIs undecided" % (n_und, len(dec)))
    assert len(dec) == 695 + 3
    assert n_und <= 0.10 * len(dec)
    assert n_und > 0                                                           # the sweep does reach RoIs a 1-ulp log2f decides
    for k, bound in enumerate(R.LEVEL_BOUNDS):
        near = np.asarray([name.startswith("side%d-" % bound) or name.startswith("side%d+" % bound) for name in R.LEVEL_SWEEP_IDS])
        near &= np.asarray(["-by-" not in name for name in R.LEVEL_SWEEP_IDS])
        assert near.sum() == 4 * 17 * 2
        got = set(lv[near & dec].tolist())
        assert got == {k, k + 1}, (bound, got)                                 # decided RoIs on both sides, within 8 ulps of the side
    names = dict(zip(R.LEVEL_SWEEP_IDS, range(len(lv))))
    for name in ("zero-area", "x2-below-x1", "both-sides-negative"):
        assert lv[names[name]] == 0 and dec[names[name]]
    r = R.LEVEL_SWEEP[names["both-sides-negative"]]
    assert (r[2] - r[0]) * (r[3] - r[1]) > 0 and R.roi_samples(r, 7, 4, 40, 48)[0] is None


def test_roi_edge_hits_every_target_on_every_level_and_axis():
    assert np.isfinite(R.ROI_EDGE).all() and np.abs(R.ROI_EDGE).max() <= 20000
    lv, dec = R.level_ref(R.ROI_EDGE)
    assert dec.all()
    hit = set()
    for roi, level, tgt in zip(R.ROI_EDGE, lv, R.ROI_EDGE_TARGETS):
        if tgt is None:
            continue
        l, axis, tag = tgt
        assert level == l, (tgt, level)
        H, W = R.MAP_HW[l]
        ys, xs = R.roi_samples(roi, R.ROI_P, R.STRIDES[l], H, W)
        for ax, v in (("y", ys), ("x", xs)):
            if axis in (ax, "both"):
                t = R.roi_edge_target_value(l, ax, tag)
                assert (_bits(v) == _bits(t)).any(), (tgt, ax, float(t))
                hit.add((l, ax, tag))
                if axis == "both":
                    hit.add((l, "both", tag))
    for l in range(4):
        for ax in ("y", "x"):
            for tag in ("m1", "zero", "below-m1", "top-1", "top", "above-top"):
                assert (l, ax, tag) in hit, (l, ax, tag)
        for tag in ("m1", "zero", "below-m1", "top-1", "top", "above-top"):
            assert (l, "both", tag) in hit
    # one step outside really is outside, and the step on the border is not
    for l, (H, W) in enumerate(R.MAP_HW):
        bad, *_ = R._edge_rules(np.asarray([R.roi_edge_target_value(l, "y", t) for t in ("m1", "below-m1", "top", "above-top")], F32), H)
        assert bad.tolist() == [False, True, False, True]
    ys, xs = R.roi_samples(R.ROI_EDGE[R.ROI_EDGE_IDS.index("grid-65-columns")], 7, 32, 5, 6)
    assert xs.shape[1] == 65 and ys.shape[1] == 1
    ys, xs = R.roi_samples(R.ROI_EDGE[R.ROI_EDGE_IDS.index("grid-65-rows")], 7, 32, 5, 6)
    assert ys.shape[1] == 65 and xs.shape[1] == 1


def test_decode_cases_keep_their_distance_from_the_validity_border():
    ref = R.decode_pipeline_ref(R.decode_case_preds(), R.DECODE_SHAPES, R.DECODE_K, R.DECODE_IMG_HW, R.DECODE_SIZES, R.DECODE_STRIDES)
    cases, slots = R.decode_cases(), R.decode_case_slots()
    exact_slots = {slots[n] for n, c in cases.items() if c[5]}
    for n, c in cases.items():
        if c[5]:
            assert c[4][2] == 0 and c[4][3] == 0, n                            # exact without expf
    for b in range(2):
        for l, lv in enumerate(ref[b]):
            for j in range(len(lv["idx"])):
                if not np.isfinite(lv["boxes"][j]).all() or lv["margin"][j] == 0 and not lv["exact"][j]:
                    continue                                                   # non-finite: no emptiness decision to be near
                if (l, int(lv["idx"][j])) in exact_slots or lv["exact"][j]:
                    assert lv["exact"][j]
                    continue
                assert abs(lv["margin"][j]) > 1e-3, (b, l, j, lv["margin"][j])
    # the two border cases: zero width exactly, and one step of width
    lv = ref[0][0]
    j0 = int(np.nonzero(lv["idx"] == slots["zero-width-at-left-border"][1])[0][0])
    j1 = int(np.nonzero(lv["idx"] == slots["one-step-of-width"][1])[0][0])
    assert lv["boxes"][j0][2] == 0.0 and lv["margin"][j0] == 0.0 and not lv["valid"][j0]
    assert lv["boxes"][j1][2] == 2.0 ** -20 and lv["valid"][j1]
    j2 = int(np.nonzero(ref[1][0]["idx"] == slots["zero-width-at-image-1-border"][1])[0][0])
    assert ref[1][0]["boxes"][j2][0] == ref[1][0]["boxes"][j2][2] == 12.0 and not ref[1][0]["valid"][j2]


def test_nms_edge_thresholds_are_hit_exactly():
    cases = {c[0]: c for c in R.NMS_EDGE}
    for name in R.NMS_ON_THRESHOLD:
        _, boxes, cats, th, _, (i, j) = cases[name]
        assert _bits(R.iou_ref(boxes[i], boxes[j:j + 1]))[0] == _bits(F32(th))[()], name
        assert _bits(R.iou_ref(boxes[j], boxes[i:i + 1]))[0] == _bits(F32(th))[()], name
    for name in R.NMS_ABOVE_THRESHOLD:
        _, boxes, cats, th, _, (i, j) = cases[name]
        assert _bits(R.iou_ref(boxes[i], boxes[j:j + 1]))[0] == _bits(np.nextafter(F32(th), F32(1)))[()], name
    assert np.isnan(R.iou_ref(cases["zero-area-duplicates"][1][0], cases["zero-area-duplicates"][1][1:2]))[0]      # 0 / 0
    assert R.iou_ref(cases["duplicates"][1][0], cases["duplicates"][1][1:2])[0] == 1.0
    for _, boxes, _, _, _, _ in R.NMS_EDGE:
        assert np.array_equal(boxes, np.round(boxes)) and np.abs(boxes).max() < 2 ** 24
    d = cases["chunk-all-disjoint"][1]
    assert len(d) == 64 and all(not (R.iou_ref(d[i], d[i + 1:]) > 0).any() for i in range(63))
    o = cases["chunk-one-overlap"][1]
    assert sum(int((R.iou_ref(o[i], o[i + 1:]) > 0).sum()) for i in range(63)) == 1
