"""The references of tests/train_fwd_ref.py on the CPU: agreement with oracle/train.py where the two must agree (matcher + pairwise_iou,
sample_k, get_deltas and the torch restatements of the regression losses, rasterize_polygon_within_box), the loss gradients against float64
autograd, every seeded defect caught by a named case (CATCHES), and every case's own coverage conditions."""
import numpy as np
import pytest
import torch

import train_fwd_cases as Cs
import train_fwd_ref as R
from oracle import maskrcnn as M, train as T

F32 = np.float32
cases = Cs.cases


def label_ref(c, defect=None):
    return R.anchor_labels_ref(c["levels"], c["cells"], c["gt"], c["lo"], c["hi"], defect)


def differs(a, b):
    if isinstance(a, LossOut):
        return a.differs(b)
    if isinstance(a, dict):
        return any(differs(a[k], b[k]) for k in ("match_val", "match_idx", "gt_best", "label"))
    if isinstance(a, (tuple, list)):
        return any(differs(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return not np.array_equal(R.bits(a) if a.dtype == np.float32 else a, R.bits(b) if b.dtype == np.float32 else b)


# ---------------------------------------------------------------------------------------------------------------- against the oracle
def test_hash_keys_and_selection_match_the_oracle():
    rng = np.random.default_rng(0)
    for seed, image, stream in ((0, 0, 0), (11, 1, 2), (0xFFFFFFFF, 7, 3)):
        idx = np.arange(5000)
        assert np.array_equal(R.hash32(seed, image, stream, idx), T.hash32(seed, image, stream, idx))
        cand = np.sort(rng.choice(5000, 700, replace=False))
        keys = np.zeros(5000, np.uint32)
        keys[cand] = R.sample_keys_ref(seed, image, stream, cand)
        for k in (0, 1, 128, 700, 900):
            assert np.array_equal(R.select_ref(keys, k), T.sample_k(cand, min(k, len(cand)), seed, image, stream))
    ident = rng.integers(0, 40, size=300)          # repeated identities: ties by ascending index
    keys = R.sample_keys_ref(3, 0, 2, ident)
    assert np.array_equal(R.select_ref(keys, 50), T.sample_k(np.arange(300), 50, 3, 0, 2, ident))
    assert len(set(keys[R.select_ref(keys, 50)].tolist())) < 50


def test_floor_key_seed_inverts_the_hash():
    for image, stream, idx in ((0, 0, 0), (1, 0, 49152), (3, 2, 200017), (0, 3, 0x7FFFFFFF)):
        s = R.floor_key_seed(image, stream, idx)
        assert int(R.hash32(s, image, stream, [idx])[0]) == 0xFFFFFFFF
        assert int(R.sample_keys_ref(s, image, stream, [idx])[0]) == 1 and int(R.sample_keys_ref(s, image, stream, [idx], "key_floor_missing")[0]) == 0
    k = R.sample_keys_ref(5, 1, 0, np.arange(200000))          # a bijection with an odd multiplier: no two indices share a key
    assert len(np.unique(k)) == len(k)


def test_anchors_and_cells_match_the_oracle_and_the_library():
    from ampis_amd import ops
    cells = R.default_cells()
    got = R.anchors_ref(Cs.LV2K, cells)
    want = torch.cat([M.grid_anchors(h, w, s, M.ANCHOR_SIZES[l]) for l, (h, w, s) in enumerate(Cs.LV2K)]).numpy()
    assert np.array_equal(R.bits(got), R.bits(want))
    for sizes, ratios in (((32, 64, 128, 256, 512), None), (Cs.SIZES_A9, list(Cs.RATIOS)), ([[s] for s in (32, 64, 128, 256, 512)], [1.0])):
        lib_cells = ops.cell_anchors(sizes=sizes, ratios=ratios)
        mine = R.default_cells([s[0] if ratios == [1.0] else s for s in sizes] if ratios == [1.0] else sizes, tuple(ratios) if ratios else Cs.RATIOS)
        for a, b in zip(lib_cells, mine):
            assert np.array_equal(R.bits(np.asarray(a, F32)[:len(b)]), R.bits(b))


@pytest.mark.parametrize("name", ["thresholds-a9", "a1-g1-b1", "dups-g300", "counts", "waves"])
def test_anchor_labels_match_matcher_and_pairwise_iou(name):
    c = cases("label_cases")[name]
    r = label_ref(c)
    anc = torch.from_numpy(R.anchors_ref(c["levels"], c["cells"]))
    g0 = 0
    for b, gt in enumerate(c["gt"]):
        mq = T.pairwise_iou(torch.from_numpy(np.asarray(gt, F32).reshape(-1, 4)), anc)
        matches, ml = T.matcher(mq, (F32(c["lo"]), F32(c["hi"])), (0, -1, 1), True)
        assert np.array_equal(ml.numpy(), r["label"][b]), (name, b)
        if len(gt):
            assert np.array_equal(matches.numpy(), r["match_idx"][b])
            assert np.array_equal(R.bits(mq.max(dim=0)[0].numpy()), R.bits(r["match_val"][b]))
            assert np.array_equal(R.bits(mq.max(dim=1)[0].numpy()), r["gt_best"][g0:g0 + len(gt)])
        else:
            assert not r["label"][b].any() and not r["match_val"][b].any()
        g0 += len(gt)


@pytest.mark.parametrize("name", ["2k/more-pos", "2k/fewer-pos", "180/scarce", "50k/pos-across-chunks", "2k/floor-key", "2k/pos-max-0", "2k/batch-1"])
def test_rpn_sampler_matches_sample_k(name):
    c = cases("rpn_sample_cases")[name]
    sampled, counts = R.rpn_sample_ref(c["label"], c["seed"], c["batch"], c["pos_max"])
    for b in range(c["B"]):
        pos_all, neg_all = np.flatnonzero(c["label"][b] == 1), np.flatnonzero(c["label"][b] == 0)
        npos = min(len(pos_all), c["pos_max"])
        nneg = min(len(neg_all), c["batch"] - npos)
        want = np.concatenate([T.sample_k(pos_all, npos, c["seed"], b, 0), T.sample_k(neg_all, nneg, c["seed"], b, 1)])
        assert (counts[b] == (npos, nneg)).all() and np.array_equal(sampled[b, :npos + nneg], want)


@pytest.mark.parametrize("name", ["empty-edges", "n-below-batch", "n-1025", "iou-edges", "repeated-identities", "floor-key"])
def test_roi_sampler_matches_the_oracle_steps(name):
    d = cases("roi_sample_cases")[name]
    rois, roi_cls, roi_gti, counts = Cs.roi_ref_of(d)
    K = d["K"]
    for b in range(d["B"]):
        P = min(int(d["count"][b]), d["Pcap"])
        gtb = torch.from_numpy(d["gt"][b].reshape(-1, 4))
        pb = torch.cat([torch.from_numpy(d["prop"][b, :P]), gtb])
        mq = T.pairwise_iou(gtb, pb)
        matches, ml = T.matcher(mq, (F32(d["thresh"]),), (0, 1), False)
        cls = torch.from_numpy(d["cls"][b].astype(np.int64))[matches].clone() if len(gtb) else torch.full((len(pb),), K)
        cls[ml == 0] = K
        fg_all, bg_all = torch.nonzero(cls != K).squeeze(1).numpy(), torch.nonzero(cls == K).squeeze(1).numpy()
        nfg = min(len(fg_all), d["fg_max"])
        nbg = min(len(bg_all), d["batch"] - nfg)
        ident = np.concatenate([d["anchor"][b, :P], d["num_anchors"] + np.arange(len(gtb))])
        sel = np.concatenate([T.sample_k(fg_all, nfg, d["seed"], b, 2, ident), T.sample_k(bg_all, nbg, d["seed"], b, 3, ident)]).astype(np.int64)
        n = nfg + nbg
        assert (counts[b] == (nfg, nbg)).all()
        assert np.array_equal(R.bits(rois[b, :n]), R.bits(pb[sel].numpy())) and np.array_equal(roi_cls[b, :n], cls[sel].numpy())
        assert np.array_equal(roi_gti[b, :n], matches[sel].numpy())
        assert (roi_cls[b, n:] == -1).all() and not rois[b, n:].any()


def test_mask_targets_match_the_oracle_and_the_ratio_instances_differ():
    for name, polys, box in cases("mask_cases"):
        want = T.rasterize_polygon_within_box([np.asarray(p) for p in polys], box, 28)
        assert np.array_equal(R.mask_target_ref(polys, box, "double"), want), name
        if name.startswith("ratio-"):          # the instances the two precisions of 28 / max(side, 0.1) disagree on
            assert not np.array_equal(R.mask_target_ref(polys, box, "float"), want), name
            assert all(float(v) == int(v) for p in polys for v in p)
    by = {n: R.mask_target_ref(p, b) for n, p, b in cases("mask_cases")}
    assert by["covering"].all() and not by["outside"].any()
    for m in (7, 52, 99):          # the two sides of a rounding boundary give different targets; at and above it the same
        assert not np.array_equal(by[f"boundary-{m}-below"], by[f"boundary-{m}-at"]) and np.array_equal(by[f"boundary-{m}-at"], by[f"boundary-{m}-above"])


# ---------------------------------------------------------------------------------------------------------------- losses
def _torch_reg(mode, beta, pd, src, tgt, w):
    from test_loss_cfg_gpu import giou_parts, smooth_l1
    if mode == "giou":
        return giou_parts(M.apply_deltas(pd, src, w), tgt).sum()
    return smooth_l1(pd - T.get_deltas(src, tgt, w), beta if mode == "smooth_l1" else 0.0)


def tie_cells(mode, p4, src, gt, w):
    """[n, 4] bool: the delta gradients that float64 autograd may choose otherwise than the kernel, because the kernel decides them on fp32 bits
    that double arithmetic does not reproduce: d == 0 in fp32 (L1 / smooth-L1: the double difference is not 0), a predicted corner equal to the
    GT corner (GIoU: the pinned subgradient; autograd splits the tie, which moves the whole row), a scale delta exactly at the fp32 clamp
    constant (not clamped by the kernel, clamped against the double constant)."""
    p4, src, gt = np.asarray(p4, F32), np.asarray(src, F32), np.asarray(gt, F32)
    tie = np.zeros(p4.shape, bool)
    if mode == "giou":
        x = R.giou_ref([p4[:, q] for q in range(4)], src, w, gt)[2]["corners"]
        tie[np.logical_or.reduce([c.x & (c.f == gt[:, q]) for q, c in enumerate(x)])] = True
        for q in (2, 3):
            tie[:, q] |= p4[:, q] / F32(w[q]) == R.SCALE_CLAMP
    else:
        t = R.deltas_ref(src, gt, w)
        for q in range(4):
            tie[:, q] = (p4[:, q] - t[q].f) == 0
    return tie


@pytest.mark.parametrize("name", ["k3-b64-l1", "k3-b64-smooth_l1", "k3-b64-giou", "k80-b64-giou", "k1-b2048-smooth_l1", "k3-b1-smooth_l1-edge"])
def test_box_loss_reference_against_float64_autograd_and_the_restatements(name):
    d = cases("box_loss_cases")[name]
    R.E.unsafe.clear()
    partial, gm = Cs.box_loss_ref_of(d)
    assert not R.E.unsafe, R.E.unsafe
    K, batch, B = d["K"], d["batch"], d["B"]
    pred = torch.from_numpy(d["pred"].astype(np.float64)).requires_grad_(True)
    cls = torch.from_numpy(d["roi_cls"].reshape(-1).astype(np.int64))
    used = torch.nonzero(cls >= 0).squeeze(1)
    ce = torch.nn.functional.cross_entropy(pred[used, :K + 1], cls[used], reduction="sum")
    fg = torch.nonzero((cls >= 0) & (cls < K)).squeeze(1)
    src = torch.from_numpy(d["rois"].reshape(-1, 4).astype(np.float64))[fg]
    gt_all = np.concatenate([g.reshape(-1, 4) for g in d["roi"]["gt"]]).astype(np.float64)
    goff = np.concatenate([[0], np.cumsum([len(g) for g in d["roi"]["gt"]])])
    tgt = torch.from_numpy(gt_all[goff[fg.numpy() // batch] + d["roi_gti"].reshape(-1)[fg.numpy()]])
    pd = pred[:, K + 1:K + 1 + 4 * K].reshape(-1, K, 4)[fg, cls[fg]]
    loc = _torch_reg(d["mode"], d["beta"], pd, src, tgt, d["w"])
    inv = float(F32(1) / F32(d["total_rois"]))
    (ce * inv + loc * float(F32(inv) * F32(d["w_reg"]))).backward()
    got_ce, got_loc = sum(float(p[0].v) for p in partial), sum(float(p[1].v) for p in partial)
    assert got_ce == pytest.approx(float(ce.detach()), rel=1e-9) and got_loc == pytest.approx(float(loc.detach()), rel=1e-6)          # giou: the fp32 eps / clamp constants
    # the gradient: EVERY cell within 1e-6 of autograd (the fp32 constants eps = 1e-7f and 0.1f against their doubles) but the listed ties
    ref = pred.grad.numpy()
    tie = np.zeros(ref.shape, bool)
    fgn, cfg = fg.numpy(), cls[fg].numpy()
    col = K + 1 + 4 * cfg
    p4 = np.stack([d["pred"][fgn, col + q] for q in range(4)], 1)
    t4 = tie_cells(d["mode"], p4, d["rois"].reshape(-1, 4)[fgn], tgt.numpy(), d["w"])
    for q in range(4):
        tie[fgn, col + q] = t4[:, q]
    err, scale = np.abs(gm.v - ref), np.abs(ref).max()
    assert (err[~tie] <= 1e-6 * scale).all(), (float(err[~tie].max()), np.argwhere((err > 1e-6 * scale) & ~tie)[:4].tolist())
    print(f"{name}: {int((~tie).sum())} cells within 1e-6 of autograd, {int(tie.sum())} ties ({int((tie & (err > 1e-6 * scale)).sum())} of them decided otherwise)")
    assert tie.sum() < 0.5 * 4 * len(fgn) or len(fgn) <= 2          # the appended GT boxes (source == GT) are about a third of the foreground
    assert gm.written.all() and not gm.v[:, 5 * K + 1:].any()


@pytest.mark.parametrize("name", ["a3-l1-b256-p128", "a3-smooth_l1-b256-p128", "a3-giou-b256-p128", "a9-giou-b256-p128", "a3-giou-b1-p1", "a3-smooth_l1-edge-b1-p1"])
def test_rpn_loss_reference_against_the_restatements(name):
    d = cases("rpn_loss_cases")[name]
    R.E.unsafe.clear()
    partial, maps = Cs.rpn_loss_ref_of(d)
    assert not R.E.unsafe, R.E.unsafe
    A, off = d["A"], R.level_offsets(d["levels"], d["A"])
    anc = torch.from_numpy(R.anchors_ref(d["levels"], d["cells"]).astype(np.float64))
    preds = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in d["preds"]]
    bce, loc = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for b in range(2):
        npos, nneg = d["counts"][b]
        an = d["sampled"][b, :npos + nneg].astype(np.int64)
        lvl = np.searchsorted(off, an, side="right") - 1
        pix, k = (an - off[lvl]) // A, (an - off[lvl]) % A
        logits = torch.stack([preds[l][b, p, kk] for l, p, kk in zip(lvl, pix, k)])
        bce = bce + torch.nn.functional.binary_cross_entropy_with_logits(logits, (torch.arange(len(an)) < npos).double(), reduction="sum")
        if npos:
            pd = torch.stack([preds[l][b, p, A + 4 * kk:A + 4 * kk + 4] for l, p, kk in zip(lvl[:npos], pix[:npos], k[:npos])])
            gtb = torch.from_numpy(d["gt"][b].astype(np.float64))[d["lab"]["match_idx"][b][an[:npos]].astype(np.int64)]
            loc = loc + _torch_reg(d["mode"], d["beta"], pd, anc[an[:npos]], gtb, (1.0, 1.0, 1.0, 1.0))
    assert sum(float(p[0].v) for p in partial) == pytest.approx(float(bce.detach()), rel=1e-9)
    assert sum(float(p[1].v) for p in partial) == pytest.approx(float(loc.detach()), rel=1e-6, abs=1e-9)
    inv = F32(1) / F32(d["batch"] * 2)
    (bce * float(inv * F32(d["w_cls"])) + loc * float(inv * F32(d["w_cls"]) * F32(d["w_loc"]))).backward()
    ties = [np.zeros(m.v.shape, bool) for m in maps]          # the delta cells the kernel decides on fp32 bits (tie_cells)
    anc32 = R.anchors_ref(d["levels"], d["cells"])
    for b in range(2):
        npos = int(d["counts"][b, 0])
        an = d["sampled"][b, :npos].astype(np.int64)
        lvl = np.searchsorted(off, an, side="right") - 1
        pix, k = (an - off[lvl]) // A, (an - off[lvl]) % A
        if npos:
            p4 = np.stack([d["preds"][l][b, px, A + 4 * kk:A + 4 * kk + 4] for l, px, kk in zip(lvl, pix, k)])
            t4 = tie_cells(d["mode"], p4, anc32[an], d["gt"][b][d["lab"]["match_idx"][b][an]], (1.0, 1.0, 1.0, 1.0))
            for i in range(npos):
                ties[lvl[i]][b, pix[i], A + 4 * k[i]:A + 4 * k[i] + 4] = t4[i]
    scale = max(float(p.grad.abs().max()) for p in preds if p.grad is not None)
    for m, p, tie in zip(maps, preds, ties):
        ref = p.grad.numpy() if p.grad is not None else np.zeros(m.v.shape)
        err = np.abs(m.v - ref)
        assert err[..., :A].max() <= 1e-9
        assert (err[~tie] <= 1e-6 * scale).all(), (float(err[~tie].max()), np.argwhere((err > 1e-6 * scale) & ~tie)[:4].tolist())
        assert not m.written[..., 5 * A:].any() and not m.v[~m.written].any()
    assert sum(int(t.sum()) for t in ties) < 0.5 * 4 * int(d["counts"][:, 0].sum()) or d["batch"] == 1
    n = int(d["counts"].sum())
    assert sum(int(m.written[..., :A].sum()) for m in maps) == n and sum(int(m.written[..., A:].sum()) for m in maps) == 4 * int(d["counts"][:, 0].sum())


def test_deltas_match_get_deltas():
    rng = np.random.default_rng(4)
    src, gt = Cs._rand_gt(rng, 200, 0, 300), Cs._rand_gt(rng, 200, 0, 300)
    for w in ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)):
        t = R.deltas_ref(src, gt, w)
        want = T.get_deltas(torch.from_numpy(src), torch.from_numpy(gt), w).numpy()
        for q in range(4):
            if q < 2:
                assert t[q].x.all() and np.array_equal(R.bits(t[q].f), R.bits(want[:, q]))
            else:
                assert (np.abs(want[:, q] - t[q].v) <= t[q].e).all()


@pytest.mark.parametrize("name", ["g0-a0.25", "g1-a-1", "g2-a0.25", "g2-a-1", "single-g1-a0.25"])
def test_focal_reference_against_float64_autograd(name):
    x, labels, K, alpha, gamma, scale = cases("focal_cases")[name]
    loss, grad = R.focal_ref(x, labels, K, alpha, gamma, scale)
    assert np.isfinite(loss.v).all() and np.isfinite(grad.v).all() and np.isfinite(loss.e).all() and np.isfinite(grad.e).all()
    X = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy((labels[:, None] == np.arange(K)[None, :]).astype(np.float64))
    p = torch.sigmoid(X)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(X, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    l = ce * ((1 - pt) ** gamma)
    if alpha >= 0:
        l = (float(F32(alpha)) * t + (1 - float(F32(alpha))) * (1 - t)) * l
    live = torch.from_numpy(labels >= 0)[:, None].expand_as(l)
    l = torch.where(live, l, torch.zeros_like(l))
    (l.sum() * float(F32(scale))).backward()
    assert np.abs(loss.v - l.detach().numpy()).max() <= 1e-9 * max(1.0, float(l.detach().max()))
    sat = np.abs(x) > 50          # 1 - sigmoid saturates in float64 as well: the product rule's two terms are compared where they exist
    assert np.abs(grad.v - X.grad.numpy())[~sat].max() <= 1e-9
    assert not grad.v[labels < 0].any() and not loss.v[labels < 0].any() and (labels == K).any() and (labels < 0).any()


# ---------------------------------------------------------------------------------------------------------------- seeded defects
CATCHES = {
    "last_max_wins": [("label", "dups-g300")],
    "thresholds_strict": [("label", "thresholds-a9")],
    "lowq_skips_zero_best": [("label", "waves")],
    "second_gt_tile_dropped": [("label", "dups-g300"), ("label", "counts")],
    "lane_chunk_63_dropped": [("label", "dups-g300"), ("label", "counts")],
    "key_floor_missing": [("rpn", "180/floor-key"), ("rpn", "2k/floor-key"), ("rpn", "50k/floor-key")],
    "neg_quota_ignores_npos": [("rpn", "2k/fewer-pos"), ("rpn", "50k/fewer-pos"), ("rpn", "196k/no-pos")],
    "chunk_boundary_off_by_one": [("rpn", "50k/pos-across-chunks")],
    "ties_by_descending_index": [("roi", "repeated-identities")],
    "gt_not_appended": [("roi", "empty-edges"), ("roi", "n-1025"), ("roi", "iou-edges")],
    "iou_thresh_strict": [("roi", "iou-edges")],
    "prop_count_not_clamped": [("roi", "empty-edges")],
    "unused_rows_not_zeroed": [("box", "k3-b64-l1"), ("box", "k80-b64-giou")],
    "deltas_of_class_0": [("box", "k3-b64-smooth_l1"), ("box", "k80-b64-l1")],
    "beta_edge_inclusive": [("box", "k3-b1-smooth_l1-edge"), ("rpn_loss", "a3-smooth_l1-edge-b1-p1")],
    "ratio_in_other_precision": [("mask", f"ratio-{i}") for i in range(6)],
    "bits_row_major": [("mask", "integer-0"), ("mask", "left-and-above")],
}


class LossOut:
    """the outputs of a loss reference as the GPU tests compare them: the written cells, the bits where they are known, the value within its
    bound elsewhere -- so a defect counts as caught only where a kernel that had it would fail R.check_bound or the structure check"""
    def __init__(self, partial, maps):
        self.el = [p[j] for p in partial for j in range(2)] + [m.as_e() for m in (maps if isinstance(maps, list) else [maps])]
        self.written = [m.written for m in (maps if isinstance(maps, list) else [maps])]

    def differs(self, bad):
        if any(not np.array_equal(a, b) for a, b in zip(self.written, bad.written)):
            return True
        for g, b in zip(self.el, bad.el):
            dev = np.where(b.x, b.f.astype(np.float64), b.v)          # what a kernel with the defect holds
            if (g.x & (R.bits(dev.astype(F32)) != R.bits(g.f))).any() or (~g.x & (np.abs(dev - g.v) > g.e)).any():
                return True
        return False


def _ref(kind, name, defect=None):
    if kind == "label":
        return label_ref(cases("label_cases")[name], defect)
    if kind == "rpn":
        c = cases("rpn_sample_cases")[name]
        return R.rpn_sample_ref(c["label"], c["seed"], c["batch"], c["pos_max"], defect)
    if kind == "roi":
        return Cs.roi_ref_of(cases("roi_sample_cases")[name], defect)
    if kind == "box":
        return LossOut(*Cs.box_loss_ref_of(cases("box_loss_cases")[name], defect))
    if kind == "rpn_loss":
        return LossOut(*Cs.rpn_loss_ref_of(cases("rpn_loss_cases")[name], defect))
    polys, box = {n: (p, b) for n, p, b in cases("mask_cases")}[name]
    return R.mask_target_ref(polys, box, defect=defect)


def test_the_catches_table_names_every_defect():
    assert set(CATCHES) == set(R.LABEL_DEFECTS + R.RPN_SAMPLE_DEFECTS + R.ROI_SAMPLE_DEFECTS + R.LOSS_DEFECTS + R.MASK_DEFECTS)
    assert all(CATCHES[d] for d in CATCHES)


@pytest.mark.parametrize("defect", sorted(CATCHES))
def test_every_defect_is_caught(defect):
    for kind, name in CATCHES[defect]:
        assert differs(_ref(kind, name), _ref(kind, name, defect)), (defect, kind, name)


def test_defects_the_plain_cases_cannot_see():
    """what makes the edge cases necessary"""
    assert not differs(_ref("label", "counts"), _ref("label", "counts", "last_max_wins"))                  # no duplicate boxes: no tie
    assert not differs(_ref("label", "counts"), _ref("label", "counts", "thresholds_strict"))              # random IoUs never sit on a threshold
    assert not differs(_ref("rpn", "2k/more-pos"), _ref("rpn", "2k/more-pos", "neg_quota_ignores_npos"))   # npos == pos_max hides the quota rule
    assert not differs(_ref("rpn", "50k/more-pos"), _ref("rpn", "50k/more-pos", "chunk_boundary_off_by_one"))
    assert not differs(_ref("roi", "n-1025"), _ref("roi", "n-1025", "ties_by_descending_index"))           # distinct identities: no tie (the bijection)
    assert not differs(_ref("roi", "n-1025"), _ref("roi", "n-1025", "iou_thresh_strict"))
    assert not differs(_ref("mask", "integer-3"), _ref("mask", "integer-3", "ratio_in_other_precision"))
    # |d| == beta on a row with a logf on its path: the gradient is +-1 on both sides and the one-ulp loss difference drowns in the row's sum
    for kind, name in (("box", "k3-b64-smooth_l1"), ("rpn_loss", "a3-smooth_l1-b256-p128"), ("rpn_loss", "a3-smooth_l1-b1-p1")):
        assert not differs(_ref(kind, name), _ref(kind, name, "beta_edge_inclusive")), (kind, name)


def test_the_name_lists_are_the_tables():
    for names, kind in ((Cs.LABEL_NAMES, "label_cases"), (Cs.RPN_SAMPLE_NAMES, "rpn_sample_cases"), (Cs.ROI_SAMPLE_NAMES, "roi_sample_cases"),
                        (Cs.RPN_LOSS_NAMES, "rpn_loss_cases"), (Cs.BOX_LOSS_NAMES, "box_loss_cases"), (Cs.FOCAL_NAMES, "focal_cases")):
        assert sorted(names) == sorted(cases(kind)) and len(set(names)) == len(names), kind


# ---------------------------------------------------------------------------------------------------------------- coverage conditions
def test_label_cases_hold_their_edges():
    lc = cases("label_cases")
    r = label_ref(lc["thresholds-a9"])
    assert ((r["rule"] == R.RULES.index("hi_eq")) & ~r["lowq"] & (r["label"] == 1)).any()          # labelled 1 by equality with hi alone
    assert ((r["rule"] == R.RULES.index("lo_eq")) & ~r["lowq"] & (r["label"] == -1)).any()         # labelled -1 by equality with lo alone
    assert len(lc["thresholds-a9"]["cells"][0]) == 9 and len(lc["a1-g1-b1"]["cells"][0]) == 1 and len(lc["a1-g1-b1"]["gt"]) == 1
    r, m = label_ref(lc["dups-g300"]), label_ref(lc["dups-g300"], "last_max_wins")
    g = lc["dups-g300"]["gt"][0]
    for i, j in Cs.DUP_PAIRS:          # each pair is some anchor's best: the first index stands, the mutant takes the second
        assert np.array_equal(g[i], g[j]) and ((r["match_idx"][0] == i) & (m["match_idx"][0] == j)).any(), (i, j)
    assert [len(g) for g in lc["counts"]["gt"]] == [1, 64, 65, 256, 257, 300]
    w = lc["waves"]
    anc = R.anchors_ref(w["levels"], w["cells"])
    off = R.level_offsets(w["levels"], 3)
    assert len(anc) == 180 and any(off[l] // 64 == (off[l] - 1) // 64 for l in range(1, 5))          # a wave spans two levels; the last wave is partial
    cov = [R.wave_coverage(anc, g) for g in w["gt"]]
    last = (len(anc) - 1) // 64
    assert cov[0][0] == ({last}, {last})                                   # touches anchors of the last, partial wave only
    assert 0 in cov[0][1][0] and 0 not in cov[0][1][1]                     # inside wave 0's bounding box, none of its anchors
    assert len(w["gt"][1]) == 0 and len(w["gt"][0]) and len(w["gt"][2])    # an image without GT between two that have some
    assert cov[2][0] == (set(), set())                                     # no wave's bounding box
    assert cov[3][0][1] == set() and w["gt"][3][0, 0] == w["gt"][3][0, 2]  # zero area
    r = label_ref(w)
    assert r["zero_best"].tolist() == [False, False, True, True] and (r["label"][2] == 1).all() and not r["label"][1].any() and not r["match_val"][1].any()


def test_rpn_sample_cases_hold_their_edges():
    rc = cases("rpn_sample_cases")
    want_path = {"180": ("one_wg", 1), "2k": ("chunked", 1), "50k": ("chunked", 2), "196k": ("chunked", 5)}
    for name, c in rc.items():
        shape = name.split("/")[0]
        N = Cs.total(c["levels"])
        path = R.rpn_sample_path_ref(N, c["B"], c["batch"])
        sampled, counts = R.rpn_sample_ref(c["label"], c["seed"], c["batch"], c["pos_max"])
        npos_c, nneg_c = (c["label"] == 1).sum(1), (c["label"] == 0).sum(1)
        q = c.get("quota")
        if c["batch"] == 256:
            assert path == want_path[shape], (name, path)
        if q == "batch-512":          # 4 * 512 > 2004 and 5 * 512 > 2048: the one-workgroup selection over memory
            assert path[0] == ("chunked" if shape == "50k" else "one_wg"), (name, path)
        if q == "more-pos":
            assert (npos_c > c["pos_max"]).all() and (counts[:, 0] == c["pos_max"]).all()
        if q == "fewer-pos":
            assert (npos_c < c["pos_max"]).all() and (counts[:, 1] == np.minimum(c["batch"] - npos_c, nneg_c)).all() and (counts[:, 0] == npos_c).all()
        if q == "scarce":
            assert (counts.sum(1) < c["batch"]).all() and (counts.sum(1) == npos_c + nneg_c).all()
        if q == "no-pos":
            assert not npos_c.any() and (counts[:, 0] == 0).all() and (counts[:, 1] > 0).all()
        if q == "no-neg":
            assert not nneg_c.any() and (counts[:, 1] == 0).all() and (counts[:, 0] == c["pos_max"]).all()
        if q == "pos-max-0":
            assert c["pos_max"] == 0 and npos_c.all() and (counts[:, 0] == 0).all() and (counts[:, 1] > 0).all()
        if q == "batch-1":
            assert c["batch"] == 1 and (counts.sum(1) == 1).all()
        if "floor" in c:
            b, idx = c["floor"]
            assert counts[b, 0] < c["pos_max"] and sampled[b, counts[b, 0] - 1] == idx          # scarce: still taken, and last
    ch = R.SAMPLE_CHUNK
    s, k = R.rpn_sample_ref(rc["50k/pos-in-second-chunk"]["label"], 7, 256, 128)
    assert all((s[b, :k[b, 0]] >= ch).all() and k[b, 0] == 128 for b in range(2))
    s, k = R.rpn_sample_ref(rc["50k/pos-across-chunks"]["label"], 8, 256, 128)
    assert all({ch - 1, ch} <= set(s[b, :k[b, 0]].tolist()) for b in range(2))
    lab = rc["50k/thin-second-chunk"]["label"]
    assert (((lab[:, ch:] == 0).sum(1) < 256) & ((lab[:, ch:] == 0).sum(1) > 0)).all() and not (lab[:, ch:] == 1).any()
    c = rc["2k/same-labels-two-images"]
    s, k = R.rpn_sample_ref(c["label"], c["seed"], 256, 128)
    assert np.array_equal(c["label"][0], c["label"][1]) and not np.array_equal(s[0], s[1])          # only the image term of the hash differs


def test_roi_sample_cases_hold_their_edges():
    rc = cases("roi_sample_cases")
    d = rc["empty-edges"]
    G = [len(g) for g in d["gt"]]
    assert (d["count"][0] == 0 and G[0] > 0) and (d["count"][1] > 0 and G[1] == 0) and (d["count"][2] == 0 and G[2] == 0) and d["count"][3] > d["Pcap"]
    assert Cs.roi_ref_of(d)[3].tolist()[2] == [0, 0]
    d = rc["n-below-batch"]
    assert all(min(int(c), d["Pcap"]) + len(g) < d["batch"] for c, g in zip(d["count"], d["gt"])) and d["K"] == 80
    r = Cs.roi_ref_of(d)
    assert (r[3][:, 0] < d["fg_max"]).all() and (r[1][0, r[3][0].sum():] == -1).all()          # the cap does not bind; unused slots
    d = rc["n-1025"]
    assert int(d["count"][0]) + len(d["gt"][0]) == 1025 and (Cs.roi_ref_of(d)[3][:, 0] == d["fg_max"]).all()          # the cap binds
    d = rc["n-8193-batch-2048"]
    assert int(d["count"][0]) + len(d["gt"][0]) == 8193 and d["batch"] == 2048 and d["K"] == 1
    d = rc["iou-edges"]
    q = R.iou_ref(d["gt"][0], d["prop"][0])
    assert q[0, 0] == F32(0.5) == F32(d["thresh"]) and 0 < q[0, 2] < F32(0.5) and q[1, 1] == q[2, 1] == 1
    r = Cs.roi_ref_of(d)
    n = int(r[3][0].sum())
    rows = {tuple(b): (c, g) for b, c, g in zip(r[0][0, :n].tolist(), r[1][0, :n].tolist(), r[2][0, :n].tolist())}
    assert rows[(0.0, 0.0, 16.0, 32.0)][0] == 2 and rows[(100.0, 100.0, 140.0, 150.0)] == (0, 1) and rows[(60.0, 10.0, 60.0, 30.0)][0] == d["K"]
    d = rc["repeated-identities"]
    r = Cs.roi_ref_of(d)
    fgc = np.flatnonzero(np.concatenate([R.iou_ref(d["gt"][0], d["prop"][0]).max(0) >= F32(0.5), np.ones(len(d["gt"][0]), bool)]))
    assert len(fgc) > d["fg_max"] + len(d["gt"][0]) and r[3][0, 0] == d["fg_max"]
    got = [row for row in r[0][0, :d["fg_max"]].tolist() if row not in d["gt"][0].tolist()]          # the GT boxes have keys of their own
    assert len(got) >= d["fg_max"] - len(d["gt"][0]) > 0          # one identity: a run of equal keys, cut by the cap, in index order
    assert got == d["prop"][0][fgc[:len(got)]].tolist()
    d = rc["floor-key"]
    r = Cs.roi_ref_of(d)
    nfg = int(r[3][0, 0])
    i = int(np.flatnonzero(d["anchor"][0] == d["floor_ident"])[0])
    assert nfg < d["fg_max"] and np.array_equal(r[0][0, nfg - 1], d["prop"][0, i])          # scarce: taken, and last among the foreground


def test_loss_cases_hold_their_edges():
    bc, rl = cases("box_loss_cases"), cases("rpn_loss_cases")
    for name, d in list(bc.items()) + list(rl.items()):
        cv = d["cover"]
        big = d["batch"] > 1
        assert R.reg_mode(d["ltype"], d["beta"]) == d["mode"]          # the host's rule: smooth-L1 below beta 1e-5 runs the L1 kernel
        if d["mode"] == "l1" and int(d["counts"][:, 0].sum()):
            assert cv["d_zero"] >= 1, name
        if d["mode"] == "smooth_l1" and big:
            assert cv["beta_edge"] >= 1, name
        if d["mode"] == "giou" and big:
            assert cv["clamp_at"] >= 1 and cv["clamp_above"] >= 1 and cv["equal"] >= 1, name
        if big:
            assert cv["big_logit"] >= 2 and cv["equal"] >= 1, name
    for name in ("k3-b64-giou", "a3-giou-b256-p128", "a9-giou-b256-p128"):
        d = (bc if name in bc else rl)[name]
        if name in bc:
            b = 2
            fg = np.flatnonzero((d["roi_cls"][b] >= 0) & (d["roi_cls"][b] < d["K"]))
            col = d["K"] + 1 + 4 * d["roi_cls"][b, fg]
            p = [d["pred"][b * d["batch"] + fg, col + q] for q in range(4)]
            src, gt, w = d["rois"][b, fg], d["roi"]["gt"][b][d["roi_gti"][b, fg]], d["w"]
        else:
            b, A, off = 0, d["A"], R.level_offsets(d["levels"], d["A"])
            an = d["sampled"][b, :d["counts"][b, 0]].astype(np.int64)
            lvl = np.searchsorted(off, an, side="right") - 1
            pix, k = (an - off[lvl]) // A, (an - off[lvl]) % A
            p = [np.asarray([d["preds"][l][b, px, A + 4 * kk + q] for l, px, kk in zip(lvl, pix, k)], F32) for q in range(4)]
            src, gt, w = R.anchors_ref(d["levels"], d["cells"])[an], d["gt"][b][d["lab"]["match_idx"][b][an]], (1.0, 1.0, 1.0, 1.0)
        R.E.unsafe.clear()
        loss, grad, info = R.giou_ref(p, src, w, gt)
        assert not R.E.unsafe and {"disjoint", "nested", "partial"} <= set(info["kind"].tolist()), (name, set(info["kind"].tolist()))
        cw, ch = info["clamped_w"], info["clamped_h"]
        at = (np.asarray(p[2], F32) / F32(w[2]) == R.SCALE_CLAMP)
        assert at.any() and not cw[at].any() and (grad[2].v[at] != 0).all()          # at the clamp: not clamped, a gradient
        assert ch.any() and not grad[3].v[ch].any()                                   # one ulp above: gradient 0
        x1, y1, x2, y2 = info["corners"]
        eq = x1.x & (x1.f == gt[:, 0]) & (y1.f == gt[:, 1]) & (x2.f == gt[:, 2]) & (y2.f == gt[:, 3])
        # the pinned subgradient: neither the I-term nor the C-term, so only gU (I / (U + eps)^2 - 1 / (C + eps), ~1e-11 with I = U = C) is
        # left: it cancels in dx, dy and stays in dw, dh; no transcendental on the path (expf(0) = 1), so the reference knows the bits
        assert eq.any() and not grad[0].v[eq].any() and not grad[1].v[eq].any() and (np.abs(grad[2].v[eq]) < 1e-6).all() and (loss.v[eq] < 1e-6).all()
        assert all(g.x[eq].all() for g in grad) and loss.x[eq].all()
    d = bc["k3-b64-l1"]
    assert (d["roi_cls"][0] == -1).any() and (d["roi_cls"][1] == d["K"]).all() and (d["roi_cls"][2] >= 0).all()          # unused rows; all background
    assert bc["k80-b64-l1"]["ld"] == 416 and bc["k1-b64-l1"]["ld"] == 16 and bc["k1-b2048-l1"]["batch"] == 2048
    assert (bc["k1-b2048-l1"]["roi_cls"][0, 512:] == 0).any()          # foreground rows beyond the first 512
    for name, ref_of in (("k3-b1-smooth_l1-edge", Cs.box_loss_ref_of), ("a3-smooth_l1-edge-b1-p1", Cs.rpn_loss_ref_of)):
        d = (bc if name in bc else rl)[name]          # |d| == beta with exact zeros as targets: the regression sum of each image is ONE exact term
        good, bad = ref_of(d)[0], ref_of(d, "beta_edge_inclusive")[0]
        assert d["batch"] == 1 and d["cover"]["beta_edge_exact"] == 2 and (d["counts"] == (1, 0)).all()
        for b in range(2):          # linear: |d| - 0.5 beta; the quadratic branch gives 0.5 d^2 / beta, one ulp above
            assert good[b][1].x and good[b][1].f == F32(0.1) - F32(0.5) * F32(0.1) and bad[b][1].f == np.nextafter(good[b][1].f, F32(1))
    for name in ("k3-b1-l1", "a3-l1-b1-p1", "a3-l1-b1-p0"):
        assert (bc if name in bc else rl)[name]["batch"] == 1
