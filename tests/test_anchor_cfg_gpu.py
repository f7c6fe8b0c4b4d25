"""MODEL.ANCHOR_GENERATOR.{SIZES, ASPECT_RATIOS} on the device: the selection / decode / labelling kernels for A = 1, 3, 5, 9 anchors per
location, the fused RPN head with 32 and 48 predictor rows, end-to-end inference and a training step (forward, backward, sparse == dense)
against the oracle under the same anchors, the unchanged default, and the façade.

The oracle takes A from the weight shapes and the geometry from oracle.maskrcnn.{ANCHOR_SIZES, ANCHOR_RATIOS, cell_anchors}, replaced here
for the duration of a case.  oracle/train.py identifies a proposal for the RoI sampling hash with a literal 3 anchors per location: for
A != 3 a training case uses settings under which no RoI is sub-sampled (asserted on the oracle's own counts) and compares the RoI set as a
set; everything on the RPN side uses true anchor indices and is compared exactly for every A."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DEFAULT_SIZES = [[32], [64], [128], [256], [512]]
SETS = {
    "S1": ([[8], [16], [32], [64], [128]], [0.5, 1, 2]),
    "S2": (DEFAULT_SIZES, [0.33, 0.5, 1, 2, 3]),
    "S3": ([[16, 20, 25], [32, 40, 51], [64, 81, 102], [128, 161, 203], [256, 323, 406]], [0.5, 1, 2]),
    "A1": ([[24], [48], [96], [192], [384]], [0.7]),
    "A3": (DEFAULT_SIZES, [0.5, 1.0, 2.0]),
}


def num_anchors(name):
    return len(SETS[name][0][0]) * len(SETS[name][1])


def oracle_anchors(mp, sizes, ratios):
    """oracle.maskrcnn under the anchors (sizes per level, ratios): generate_cell_anchors restated for several sizes."""
    from oracle import maskrcnn as O

    def cell(size):
        rows = []
        for s in (size if isinstance(size, (tuple, list)) else (size,)):
            area = float(s) ** 2
            for r in O.ANCHOR_RATIOS:
                w = math.sqrt(area / r)
                h = r * w
                rows.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
        return torch.tensor(rows, dtype=torch.float32)

    mp.setattr(O, "ANCHOR_SIZES", tuple(tuple(s) for s in sizes))
    mp.setattr(O, "ANCHOR_RATIOS", tuple(float(r) for r in ratios))
    mp.setattr(O, "cell_anchors", cell)


def model_kw(name):
    sizes, ratios = SETS[name]
    return dict(anchor_sizes=sizes, aspect_ratios=[ratios])


# ------------------------------------------------------------------------------------------------------------------ op level
def _levels(B, rng, shapes, A):
    ld = 16 * ((5 * A + 15) // 16)
    preds = []
    for (h, w) in shapes:
        p = rng.normal(0, 2, (B, h * w, ld)).astype(np.float32)
        p[:, :, :A] = np.round(p[:, :, :A] * 4) / 4          # ties: the index tie-break is exercised
        p[:, :, A:] *= 0.3
        p[:, :, 5 * A:] = 0
        preds.append(torch.from_numpy(p))
    return preds


@pytest.mark.parametrize("name", ["A1", "A3", "S2", "S3"])
def test_rpn_topk_and_decode_for_other_anchor_counts(gpu_ctx, name, monkeypatch):
    """amp_rpn_topk + amp_rpn_decode (+ the sort) against rpn_select_candidates under the same anchors, to the exactness of
    tests/test_stages_gpu.py::test_rpn_decode_and_sort: order and logits exact, boxes to 1e-4 px."""
    from ampis_amd import ops
    from oracle import maskrcnn as O
    sizes, ratios = SETS[name]
    A = num_anchors(name)
    oracle_anchors(monkeypatch, sizes, ratios)
    rng = np.random.default_rng(3 + A)
    B, k, H, W = 2, 300, 200, 176
    shapes = [(50, 44), (25, 22), (13, 11), (7, 6), (4, 3)]
    preds = _levels(B, rng, shapes, A)
    dp = [p.to(DEV) for p in preds]
    si, sl, sc = ops.rpn_topk(gpu_ctx, dp, shapes, B, k, sizes=sizes, ratios=ratios)
    boxes, keys = ops.rpn_decode(gpu_ctx, dp, shapes, B, k, si, sl, sc, H, W, sizes=sizes, ratios=ratios)
    sb, ss, scat, cnt, pos = ops.sort_gather(gpu_ctx, keys, boxes)
    torch.cuda.synchronize()
    si_h, sc_h = si.cpu().numpy(), sc.cpu().numpy()
    for b in range(B):
        for l, p in enumerate(preds):
            logits = p[b, :, :A].reshape(-1)
            kk = min(k, logits.numel())
            assert sc_h[b, l] == kk
            assert np.array_equal(si_h[b, l, :kk], O.sort_desc_stable(logits)[:kk].numpy()), (b, l)
    cfg = O.Cfg(num_classes=2, pre_nms_topk=k)
    outs = [(p[:, :, :A].reshape(B, -1), p[:, :, A:5 * A].reshape(B, -1, 4)) for p in preds]
    cands = O.rpn_select_candidates(outs, shapes, cfg)
    for b in range(B):
        cb, cl, clv = cands[b][0], cands[b][1], cands[b][2]
        cb = O.clip_boxes(cb, H, W)
        keep = ((cb[:, 2] - cb[:, 0]) > 0) & ((cb[:, 3] - cb[:, 1]) > 0) & torch.isfinite(cb).all(1)
        order = O.sort_desc_stable(cl[keep])
        rb, rl, rv = cb[keep][order].numpy(), cl[keep][order].numpy(), clv[keep][order].numpy()
        n = int(cnt[b].item())
        assert n == len(rb)
        assert np.array_equal(ss[b, :n].cpu().numpy(), rl)
        assert np.array_equal(scat[b, :n].cpu().numpy(), rv)
        assert np.abs(sb[b, :n].cpu().numpy() - rb).max() < 1e-4


@pytest.mark.parametrize("name", ["A1", "S1", "S2", "S3"])
def test_anchor_labels_for_other_anchor_sets(gpu_ctx, name, monkeypatch):
    """amp_anchor_labels against oracle.train.pairwise_iou + matcher under the same anchors: labels, best IoU and best GT of every anchor
    and the best IoU of every GT box, exact (tests/test_train_fwd_gpu.py::test_anchor_labels_edge_cases' comparison)."""
    from ampis_amd import _lib, ops
    from oracle import maskrcnn as M, train as T
    sizes, ratios = SETS[name]
    oracle_anchors(monkeypatch, sizes, ratios)
    rng = np.random.default_rng(11)
    shapes = [(64, 80), (32, 40), (16, 20), (8, 10), (4, 5)]
    H, W = 256, 320

    def boxes(n):
        c = rng.uniform([0, 0], [W, H], size=(n, 2)); s = rng.uniform(4, 120, size=(n, 2))
        return np.concatenate([np.clip(c - s / 2, 0, None), np.minimum(c + s / 2, [W, H])], axis=1).astype(np.float32)

    per_image = [boxes(40), boxes(7)]
    B = len(per_image)
    anchors = torch.cat([M.grid_anchors(h, w, M.STRIDES[l], M.ANCHOR_SIZES[l]) for l, (h, w) in enumerate(shapes)])
    A = anchors.shape[0]
    assert A == num_anchors(name) * sum(h * w for h, w in shapes)
    gt_all = np.concatenate(per_image).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in per_image])]).astype(np.int32)
    d_gt, d_off = torch.from_numpy(gt_all).to(DEV), torch.from_numpy(off).to(DEV)
    ld = 16 * ((5 * num_anchors(name) + 15) // 16)
    dummy = [torch.zeros((B, h * w, ld), device=DEV) for h, w in shapes]
    lv = ops.make_rpn_levels(dummy, shapes, sizes=sizes, ratios=ratios)
    mv = torch.empty((B, A), device=DEV); mi = torch.empty((B, A), dtype=torch.int32, device=DEV)
    best = torch.zeros((len(gt_all),), dtype=torch.int32, device=DEV)
    lab = torch.empty((B, A), dtype=torch.int8, device=DEV)
    ops.check(_lib.lib().amp_anchor_labels(gpu_ctx.handle, C.byref(lv), B, ops.ptr(d_gt), ops.ptr(d_off), int(len(gt_all)), 0.3, 0.7,
                                           ops.ptr(mv), ops.ptr(mi), ops.ptr(best), ops.ptr(lab)), "amp_anchor_labels")
    torch.cuda.synchronize()
    for b in range(B):
        mq = T.pairwise_iou(torch.from_numpy(per_image[b]), anchors)
        matches, ml = T.matcher(mq, (0.3, 0.7), (0, -1, 1), True)
        assert np.array_equal(lab[b].cpu().numpy(), ml.numpy())
        assert np.array_equal(mv[b].cpu().numpy(), mq.max(dim=0)[0].numpy())
        assert np.array_equal(mi[b].cpu().numpy(), matches.numpy().astype(np.int32))
        assert np.array_equal(best[off[b]:off[b + 1]].cpu().numpy().view(np.float32), mq.max(dim=1)[0].numpy())


@pytest.mark.parametrize("A", [5, 9])
def test_fused_wide_rpn_head_matches_the_two_convolutions(gpu_ctx, A):
    """amp_rpn_head_fused_ld with 32 / 48 predictor rows against the two convolutions on the same operands and torch in fp64, under the
    bound of tests/test_stages_gpu.py::test_fused_rpn_head_matches_the_two_convolutions; the pad rows are exactly 0."""
    from ampis_amd import ops, _lib
    if gpu_ctx.conv_mode != gpu_ctx.CONV_F16X3:
        with pytest.raises(_lib.AmpError):
            _lib.check(_lib.lib().amp_rpn_head_fused_ld(gpu_ctx.handle, None, 1, 1, 1, None, None, None, None, 32, None), "amp_rpn_head_fused_ld")
        return
    ld, n = 16 * ((5 * A + 15) // 16), 5 * A
    g = torch.Generator().manual_seed(21 + A)
    B, H, W = 2, 112, 120                                        # 26 880 pixels, ragged against the 128-row tiles
    x = (torch.randn(B, H, W, 256, generator=g).clamp_(min=0)).to(DEV)
    wc = (torch.randn(256, 3, 3, 256, generator=g) * 0.02).to(DEV)
    bc = (torch.randn(256, generator=g) * 0.1).to(DEV)
    wp = torch.zeros(ld, 1, 1, 256); wp[:n] = torch.randn(n, 1, 1, 256, generator=g) * 0.05
    bp = torch.zeros(ld); bp[:n] = torch.randn(n, generator=g) * 0.1
    wp_d, bp_d = wp.to(DEV), bp.to(DEV)
    xs = ops.split_rows(gpu_ctx, x)
    pred = torch.full((B * H * W, ld), 7.0, device=DEV)
    _lib.check(_lib.lib().amp_rpn_head_fused_ld(gpu_ctx.handle, _lib.ptr(xs), B, H, W, _lib.ptr(wc), _lib.ptr(bc), _lib.ptr(wp_d), _lib.ptr(bp_d), ld,
                                                _lib.ptr(pred)), "amp_rpn_head_fused_ld")
    t = ops.conv2d_nhwc(gpu_ctx, x, wc, None, bc, pad=1, relu=True)
    chain = ops.conv2d_nhwc(gpu_ctx, t, wp_d, None, bp_d).reshape(-1, ld)
    torch.cuda.synchronize()
    ref = torch.nn.functional.conv2d(x.cpu().double().permute(0, 3, 1, 2), wc.cpu().double().permute(0, 3, 1, 2), bc.cpu().double(), padding=1).relu()
    ref = torch.nn.functional.conv2d(ref, wp.double().permute(0, 3, 1, 2), bp.double()).permute(0, 2, 3, 1).reshape(-1, ld)
    m = ref.abs().max().item()
    e_chain, e_fused = (chain.cpu().double() - ref).abs().max().item() / m, (pred.cpu().double() - ref).abs().max().item() / m
    print(f"A = {A}: max |pred - fp64| / max: two convolutions", e_chain, "fused", e_fused)
    assert e_fused <= max(1.5 * e_chain, 5e-7), (e_fused, e_chain)
    assert float(pred[:, n:].abs().max()) == 0.0 and float(chain[:, n:].abs().max()) == 0.0      # pad rows stay pad rows
    assert not gpu_ctx.conv_range_flag()


# ------------------------------------------------------------------------------------------------------------------ end to end, inference
def _synth_image(rng, h, w):
    img = rng.normal(60, 12, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(6, 40)
        d = (yy - cy) ** 2 + (xx - cx) ** 2
        img = np.where(d < r * r, rng.normal(190, 15) - 40 * d / (r * r), img)
    img = np.clip(img + rng.normal(0, 4, (h, w)), 0, 255).astype(np.uint8)
    return np.repeat(img[:, :, None], 3, axis=2)


def _decode(m, h, w):
    from ampis_amd import rle
    return rle.decode({"size": [h, w], "counts": m["counts"]}).astype(bool)


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_inference_matches_the_oracle_under_the_same_anchors(gpu_ctx, name):
    """The inputs, the gate and the caps of tests/test_e2e_gpu.py.  Why not a larger frame (whose p2 would take the fused wide head): the
    gate holds a box to max(1e-3 px, 3 ppm of its side), which is the reference's own fp32 noise; on 384 x 512 frames S2's 0.33 / 3 ratios
    produce 432 x 5 px boxes for which the fp32 oracle ITSELF is 1.9e-3 px (4.4 ppm) from its exact-convolution evaluation -- the reference
    violates its own gate there, so such a frame cannot serve as a parity input (asserted below: the oracle's own floor has no violation).
    The fused wide head is held to the two convolutions at op level and inside a training step further down."""
    H, W = 224, 288
    from ampis_amd import params as P
    from ampis_amd.model import MaskRCNN
    from oracle import gate, maskrcnn as O
    K, B, D = 2, 2, 60
    A = num_anchors(name)
    rng = np.random.default_rng(5)
    imgs = np.stack([_synth_image(rng, H, W) for _ in range(B)])
    npp = P.init_params(K, seed=3, style="spread", num_anchors=A)
    cfg = O.Cfg(num_classes=K, detections_per_image=D)
    with pytest.MonkeyPatch.context() as mp:
        oracle_anchors(mp, *SETS[name])
        stages = {}
        ref = O.infer(imgs, O.to_torch_params(npp), cfg, stages=stages)
        if A == 3:
            # not vacuous: on this input the oracle's proposals under the custom anchors are not its proposals under the default anchors
            with pytest.MonkeyPatch.context() as mp2:
                oracle_anchors(mp2, *SETS["A3"])
                st0 = {}
                O.infer(imgs, O.to_torch_params(npp), cfg, stages=st0)
            for b in range(B):
                p1, p0 = stages["props"][b][0].numpy(), st0["props"][b][0].numpy()
                assert p1.shape != p0.shape or np.abs(p1 - p0).max() > 1.0, "the custom anchors change nothing on this input"
        model = MaskRCNN(gpu_ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), detections_per_image=D, **model_kw(name))
        model.load_params(npp)
        out = model.infer(imgs)
        # the predictor maps: A logits, 4 A deltas, zero pad rows
        ld = 16 * ((5 * A + 15) // 16)
        for i, tapname in enumerate(["rpn_pred2", "rpn_pred3", "rpn_pred4", "rpn_pred5", "rpn_pred6"]):
            logits, deltas = stages["rpn_outs"][i]
            got = model.tap(tapname)
            assert got.shape[2] == ld
            HW = got.shape[1]
            r = np.concatenate([logits.numpy().reshape(B, HW, A), deltas.numpy().reshape(B, HW, 4 * A)], axis=2)
            assert float(np.abs(got[:, :, :5 * A] - r).max() / max(1e-6, np.abs(r).max())) < 2e-4, tapname
            assert not got[:, :, 5 * A:].any(), tapname
        st = gate.merge([gate.check_image(o, r, H, W, lambda m: _decode(m, H, W)) for o, r in zip(out, ref)])
        print(f"{name} e2e gate:", gate.summary(st))
        assert st["instances"] > 20 and st["identical"] + st["tie_masks"] == st["instances"]
        _, floor = gate.floor_of(lambda: O.infer(imgs, O.to_torch_params(npp), cfg), (H, W))
        assert floor["violations"] == 0, "the reference's own arithmetic violates the gate on this input: not a parity input"
        print(f"{name} e2e gate |", gate.assert_floor(st, floor, sigmas=3.0, floor_sigmas=2.5))
        model.close()


# ------------------------------------------------------------------------------------------------------------------ training step
def _train_names(npp):
    return [k for k in npp if ".norm." not in k and not k.startswith("backbone.bottom_up.stem") and not k.startswith("backbone.bottom_up.res2")]


# (H, W, synth seed, GT per image, parameter seed, sampling seed) of tests/test_train_fwd_gpu.py and of tests/test_train_bwd_gpu.py
FWD_INPUT = (256, 320, 5, 60, 1, 7)
BWD_INPUT = (192, 256, 9, 40, 2, 3)


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_training_forward_matches_the_oracle_under_the_same_anchors(gpu_ctx, name):
    """The inputs of tests/test_train_fwd_gpu.py: anchor labels and the sampled anchors exact, the RoI set, the five losses to
    test_losses_match_oracle's tolerance, and the sparse RPN backward against the dense one."""
    _training_case(gpu_ctx, name, FWD_INPUT, autograd=False)


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_training_backward_matches_autograd_under_the_same_anchors(gpu_ctx, name):
    """The inputs of tests/test_train_bwd_gpu.py, with its bound: every trainable gradient within 2e-3 of its tensor's largest entry of
    torch autograd of the oracle, the sparse RPN backward live.  The bound goes with that input: on the forward test's 256 x 320 frame
    the fp32 autograd reference is a noisier yardstick for five tensors (res4.*.conv3.weight: 1.5e-3 already with the default anchors,
    2.3e-3 .. 3.1e-3 with S1, against 1.4e-4 / 2.1e-4 on this frame; every other tensor below 7e-4 on both), so the gradients are
    held to autograd here and the forward quantities there."""
    _training_case(gpu_ctx, name, BWD_INPUT, autograd=True)


def _training_case(gpu_ctx, name, inputs, autograd):
    """Anchor labels and the sampled anchors exact; the five losses to test_losses_match_oracle's tolerance; with autograd every
    trainable gradient against torch autograd of the oracle with the sparse RPN backward live (tests/test_train_bwd_gpu.py's bound); the
    sparse backward against the dense one (tests/test_backward_gpu.py::test_sparse_rpn_backward_equals_the_dense_one's bounds)."""
    from ampis_amd import _lib, params as P, synth
    from ampis_amd.model import MaskRCNN
    from oracle import maskrcnn as M, train as T
    H, W, sseed, ngt, pseed, tseed = inputs
    K, B = 2, 2
    A = num_anchors(name)
    imgs, gts = synth.batch(B, H, W, seed=sseed)
    gts = [dict(boxes=g["boxes"][:ngt], classes=g["classes"][:ngt], polygons=g["polygons"][:ngt]) for g in gts]
    npp = P.init_params(K, seed=pseed, style="spread", num_anchors=A)
    names = _train_names(npp)
    full = A == 3        # the oracle's RoI sampling identities are right for A = 3 only: elsewhere nothing may be sub-sampled
    tkw = {} if full else dict(post_nms_topk=256, roi_batch=1024, roi_pos_frac=0.5)
    mkw = {} if full else dict(post_nms_topk_train=256, roi_batch=1024, roi_fg_frac=0.5)
    cfg = T.TrainCfg(num_classes=K, seed=tseed, **tkw)
    with pytest.MonkeyPatch.context() as mp:
        oracle_anchors(mp, *SETS[name])
        tp = M.to_torch_params(npp)
        st, ref_grads = {}, None
        if autograd:
            for k in names:
                tp[k].requires_grad_(True)
            ref = T.forward_losses(imgs, gts, tp, cfg, stages=st)
            sum(ref.values()).backward()
            ref_grads = {k: tp[k].grad.detach().numpy() for k in names}
        else:
            ref = T.forward_losses(imgs, gts, tp, cfg, stages=st)
        ref = {k: float(v.detach()) for k, v in ref.items()}
        anchors = st["anchors"]
        labels_ref = [T.matcher(T.pairwise_iou(torch.as_tensor(gts[b]["boxes"], dtype=torch.float32), anchors), (0.3, 0.7), (0, -1, 1), True)[1].numpy()
                      for b in range(B)]
    if not full:
        for b in range(B):       # the no-sub-sampling condition, on the oracle's own counts
            n_cand = len(st["props"][b]) + len(gts[b]["boxes"])
            n_fg = int((st["roi_cls"][b] != K).sum())
            assert len(st["props"][b]) == 256 and n_cand == 256 + ngt == len(st["rois"][b]) and n_fg <= 512, (n_cand, len(st["rois"][b]), n_fg)
    model = MaskRCNN(gpu_ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), train=True, max_gt=4096, max_poly_doubles=4096 * 64,
                     **mkw, **model_kw(name))
    model.load_params(npp)
    assert model.get_tensor("proposal_generator.rpn_head.anchor_deltas.weight").shape == (4 * A, 256, 1, 1)
    out, ran = {}, {}
    try:
        _lib.lib().amp_debug_set_rpn_train_fuse(0)      # one forward pass for both backward passes
        for on in (0, 1):
            _lib.lib().amp_debug_set_rpn_sparse(on)
            losses = model.forward_losses(imgs, gts, seed=tseed, backward=True)
            out[on] = (losses, {k: model.get_tensor(k, grad=True) for k in names})
            ran[on] = _lib.lib().amp_debug_last_rpn_sparse(model._h)
    finally:
        _lib.lib().amp_debug_set_rpn_sparse(-1)
        _lib.lib().amp_debug_set_rpn_train_fuse(-1)
    assert ran == {0: 0, 1: 1}
    got, grads = out[1]
    # RPN side: exact for every A
    label, sampled, counts = model.tap("rpn_label"), model.tap("rpn_sampled"), model.tap("rpn_counts")
    assert label.shape == (B, anchors.shape[0])
    for b in range(B):
        assert np.array_equal(label[b], labels_ref[b])
        pos, neg, _ = st["rpn_samples"][b]
        assert counts[b, 0] == len(pos) and counts[b, 1] == len(neg) and len(pos) + len(neg) == 256
        assert np.array_equal(sampled[b, :len(pos)], pos.numpy())
        assert np.array_equal(sampled[b, len(pos):len(pos) + len(neg)], neg.numpy())
    # RoI side: the same set (A = 3: the same order too)
    rois, cls, rcounts = model.tap("train_rois"), model.tap("train_roi_cls"), model.tap("train_roi_counts")
    for b in range(B):
        rc, rr = st["roi_cls"][b].numpy(), st["rois"][b].numpy()
        n = len(rc)
        assert rcounts[b, 0] + rcounts[b, 1] == n and rcounts[b, 0] == int((rc != K).sum())
        if full:
            assert np.array_equal(cls[b, :n], rc) and np.abs(rois[b, :n] - rr).max() < 5e-3
        else:
            d = np.abs(rois[b, :n][:, None, :] - rr[None, :, :]).max(axis=2)
            j = d.argmin(axis=1)
            assert d.min(axis=1).max() < 5e-3 and np.array_equal(cls[b, :n], rc[j])
            assert d.min(axis=0).max() < 5e-3                    # every oracle RoI is taken
    for k in ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask"):
        print(name, k, got[k], ref[k])
        assert got[k] == pytest.approx(ref[k], rel=2e-4, abs=1e-6), (k, got[k], ref[k])
    bad, worst = [], (0.0, "")
    for k in (names if autograd else ()):
        g, r = grads[k], ref_grads[k]
        assert g.shape == r.shape, k
        err = float(np.abs(g - r).max()) / max(float(np.abs(r).max()), 1e-8)
        worst = max(worst, (err, k))
        if err > 2e-3:
            bad.append((err, k))
    print(name, "worst gradient against autograd:", worst)
    assert not bad, f"{len(bad)} tensors off: {sorted(bad, reverse=True)[:8]}"
    # sparse == dense on the same forward pass
    assert out[0][0] == out[1][0]
    tol = 2e-5 if gpu_ctx.conv_mode == gpu_ctx.CONV_F16X3 else 1e-4
    for k in names:
        r, g = out[0][1][k], out[1][1][k]
        assert float(np.abs(r).max()) > 0, k
        assert float(np.abs(g - r).max()) / float(np.abs(r).max()) < tol, k
    assert not gpu_ctx.conv_range_flag()
    model.close()


@pytest.mark.parametrize("name", ["S2", "S3"])
def test_training_step_with_the_fused_wide_head(name):
    """A frame large enough for the fused head (p2: 24 576 pixels): the step whose forward pass runs the 32 / 48 predictor rows in the conv's
    epilogue and whose sparse backward recomputes the hidden rows, against the step that saves the hidden tensor -- the bounds of
    tests/test_backward_gpu.py::test_training_forward_with_the_fused_rpn_head_and_recomputed_hidden_rows."""
    from ampis_amd import _lib, params as P, synth
    from ampis_amd.model import MaskRCNN
    ctx = _lib.Context(0)
    if ctx.conv_mode != ctx.CONV_F16X3:
        ctx.close()
        return       # the fused head exists in the f16x3 arithmetic only: both steps would be the same launches
    K, B, H, W = 2, 2, 384, 512
    A = num_anchors(name)
    imgs, gts = synth.batch(B, H, W, first_index=520)
    npp = P.init_params(K, seed=0, style="spread", num_anchors=A)
    m = MaskRCNN(ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=W, train=True, max_gt=B * 800, max_poly_doubles=B * 800 * 64, **model_kw(name))
    m.load_params(npp)
    names = _train_names(npp)
    out = {}
    try:
        for fuse in (0, 1, 1):
            _lib.lib().amp_debug_set_rpn_train_fuse(fuse)
            losses = m.forward_losses(imgs, gts, seed=9, backward=True)
            got = (losses, {k: m.get_tensor(k, grad=True) for k in names}, m.tap("rpn_pred2"), m.tap("rpn_pred4"))
            if fuse in out:
                assert got[0] == out[fuse][0] and all(np.array_equal(got[1][k], out[fuse][1][k]) for k in names)
            out[fuse] = got
    finally:
        _lib.lib().amp_debug_set_rpn_train_fuse(-1)
    assert not ctx.conv_range_flag()
    for t in (2, 3):
        a, b = out[0][t], out[1][t]
        assert float(np.abs(a - b).max()) <= 2e-6 * float(np.abs(a).max())
        assert not a[:, :, 5 * A:].any() and not b[:, :, 5 * A:].any()
    assert not np.array_equal(out[0][2], out[1][2])          # p2 did take the fused head
    for k in out[0][0]:
        assert out[1][0][k] == pytest.approx(out[0][0][k], rel=1e-5), (k, out[0][0], out[1][0])
    for k in names:
        r, g = out[0][1][k], out[1][1][k]
        assert float(np.abs(g - r).max()) / float(np.abs(r).max()) < 5e-3, k
    m.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the default is unchanged
@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_default_anchors_given_explicitly_change_nothing(mode):
    """A model built with the default sizes / ratios passed explicitly against one built without them: detections, RLE strings, losses,
    gradients and the weights after an SGD step bit for bit, in both conv modes."""
    from ampis_amd import _lib, params as P, synth
    from ampis_amd.model import MaskRCNN
    ctx = _lib.Context(0)
    ctx.conv_mode = mode
    K, B, H, W = 2, 2, 384, 512                                   # p2 takes the fused head in f16x3
    imgs, gts = synth.batch(B, H, W, first_index=300)
    npp = P.init_params(K, seed=2, style="spread")
    names = _train_names(npp)
    res = []
    for kw in ({}, dict(anchor_sizes=DEFAULT_SIZES, aspect_ratios=[[0.5, 1.0, 2.0]])):
        m = MaskRCNN(ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=W, train=True, max_gt=B * 800, max_poly_doubles=B * 800 * 64, **kw)
        m.load_params(npp)
        dets = m.infer(imgs)
        losses = m.forward_losses(imgs, gts, seed=3, backward=True)
        grads = {k: m.get_tensor(k, grad=True) for k in names}
        m.sgd_step(0.01, 0.9, 1e-4)
        weights = {k: m.get_tensor(k) for k in names}
        res.append((dets, losses, grads, weights))
        m.close()
    (d0, l0, g0, w0), (d1, l1, g1, w1) = res
    assert sum(len(d["scores"]) for d in d0) > 10
    for a, b in zip(d0, d1):
        assert np.array_equal(a["boxes"], b["boxes"]) and np.array_equal(a["scores"], b["scores"]) and np.array_equal(a["classes"], b["classes"])
        assert [x["counts"] for x in a["masks"]] == [x["counts"] for x in b["masks"]]
    assert l0 == l1
    for k in names:
        assert np.array_equal(g0[k], g1[k]), k
        assert np.array_equal(w0[k], w1[k]), k
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ façade
def _zoo_cfg(name):
    from ampis_amd import model_zoo
    from ampis_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_3x.yaml"))
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = SETS[name][0]
    cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS = [SETS[name][1]]
    return cfg


def test_default_predictor_honours_the_anchor_keys(tmp_path):
    """DefaultPredictor with S1 in the cfg against the oracle under S1 (on the parent commit the keys were ignored: the detections were
    those of the default anchors)."""
    from ampis_amd import checkpoint, params as P
    from ampis_amd.engine import DefaultPredictor
    from oracle import gate, maskrcnn as O
    K, H, W, D = 2, 224, 288, 60
    rng = np.random.default_rng(5)
    img = _synth_image(rng, H, W)
    npp = P.init_params(K, seed=3, style="spread")
    checkpoint.save_checkpoint(tmp_path / "w.pth", npp)
    cfg = _zoo_cfg("S1")
    cfg.MODEL.WEIGHTS, cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.TEST.DETECTIONS_PER_IMAGE = str(tmp_path / "w.pth"), K, D
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = H, W           # no resize
    pred = DefaultPredictor(cfg)
    inst = pred(img)["instances"]
    assert pred._model.num_anchors == 3 and pred._model.anchor_sizes[0] == (8.0,)
    ocfg = O.Cfg(num_classes=K, detections_per_image=D)
    with pytest.MonkeyPatch.context() as mp:
        oracle_anchors(mp, *SETS["S1"])
        ref = O.infer(img[None], O.to_torch_params(npp), ocfg)
    ref0 = O.infer(img[None], O.to_torch_params(npp), ocfg)
    assert len(ref[0]["boxes"]) != len(ref0[0]["boxes"]) or float((ref[0]["boxes"] - ref0[0]["boxes"]).abs().max()) > 1.0
    hip = dict(boxes=inst.pred_boxes.tensor.numpy(), scores=inst.scores.numpy(), classes=inst.pred_classes.numpy(), masks=inst.pred_masks.rle)
    st = gate.check_image(hip, ref[0], H, W, lambda m: _decode(m, H, W))
    assert st["instances"] > 5 and st["identical"] + st["tie_masks"] == st["instances"]
    pred.close()


def _ddicts(n, h, w, seed):
    from ampis_amd import synth
    out = []
    for i in range(n):
        img, gt = synth.micrograph(i, h, w, seed=seed)
        annos = [{"bbox": b.tolist(), "bbox_mode": 0, "segmentation": [p.tolist()], "category_id": 0}
                 for b, p in list(zip(gt["boxes"], gt["polygons"]))[:50]]
        out.append({"file_name": f"synthetic_{i}.png", "image_bgr": img, "height": h, "width": w, "image_id": i, "annotations": annos,
                    "mask_format": "polygonmask", "num_instances": len(annos)})
    return out


def test_default_trainer_with_five_anchors_checkpoints_and_resumes(tmp_path, caplog):
    """DefaultTrainer with S2: the RPN predictors in state_dict / checkpoint have A = 5 rows; resume continues bit for bit; an A = 3
    checkpoint loaded non-strict re-initialises exactly the four RPN predictor tensors, with a warning naming them; on resume it is an error."""
    import logging
    from ampis_amd import checkpoint, params as P
    from ampis_amd.data import DatasetCatalog, MetadataCatalog
    from ampis_amd.engine import DefaultTrainer
    DatasetCatalog.clear()
    train = _ddicts(4, 160, 224, 80)
    DatasetCatalog.register("particle_Train", lambda: train)
    MetadataCatalog.get("particle_Train").set(thing_classes=["particle"])
    a3 = P.init_params(1, seed=4, style="spread")                         # a checkpoint trained with the default anchors
    checkpoint.save_checkpoint(tmp_path / "a3.pth", a3)
    cfg = _zoo_cfg("S2")
    cfg.DATASETS.TRAIN, cfg.DATASETS.TEST = ("particle_Train",), ()
    cfg.SOLVER.IMS_PER_BATCH, cfg.SOLVER.MAX_ITER, cfg.SOLVER.CHECKPOINT_PERIOD = 2, 3, 3
    cfg.SOLVER.BASE_LR, cfg.SOLVER.WARMUP_ITERS = 0.002, 1
    cfg.MODEL.WEIGHTS, cfg.MODEL.ROI_HEADS.NUM_CLASSES = str(tmp_path / "a3.pth"), 1
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (0,), 1000
    cfg.OUTPUT_DIR = str(tmp_path / "out")
    rpn = "proposal_generator.rpn_head."
    four = {rpn + f"{h}.{p}" for h in ("objectness_logits", "anchor_deltas") for p in ("weight", "bias")}
    tr = DefaultTrainer(cfg)
    with caplog.at_level(logging.WARNING, logger="ampis_amd"):
        tr.resume_or_load(resume=False)
    assert {n for n, _, _ in tr.load_report["shape_mismatch"]} == four and not tr.load_report["missing"]
    warned = " ".join(r.getMessage() for r in caplog.records)
    assert all(n in warned for n in four)
    assert np.array_equal(tr.params[rpn + "conv.weight"], a3[rpn + "conv.weight"])
    assert tr.params[rpn + "objectness_logits.weight"].shape == (5, 256, 1, 1) and tr.params[rpn + "anchor_deltas.weight"].shape == (20, 256, 1, 1)
    tr.train()
    assert all(np.isfinite(v) for v, _ in tr.storage.history("total_loss"))
    sd = tr._net.state_dict()
    assert sd[rpn + "objectness_logits.weight"].shape == (5, 256, 1, 1) and sd[rpn + "anchor_deltas.bias"].shape == (20,)
    mom = tr._net.momentum_dict()
    assert mom[rpn + "anchor_deltas.weight"].shape == (20, 256, 1, 1) and np.abs(mom[rpn + "anchor_deltas.weight"]).max() > 0
    last = os.path.join(cfg.OUTPUT_DIR, open(os.path.join(cfg.OUTPUT_DIR, "last_checkpoint")).read().strip())
    stored = torch.load(last, map_location="cpu", weights_only=False)["model"]
    assert tuple(stored[rpn + "objectness_logits.weight"].shape) == (5, 256, 1, 1)
    # checkpoint -> resume: weights and momentum bit for bit
    cfg.SOLVER.MAX_ITER = 4
    tr2 = DefaultTrainer(cfg)
    tr2.resume_or_load(resume=True)
    assert tr2.start_iter == 3
    tr2._ensure_net(160, 224)
    sd2, mom2 = tr2._net.state_dict(), tr2._net.momentum_dict()
    for k in sd:
        assert np.array_equal(sd[k], sd2[k]), k
    for k in mom:
        assert np.array_equal(mom[k], mom2[k]), k
    tr2.train()
    assert [i for _, i in tr2.storage.history("total_loss")] == [3]
    # resuming that checkpoint under the default anchors: a strict load, refused
    cfg3 = _zoo_cfg("A3")
    for key in ("DATASETS", "SOLVER", "INPUT"):
        cfg3[key] = cfg[key]
    cfg3.MODEL.ROI_HEADS.NUM_CLASSES, cfg3.OUTPUT_DIR = 1, cfg.OUTPUT_DIR
    tr3 = DefaultTrainer(cfg3)
    with pytest.raises(ValueError, match="strict load failed"):
        tr3.resume_or_load(resume=True)
    tr.close(); tr2.close(); tr3.close()
    DatasetCatalog.clear()


def test_an_anchor_setting_the_native_path_cannot_hold_fails_at_construction():
    from ampis_amd.engine import DefaultPredictor, DefaultTrainer
    cfg = _zoo_cfg("S3")
    cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.33, 0.5, 1.0, 2.0]]       # 12 per location
    cfg.MODEL.WEIGHTS = ""
    with pytest.raises(ValueError, match="ANCHOR_GENERATOR"):
        DefaultPredictor(cfg)
    with pytest.raises(ValueError, match="ANCHOR_GENERATOR"):
        DefaultTrainer(cfg)
