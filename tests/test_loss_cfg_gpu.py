"""The configurable box regression losses on the device (amp_loss_opts: smooth-L1 with a quadratic zone, GIoU through apply_deltas, the loss
weights of MODEL.RPN and MODEL.ROI_BOX_HEAD): the two loss stages against a torch restatement of fvcore's smooth_l1_loss / giou_loss and
detectron2's apply_deltas, the whole training step against oracle/train.py with the two regression losses recomputed under the chosen
options, reproducibility, switching the options between steps, and the cfg reaching a trainer and a predictor.

Tolerances are those of tests/test_train_sampling_gpu.py: a loss within rel 2e-4 / abs 1e-6, a gradient within 2e-3 of the tensor's largest
entry; in the end-to-end cases a tensor whose fp32 reference gradient itself moves by more than 1e-3 under a 2^-21 relative weight jitter
(three probes) is held to 1.5 times that spread, and at most a quarter of the tensors may be such."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = 2.0 ** -21
PROBES = 3
COND = 1e-3
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------ restatements
def smooth_l1(d, beta):
    """fvcore smooth_l1_loss(reduction="sum") of the differences d."""
    if beta < 1e-5:
        return d.abs().sum()
    n = d.abs()
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum()


def giou_parts(b1, b2, eps=1e-7):
    """fvcore giou_loss without the reduction: per-box loss [N] of predicted boxes b1 against b2 (XYXY)."""
    x1, y1, x2, y2 = b1.unbind(-1)
    x1g, y1g, x2g, y2g = b2.unbind(-1)
    xk1, yk1, xk2, yk2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
    mask = (yk2 > yk1) & (xk2 > xk1)
    inter = torch.where(mask, (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    iou = inter / (union + eps)
    area_c = (torch.max(x2, x2g) - torch.min(x1, x1g)) * (torch.max(y2, y2g) - torch.min(y1, y1g))
    return 1 - (iou - (area_c - union) / (area_c + eps))


def reg_loss(kind, beta, pred_deltas, src, tgt, weights):
    """detectron2 _dense_box_regression_loss / FastRCNNOutputLayers.box_reg_loss on selected rows: sum, not normalised."""
    from oracle import maskrcnn as M, train as T
    if len(pred_deltas) == 0:
        return pred_deltas.sum() * 0
    if kind == "giou":
        return giou_parts(M.apply_deltas(pred_deltas, src, weights), tgt).sum()
    return smooth_l1(pred_deltas - T.get_deltas(src, tgt, weights), beta)


def pair_kind(pred_boxes, tgt):
    """'disjoint' | 'nested' | 'partial' per pair; also asserts there is no exact tie in the max / min a GIoU gradient selects by."""
    out = []
    for p, g in zip(pred_boxes.tolist(), tgt.tolist()):
        assert all(p[i] != g[i] for i in range(4)), "an exact tie between a predicted and a GT coordinate"
        iw, ih = min(p[2], g[2]) - max(p[0], g[0]), min(p[3], g[3]) - max(p[1], g[1])
        assert iw != 0 and ih != 0
        if iw <= 0 or ih <= 0:
            out.append("disjoint")
        elif (p[0] < g[0] and p[1] < g[1] and p[2] > g[2] and p[3] > g[3]) or (p[0] > g[0] and p[1] > g[1] and p[2] < g[2] and p[3] < g[3]):
            out.append("nested")
        else:
            out.append("partial")
    return out


def _opts(**kw):
    from ampis_amd import _lib
    return _lib.loss_opts(kw)


def _close(got, ref):
    return got == pytest.approx(ref, rel=2e-4, abs=1e-6)


def _grad_ok(got, ref, what):
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: gradient max error {err:.3e}, largest entry {top:.3e}")
    assert top > 0 and err <= 2e-3 * top, (what, err, top)


# ------------------------------------------------------------------------------------------------------------------ 1. stages
SHAPES = [(64, 80), (32, 40), (16, 20), (8, 10), (4, 5)]


class RpnStage:
    """Labels and matches of random GT boxes on a 256 x 320 frame (amp_anchor_labels), then amp_rpn_sample_loss[_ex] on predictions the
    test writes.  The sample depends on the labels and the seed only, so one call finds the positives the predictions are shaped for."""

    def __init__(self, ctx, seed=0):
        from ampis_amd import _lib, ops
        from oracle import maskrcnn as M
        self.ctx, self.B, self.batch, self.pos_max, self.seed = ctx, 2, 256, 128, 11
        rng = np.random.default_rng(seed)
        H, W = 256, 320
        per_image = []
        for n in (24, 17):
            c = rng.uniform([20, 20], [W - 20, H - 20], size=(n, 2)); s = rng.uniform(14, 150, size=(n, 2))
            per_image.append(np.concatenate([np.clip(c - s / 2, 0, None), np.minimum(c + s / 2, [W, H])], axis=1).astype(np.float32))
        self.per_image = per_image
        self.anchors = torch.cat([M.grid_anchors(h, w, M.STRIDES[l], M.ANCHOR_SIZES[l]) for l, (h, w) in enumerate(SHAPES)])
        self.A = self.anchors.shape[0]
        self.lvl_off = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in SHAPES])])
        gt_all = np.concatenate(per_image)
        self.off = np.concatenate([[0], np.cumsum([len(p) for p in per_image])]).astype(np.int32)
        self.d_gt, self.d_off = torch.from_numpy(gt_all).to(DEV), torch.from_numpy(self.off).to(DEV)
        B, A = self.B, self.A
        self.preds = [(torch.from_numpy(rng.standard_normal((B, h * w, 16)).astype(np.float32)) * 0.5) for h, w in SHAPES]
        for p in self.preds:
            p[..., 15] = 0
        self.mv = torch.empty((B, A), device=DEV); self.mi = torch.empty((B, A), dtype=torch.int32, device=DEV)
        best = torch.zeros((len(gt_all),), dtype=torch.int32, device=DEV)
        self.lab = torch.empty((B, A), dtype=torch.int8, device=DEV)
        lv = ops.make_rpn_levels([p.to(DEV) for p in self.preds], SHAPES)
        ops.check(_lib.lib().amp_anchor_labels(ctx.handle, C.byref(lv), B, ops.ptr(self.d_gt), ops.ptr(self.d_off), int(len(gt_all)), 0.3, 0.7,
                                               ops.ptr(self.mv), ops.ptr(self.mi), ops.ptr(best), ops.ptr(self.lab)), "amp_anchor_labels")
        torch.cuda.synchronize()
        self.match = self.mi.cpu().numpy()

    def run(self, opts=None, old=False):
        """-> (dpred per level (cpu), partial [B,2], sampled [B,batch], counts [B,2])"""
        from ampis_amd import _lib, ops
        B = self.B
        d_pred = [p.to(DEV).contiguous() for p in self.preds]
        lv = ops.make_rpn_levels(d_pred, SHAPES)
        dp = [torch.zeros_like(p) for p in d_pred]
        dp_arr = (C.c_void_p * 5)(*[t.data_ptr() for t in dp])
        keys = torch.empty((B, self.A), dtype=torch.int32, device=DEV)
        sampled = torch.full((B, self.batch), -1, dtype=torch.int32, device=DEV)
        counts = torch.zeros((B, 2), dtype=torch.int32, device=DEV)
        partial = torch.zeros((B, 2), device=DEV)
        args = (self.ctx.handle, C.byref(lv), dp_arr, B, ops.ptr(self.d_gt), ops.ptr(self.d_off), ops.ptr(self.lab), ops.ptr(self.mi), ops.ptr(keys),
                self.batch, self.pos_max, self.seed, ops.ptr(sampled), ops.ptr(counts), ops.ptr(partial))
        if old:
            ops.check(_lib.lib().amp_rpn_sample_loss(*args), "amp_rpn_sample_loss")
        else:
            ops.check(_lib.lib().amp_rpn_sample_loss_ex(*args, C.byref(opts)), "amp_rpn_sample_loss_ex")
        torch.cuda.synchronize()
        return [t.cpu() for t in dp], partial.cpu(), sampled.cpu().numpy(), counts.cpu().numpy()

    def split(self, a):
        """global anchor index -> (level, pixel, anchor of the pixel)"""
        l = int(np.searchsorted(self.lvl_off, a, side="right") - 1)
        local = int(a - self.lvl_off[l])
        return l, local // 3, local % 3

    def reference(self, sampled, counts, kind, beta, w_cls, w_loc):
        """-> (sum BCE, sum regression loss, d(weighted, normalised losses)/d(pred) per level, deltas / anchors / GT of the positives)"""
        import torch.nn.functional as F
        preds = [p.clone().requires_grad_(True) for p in self.preds]
        bce, loc = torch.zeros(()), torch.zeros(())
        rows = []
        for b in range(self.B):
            npos, nneg = int(counts[b, 0]), int(counts[b, 1])
            logits, deltas = [], []
            for a in sampled[b, :npos + nneg]:
                l, pix, k = self.split(int(a))
                logits.append(preds[l][b, pix, k])
                deltas.append(preds[l][b, pix, 3 + 4 * k: 7 + 4 * k])
            tgt = torch.cat([torch.ones(npos), torch.zeros(nneg)])
            bce = bce + F.binary_cross_entropy_with_logits(torch.stack(logits), tgt, reduction="sum")
            pos = sampled[b, :npos].astype(np.int64)
            src = self.anchors[pos]
            gtb = torch.from_numpy(self.per_image[b])[self.match[b, pos].astype(np.int64)]
            pd = torch.stack(deltas[:npos])
            loc = loc + reg_loss(kind, beta, pd, src, gtb, (1.0, 1.0, 1.0, 1.0))
            rows.append((pd.detach(), src, gtb))
        norm = float(self.batch * self.B)
        (w_cls * bce / norm + w_cls * w_loc * loc / norm).backward()
        return float(bce.detach()), float(loc.detach()), [p.grad for p in preds], rows


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9, 1000.0])
def test_rpn_stage_smooth_l1(gpu_ctx, beta):
    st = RpnStage(gpu_ctx)
    w_cls, w_loc = 0.5, 2.0
    dp, partial, sampled, counts = st.run(_opts(rpn_smooth_l1_beta=beta, rpn_loss_weight=w_cls, rpn_bbox_reg_loss_weight=w_loc))
    assert counts[:, 0].min() > 8 and (counts.sum(axis=1) == st.batch).all()
    bce, loc, ref, rows = st.reference(sampled, counts, "smooth_l1", beta, w_cls, w_loc)
    from oracle import train as T
    d = torch.cat([pd - T.get_deltas(src, gtb, (1.0, 1.0, 1.0, 1.0)) for pd, src, gtb in rows]).abs()
    quad = int((d < beta).sum())
    print(f"rpn beta {beta}: {quad} of {d.numel()} elements quadratic; sums {float(partial[:, 0].sum())} / {bce}, {float(partial[:, 1].sum())} / {loc}")
    assert quad == (0 if beta == 0 else d.numel() if beta == 1000.0 else quad) and (beta != 1.0 / 9 or 0 < quad < d.numel())
    assert _close(float(partial[:, 0].sum()), bce) and _close(float(partial[:, 1].sum()), loc)
    got, want = torch.cat([t.reshape(-1, 16) for t in dp]), torch.cat([t.reshape(-1, 16) for t in ref])
    _grad_ok(got[:, :3], want[:, :3], f"rpn logits, beta {beta}")
    _grad_ok(got[:, 3:15], want[:, 3:15], f"rpn deltas, beta {beta}")
    assert not got[:, 15].any()


def test_rpn_stage_giou(gpu_ctx):
    st = RpnStage(gpu_ctx)
    _, _, sampled, counts = st.run(_opts())
    # shape the deltas of the positives: near the target, far away, shrunk, grown, and beyond the clamp in w, in h, in both
    clamped = {}
    for b in range(st.B):
        for i, a in enumerate(sampled[b, :counts[b, 0]]):
            l, pix, k = st.split(int(a))
            row = st.preds[l][b, pix, 3 + 4 * k: 7 + 4 * k]
            mode = i % 7
            if mode == 1:
                row[0] += 5.0
            elif mode == 2:
                row[2:] -= 2.0
            elif mode == 3:
                row[2:] += 2.0
            elif mode >= 4:
                which = {4: (2,), 5: (3,), 6: (2, 3)}[mode]
                for q in which:
                    row[q] = 4.5 + 0.25 * q
                clamped[(b, l, pix, k)] = which
    w_cls, w_loc = 1.0, 2.0
    dp, partial, sampled2, counts2 = st.run(_opts(rpn_loss_type="giou", rpn_bbox_reg_loss_weight=w_loc, rpn_smooth_l1_beta=0.3))
    assert np.array_equal(sampled, sampled2) and np.array_equal(counts, counts2)
    bce, loc, ref, rows = st.reference(sampled, counts, "giou", 0.0, w_cls, w_loc)
    from oracle import maskrcnn as M
    kinds = sum((pair_kind(M.apply_deltas(pd, src, (1.0, 1.0, 1.0, 1.0)), gtb) for pd, src, gtb in rows), [])
    print("rpn giou pairs:", {k: kinds.count(k) for k in set(kinds)}, "clamped rows:", len(clamped), "sums", float(partial[:, 1].sum()), loc)
    assert all(kinds.count(k) >= 5 for k in ("disjoint", "nested", "partial")) and len(clamped) >= 9
    assert max(float(pd[:, 2:].max()) for pd, _, _ in rows) > M.SCALE_CLAMP
    assert _close(float(partial[:, 0].sum()), bce) and _close(float(partial[:, 1].sum()), loc)
    got, want = torch.cat([t.reshape(-1, 16) for t in dp]), torch.cat([t.reshape(-1, 16) for t in ref])
    _grad_ok(got[:, :3], want[:, :3], "rpn logits, giou")
    _grad_ok(got[:, 3:15], want[:, 3:15], "rpn deltas, giou")
    for (b, l, pix, k), which in clamped.items():
        for q in range(2, 4):
            g, r = float(dp[l][b, pix, 3 + 4 * k + q]), float(ref[l][b, pix, 3 + 4 * k + q])
            assert (g == 0.0 and r == 0.0) if q in which else (g != 0.0 and r != 0.0), (b, l, pix, k, q, g, r)


def test_rpn_stage_defaults_are_the_old_entry_point_bit_for_bit(gpu_ctx):
    st = RpnStage(gpu_ctx)
    dp0, part0, s0, c0 = st.run(old=True)
    dp1, part1, s1, c1 = st.run(_opts())
    assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and c0[:, 0].min() > 0
    assert np.array_equal(part0.numpy().view(np.uint32), part1.numpy().view(np.uint32))
    for a, b in zip(dp0, dp1):
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))
    assert sum(int((t != 0).sum()) for t in dp0) >= int(c0.sum())
    # ... and that is the plain L1 loss: sign gradients of size 1 / (batch * B) on the deltas of the positives
    vals = torch.cat([t[..., 3:15].reshape(-1) for t in dp0])
    assert set(np.unique(vals.numpy()).tolist()) == {-1.0 / 512, 0.0, 1.0 / 512}


class BoxStage:
    """RoIs, classes and matched GT written by hand for amp_box_loss[_ex]: every third foreground pair disjoint, every third nested, the rest
    partly overlapping; background and unused rows in between."""

    def __init__(self, ctx, seed=1, weights=(10.0, 10.0, 5.0, 5.0)):
        self.ctx, self.B, self.batch, self.K, self.ld, self.weights = ctx, 2, 96, 3, 16, weights
        rng = np.random.default_rng(seed)
        B, n = self.B, self.batch
        c = rng.uniform([40, 40], [600, 400], size=(B, n, 2)); s = rng.uniform(12, 160, size=(B, n, 2))
        self.rois = np.concatenate([c - s / 2, c + s / 2], axis=2).astype(np.float32)
        self.cls = np.full((B, n), -1, np.int32)
        self.gti = np.zeros((B, n), np.int32)
        gts = []
        for b in range(B):
            used = n - 7 * (b + 1)
            g = []
            for r in range(used):
                if r % 4 == 3:
                    self.cls[b, r] = self.K
                    continue
                self.cls[b, r] = r % self.K
                x1, y1, x2, y2 = self.rois[b, r].astype(np.float64)
                w, h = x2 - x1, y2 - y1
                j = rng.uniform(0.03, 0.2, 4)
                mode = (r // 4) % 3
                if mode == 0:
                    box = [x1 + j[0] * w, y1 - j[1] * h, x2 + j[2] * w, y2 - j[3] * h]
                elif mode == 1:
                    box = [x2 + (1 + j[0]) * w, y1 + j[1] * h, x2 + (2 + j[2]) * w, y2 + (1 + j[3]) * h]
                else:
                    box = [x1 + j[0] * w, y1 + j[1] * h, x2 - j[2] * w, y2 - j[3] * h]
                self.gti[b, r] = len(g)
                g.append(box)
            gts.append(np.asarray(g, np.float32))
        self.gts = gts
        self.off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
        self.pred = (rng.standard_normal((B * n, self.ld)) * 0.6).astype(np.float32)
        self.total = int((self.cls >= 0).sum())

    def run(self, opts=None, old=False):
        from ampis_amd import _lib, ops
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        pred, rois, cls, gti, gt, off = t(self.pred), t(self.rois), t(self.cls), t(self.gti), t(np.concatenate(self.gts)), t(self.off)
        dp = torch.full_like(pred, 7.0)
        partial = torch.zeros((self.B, 2), device=DEV)
        w = (C.c_float * 4)(*self.weights)
        args = (self.ctx.handle, self.B, self.batch, self.K, ops.ptr(pred), self.ld, ops.ptr(dp), ops.ptr(rois), ops.ptr(cls), ops.ptr(gti), ops.ptr(gt),
                ops.ptr(off), w, self.total, ops.ptr(partial))
        if old:
            ops.check(_lib.lib().amp_box_loss(*args), "amp_box_loss")
        else:
            ops.check(_lib.lib().amp_box_loss_ex(*args, C.byref(opts)), "amp_box_loss_ex")
        torch.cuda.synchronize()
        return dp.cpu(), partial.cpu()

    def reference(self, kind, beta, w_reg):
        import torch.nn.functional as F
        K = self.K
        pred = torch.from_numpy(self.pred).clone().requires_grad_(True)
        cls = torch.from_numpy(self.cls.reshape(-1).astype(np.int64))
        used = torch.nonzero(cls >= 0).squeeze(1)
        ce = F.cross_entropy(pred[used, :K + 1], cls[used], reduction="sum")
        fg = torch.nonzero((cls >= 0) & (cls < K)).squeeze(1)
        src = torch.from_numpy(self.rois.reshape(-1, 4))[fg]
        b_of = fg // self.batch
        gt_all = torch.from_numpy(np.concatenate(self.gts))
        tgt = gt_all[torch.from_numpy(self.off.astype(np.int64))[b_of] + torch.from_numpy(self.gti.reshape(-1).astype(np.int64))[fg]]
        pd = pred[:, K + 1:K + 1 + 4 * K].reshape(-1, K, 4)[fg, cls[fg]]
        loc = reg_loss(kind, beta, pd, src, tgt, self.weights)
        (ce / self.total + w_reg * loc / self.total).backward()
        return float(ce.detach()), float(loc.detach()), pred.grad, (pd.detach(), src, tgt, fg, cls[fg])


@pytest.mark.parametrize("beta", [0.0, 0.5, 1000.0])
def test_box_stage_smooth_l1(gpu_ctx, beta):
    st = BoxStage(gpu_ctx)
    w_reg = 3.0
    dp, partial = st.run(_opts(box_smooth_l1_beta=beta, box_bbox_reg_loss_weight=w_reg, rpn_loss_weight=0.25))
    ce, loc, ref, (pd, src, tgt, _, _) = st.reference("smooth_l1", beta, w_reg)
    from oracle import train as T
    d = (pd - T.get_deltas(src, tgt, st.weights)).abs()
    quad = int((d < beta).sum())
    print(f"box beta {beta}: {quad} of {d.numel()} elements quadratic; sums {float(partial[:, 0].sum())} / {ce}, {float(partial[:, 1].sum())} / {loc}")
    assert quad == (0 if beta == 0 else d.numel() if beta == 1000.0 else quad) and (beta != 0.5 or 0 < quad < d.numel())
    assert _close(float(partial[:, 0].sum()), ce) and _close(float(partial[:, 1].sum()), loc)
    K = st.K
    _grad_ok(dp[:, :K + 1], ref[:, :K + 1], f"box logits, beta {beta}")
    _grad_ok(dp[:, K + 1:], ref[:, K + 1:], f"box deltas, beta {beta}")


def test_box_stage_giou(gpu_ctx):
    from oracle import maskrcnn as M
    st = BoxStage(gpu_ctx)
    K = st.K
    cls = st.cls.reshape(-1)
    clamped = {}
    for i, r in enumerate(np.nonzero((cls >= 0) & (cls < K))[0]):
        col = K + 1 + 4 * cls[r]
        st.pred[r, col:col + 2] *= 4.0                 # weights 10, 10: shifts of a fraction of the box
        st.pred[r, col + 2:col + 4] *= 3.0
        if i % 5 == 4:
            which = {0: (2,), 1: (3,), 2: (2, 3)}[(i // 5) % 3]
            for q in which:
                st.pred[r, col + q] = 5.0 * (4.3 + 0.1 * q)      # / ww = 5 -> 4.5 or 4.6 > log(1000 / 16)
            clamped[int(r)] = which
    w_reg = 10.0
    dp, partial = st.run(_opts(box_loss_type="giou", box_bbox_reg_loss_weight=w_reg, box_smooth_l1_beta=0.7))
    ce, loc, ref, (pd, src, tgt, fg, fcls) = st.reference("giou", 0.0, w_reg)
    kinds = pair_kind(M.apply_deltas(pd, src, st.weights), tgt)
    print("box giou pairs:", {k: kinds.count(k) for k in set(kinds)}, "clamped rows:", len(clamped), "sums", float(partial[:, 1].sum()), loc)
    assert all(kinds.count(k) >= 5 for k in ("disjoint", "nested", "partial")) and len(clamped) >= 9
    assert _close(float(partial[:, 0].sum()), ce) and _close(float(partial[:, 1].sum()), loc)
    _grad_ok(dp[:, :K + 1], ref[:, :K + 1], "box logits, giou")
    _grad_ok(dp[:, K + 1:], ref[:, K + 1:], "box deltas, giou")
    for r, which in clamped.items():
        col = K + 1 + 4 * cls[r]
        assert float(st.pred[r, col + which[0]]) / st.weights[which[0]] > M.SCALE_CLAMP
        for q in range(2, 4):
            g, w = float(dp[r, col + q]), float(ref[r, col + q])
            assert (g == 0.0 and w == 0.0) if q in which else (g != 0.0 and w != 0.0), (r, q, g, w)
    # rows that are not sampled and columns of other classes get exactly 0
    assert not dp[torch.from_numpy(cls < 0)].any()
    other = torch.ones_like(dp, dtype=torch.bool)
    other[:, :K + 1] = False
    for r, c in zip(fg.tolist(), fcls.tolist()):
        other[r, K + 1 + 4 * c:K + 5 + 4 * c] = False
    assert not dp[other].any()


def test_box_stage_defaults_are_the_old_entry_point_bit_for_bit(gpu_ctx):
    st = BoxStage(gpu_ctx)
    dp0, part0 = st.run(old=True)
    dp1, part1 = st.run(_opts())
    assert np.array_equal(part0.numpy().view(np.uint32), part1.numpy().view(np.uint32)) and float(part0[:, 1].min()) > 0
    assert np.array_equal(dp0.numpy().view(np.uint32), dp1.numpy().view(np.uint32))
    vals = dp0[:, st.K + 1:].reshape(-1).numpy()
    inv = np.float32(1.0) / np.float32(st.total)
    assert set(np.unique(vals).tolist()) == {float(-inv), 0.0, float(inv)}


# ------------------------------------------------------------------------------------------------------------------ 2. the training step
# images, classes, frame, synth seed, GT per image, sampling seed (the cases "tutorial" and "thresholds"' inputs of tests/test_train_sampling_gpu.py,
# default sampling); loss = the options under test
SMALL = dict(B=1, K=1, H=256, W=320, seed=21, ngt=60, sseed=4)
THREE = dict(B=2, K=3, H=224, W=288, seed=25, ngt=50, sseed=8)
GIOU_W = dict(rpn_loss_type="giou", box_loss_type="giou", rpn_bbox_reg_loss_weight=2.0, box_bbox_reg_loss_weight=10.0)
CASES = {
    "default":      dict(SMALL, loss={}),
    "betas":        dict(SMALL, loss=dict(rpn_smooth_l1_beta=1.0 / 9, box_smooth_l1_beta=1.0)),
    "giou":         dict(SMALL, loss=GIOU_W),
    "giou_3class":  dict(THREE, loss=GIOU_W),
    "weights_beta": dict(THREE, loss=dict(rpn_loss_weight=0.5, rpn_bbox_reg_loss_weight=2.0, box_smooth_l1_beta=0.5, box_bbox_reg_loss_weight=3.0)),
}
LOSS_DEFAULTS = dict(rpn_loss_type="smooth_l1", rpn_smooth_l1_beta=0.0, rpn_loss_weight=1.0, rpn_bbox_reg_loss_weight=1.0, box_loss_type="smooth_l1",
                     box_smooth_l1_beta=0.0, box_bbox_reg_loss_weight=1.0)


def _gts(case):
    from ampis_amd import synth
    imgs, gts = synth.batch(case["B"], case["H"], case["W"], seed=case["seed"])
    out = []
    for g in gts:
        n = case["ngt"]
        cls = np.asarray(g["classes"][:n], np.int64)
        cls = np.zeros_like(cls) if case["K"] == 1 else (np.arange(len(cls)) % case["K"]).astype(np.int64)
        out.append(dict(boxes=np.asarray(g["boxes"][:n], np.float32).reshape(-1, 4), classes=cls, polygons=list(g["polygons"][:n])))
    return imgs, out


def _jitter(npp, seed):
    rng = np.random.default_rng(seed)
    return {k: (v * (1 + rng.standard_normal(np.shape(v)).astype(np.float32) * np.float32(JITTER))).astype(np.float32) if ".norm." not in k else v
            for k, v in npp.items()}


def _trainable(tp):
    return [k for k in tp if ".norm." not in k and not k.startswith("backbone.bottom_up.stem") and not k.startswith("backbone.bottom_up.res2")]


def reference_step(imgs, gts, npp, cfg, loss, info=None):
    """oracle.train.forward_losses with loss_rpn_loc and loss_box_reg recomputed from its stages under `loss` (the fields of amp_loss_opts),
    the weights applied as detectron2 does; autograd of the sum over the trainable tensors.  -> (losses, gradients, names)"""
    from oracle import maskrcnn as M, train as T
    o = dict(LOSS_DEFAULTS, **loss)
    tp = M.to_torch_params(npp)
    names = _trainable(tp)
    for k in names:
        tp[k].requires_grad_(True)
    st = {}
    ref = T.forward_losses(imgs, gts, tp, cfg, stages=st)
    B, K = len(gts), cfg.num_classes
    deltas = torch.cat([d for _, d in st["rpn_outs"]], dim=1)                      # [B, A, 4]
    loc = deltas.new_zeros(())
    rpn_d = []
    for b in range(B):
        pos, _, matches = st["rpn_samples"][b]
        if len(pos):
            gtb = torch.as_tensor(gts[b]["boxes"], dtype=torch.float32).reshape(-1, 4)
            src, tgt = st["anchors"][pos], gtb[matches[pos]]
            loc = loc + reg_loss(o["rpn_loss_type"], o["rpn_smooth_l1_beta"], deltas[b][pos], src, tgt, (1.0, 1.0, 1.0, 1.0))
            rpn_d.append((deltas[b][pos].detach(), src, tgt))
    norm = float(cfg.rpn_batch * B)
    gcls = torch.cat(st["roi_cls"])
    fg = torch.nonzero((gcls >= 0) & (gcls < K)).squeeze(1)
    pboxes = torch.cat(st["rois"])
    gboxes = torch.cat([torch.as_tensor(gts[b]["boxes"], dtype=torch.float32).reshape(-1, 4)[st["roi_gtidx"][b]] if len(gts[b]["boxes"]) else st["rois"][b]
                        for b in range(B)])
    fg_pred = st["box_deltas"].view(-1, K, 4)[fg, gcls[fg]]
    box = reg_loss(o["box_loss_type"], o["box_smooth_l1_beta"], fg_pred, pboxes[fg], gboxes[fg], cfg.bbox_reg_weights) / max(gcls.numel(), 1.0)
    if not loss:       # the restatement with the default options is the oracle's own loss
        assert float((loc / norm).detach()) == pytest.approx(float(ref["loss_rpn_loc"].detach()), rel=1e-6)
        assert float(box.detach()) == pytest.approx(float(ref["loss_box_reg"].detach()), rel=1e-6)
    out = dict(loss_cls=ref["loss_cls"], loss_mask=ref["loss_mask"], loss_rpn_cls=ref["loss_rpn_cls"] * o["rpn_loss_weight"],
               loss_rpn_loc=loc / norm * (o["rpn_loss_weight"] * o["rpn_bbox_reg_loss_weight"]), loss_box_reg=box * o["box_bbox_reg_loss_weight"])
    sum(out.values()).backward()
    grads = {k: tp[k].grad.detach().numpy() if tp[k].grad is not None else np.zeros(tp[k].shape, np.float32) for k in names}
    if info is not None:
        info.update(rpn=rpn_d, box=(fg_pred.detach(), pboxes[fg], gboxes[fg]), plain={k: float(v.detach()) for k, v in ref.items()})
    return {k: float(v.detach()) for k, v in out.items()}, grads, names


def _rel_errors(got, ref):
    out = []
    for name, r in ref.items():
        g = got(name) if callable(got) else got[name]
        assert g.shape == r.shape, name
        out.append((float(np.abs(g - r).max()) / max(float(np.abs(r).max()), 1e-8), name))
    return sorted(out, reverse=True)


def coverage(info, loss, weights):
    """Which branch each regression element / pair of the reference step took: (rpn quadratic, rpn elements, box quadratic, box elements,
    clamped deltas, pair kinds)"""
    from oracle import maskrcnn as M, train as T
    o = dict(LOSS_DEFAULTS, **loss)
    rd = torch.cat([pd - T.get_deltas(s, t, (1.0, 1.0, 1.0, 1.0)) for pd, s, t in info["rpn"]]).abs()
    pd, s, t = info["box"]
    bd = (pd - T.get_deltas(s, t, weights)).abs()
    clamp = sum(int((p[:, 2:] > M.SCALE_CLAMP).sum()) for p, _, _ in info["rpn"]) + int((pd[:, 2:] / torch.tensor(weights[2:]) > M.SCALE_CLAMP).sum())
    return int((rd < o["rpn_smooth_l1_beta"]).sum()), rd.numel(), int((bd < o["box_smooth_l1_beta"]).sum()), bd.numel(), clamp


@pytest.mark.parametrize("name", list(CASES))
def test_training_step_matches_the_reference_under_the_options(gpu_ctx, name):
    from ampis_amd import params as P
    from ampis_amd.model import MaskRCNN
    from oracle import train as T
    case = CASES[name]
    B, K, H, W, loss = case["B"], case["K"], case["H"], case["W"], case["loss"]
    imgs, gts = _gts(case)
    npp = P.init_params(K, seed=case["seed"], style="spread")
    cfg = T.TrainCfg(num_classes=K, seed=case["sseed"])
    info = {}
    ref, ref_grads, names = reference_step(imgs, gts, npp, cfg, loss, info)
    spread = dict.fromkeys(names, 0.0)
    for p_ in range(PROBES):
        for e, n_ in _rel_errors(reference_step(imgs, gts, _jitter(npp, p_), cfg, loss)[1], ref_grads):
            spread[n_] = max(spread[n_], e)
    bound = {n_: 2e-3 if spread[n_] <= COND else 1.5 * spread[n_] for n_ in names}
    ill = sorted(((round(spread[n_], 5), n_) for n_ in names if spread[n_] > COND), reverse=True)
    print(f"{name}: {len(ill)} of {len(names)} gradients ill-conditioned in the fp32 reference: {ill}")
    assert len(ill) <= len(names) // 4, f"{name}: the reference is ill-conditioned on too many tensors: {ill}"
    rq, rn, bq, bn, clamp = coverage(info, loss, cfg.bbox_reg_weights)
    print(f"{name}: rpn {rq} of {rn} elements quadratic, box {bq} of {bn}; {clamp} clamped deltas")
    model = MaskRCNN(gpu_ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), train=True, max_gt=2048, max_poly_doubles=2048 * 64, loss=loss)
    try:
        model.load_params(npp)
        assert model.loss_opts() == {k: (float(np.float32(v)) if not isinstance(v, str) else v) for k, v in dict(LOSS_DEFAULTS, **loss).items()}
        got = model.forward_losses(imgs, gts, seed=case["sseed"], backward=True)
        for k, v in ref.items():
            print(f"{name}: {k} {got[k]} reference {v}")
        for k, v in ref.items():
            assert got[k] == pytest.approx(v, rel=2e-4, abs=1e-6), (name, k, got[k], v)
        errs = _rel_errors(lambda n_: model.get_tensor(n_, grad=True), ref_grads)
        print(f"{name}: worst gradients {errs[:4]}")
        assert len(errs) == len(names)
        bad = [(e, n, bound[n]) for e, n in errs if e > bound[n]]
        assert not bad, f"{name}: {len(bad)} gradients off: {bad[:8]}"
        # forward only: the same weighted losses
        fwd = model.forward_losses(imgs, gts, seed=case["sseed"], backward=False)
        assert fwd == got, (fwd, got)
        # ---- the setting under test was in force ----
        plain = info["plain"]
        if name == "default":
            assert got == pytest.approx(plain, rel=2e-4, abs=1e-6)
        if name == "betas":
            assert 0 < rq < rn and 0 < bq < bn, "both branches live in both heads"
            assert got["loss_rpn_loc"] < plain["loss_rpn_loc"] * 0.999 and got["loss_box_reg"] < plain["loss_box_reg"] * 0.999
        if name in ("giou", "giou_3class"):
            assert clamp == 0
            for k in ("loss_rpn_loc", "loss_box_reg"):
                assert got[k] != pytest.approx(plain[k], rel=1e-2), k
            assert got["loss_rpn_cls"] == pytest.approx(plain["loss_rpn_cls"], rel=2e-4)
        if name == "weights_beta":
            assert 0 < bq < bn and rq == 0
            assert got["loss_rpn_cls"] == pytest.approx(0.5 * plain["loss_rpn_cls"], rel=2e-4)
            assert got["loss_rpn_loc"] == pytest.approx(0.5 * 2.0 * plain["loss_rpn_loc"], rel=2e-4)      # beta 0 on the RPN: L1 times the weights
            assert got["loss_box_reg"] < 3.0 * plain["loss_box_reg"] * 0.999
        for k in ("loss_cls", "loss_mask"):
            assert got[k] == pytest.approx(plain[k], rel=2e-4, abs=1e-6), k
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------------------------ 3. reproducibility, switching
def test_giou_steps_are_bitwise_reproducible_and_options_switch_between_steps(gpu_ctx):
    from ampis_amd import params as P
    from ampis_amd.model import MaskRCNN
    case = dict(B=2, K=2, H=192, W=256, seed=27, ngt=40, sseed=3)
    imgs, gts = _gts(case)
    npp = P.init_params(case["K"], seed=5, style="spread")
    model = MaskRCNN(gpu_ctx, case["K"], max_batch=2, max_h=192, max_w=256, max_out_hw=256, train=True, max_gt=2048, max_poly_doubles=2048 * 64)
    try:
        model.load_params(npp)
        names = model.trainable_names()
        step = lambda: (model.forward_losses(imgs, gts, seed=3, backward=True), {k: model.get_tensor(k, grad=True) for k in names})
        l0, g0 = step()                                     # a new model holds the defaults
        assert model.loss_opts() == LOSS_DEFAULTS
        model.set_loss_opts(GIOU_W)
        l1, g1 = step()
        l2, g2 = step()
        assert l1 == l2
        for k in names:
            assert np.array_equal(g1[k].view(np.uint32), g2[k].view(np.uint32)), k
        assert model.forward_losses(imgs, gts, seed=3, backward=False) == l1
        # the switch took effect without re-creating the model: the regression losses and the gradients changed, the other losses did not
        for k in ("loss_cls", "loss_mask", "loss_rpn_cls"):
            assert l1[k] == l0[k], k
        assert l1["loss_rpn_loc"] != l0["loss_rpn_loc"] and l1["loss_box_reg"] != l0["loss_box_reg"]
        assert any(not np.array_equal(g0[k], g1[k]) for k in names if k.startswith("proposal_generator.rpn_head.anchor_deltas"))
        # weights alone scale the plain losses by exactly their factor (powers of two: the same bits, shifted)
        model.set_loss_opts(rpn_loss_weight=0.5, rpn_bbox_reg_loss_weight=4.0, box_bbox_reg_loss_weight=2.0)
        l3, _ = step()
        assert l3["loss_rpn_cls"] == 0.5 * l0["loss_rpn_cls"] and l3["loss_rpn_loc"] == 2.0 * l0["loss_rpn_loc"] and l3["loss_box_reg"] == 2.0 * l0["loss_box_reg"]
        # back to the defaults: the first step again, bit for bit
        model.set_loss_opts()
        l4, g4 = step()
        assert l4 == l0
        for k in names:
            assert np.array_equal(g0[k].view(np.uint32), g4[k].view(np.uint32)), k
        # a refusal names the field and leaves the options as they were
        from ampis_amd import _lib
        bad = _lib.loss_opts({})
        bad.box_smooth_l1_beta = float("nan")
        assert _lib.lib().amp_model_set_loss_opts(model._h, C.byref(bad)) == -1
        assert "amp_loss_opts.box_smooth_l1_beta" in _lib.lib().amp_last_error().decode()
        assert model.loss_opts() == LOSS_DEFAULTS
    finally:
        model.close()
    # an inference model has no training losses to configure
    with pytest.raises(ValueError, match="train=True"):
        MaskRCNN(gpu_ctx, 1, max_h=64, max_w=64, loss=GIOU_W)


# ------------------------------------------------------------------------------------------------------------------ 4. trainer, predictor
def _zoo_cfg():
    from ampis_amd import model_zoo
    from ampis_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_3x.yaml"))
    return cfg


def test_trainer_cfg_loss_keys_reach_the_net(tmp_path):
    """DefaultTrainer from a cfg with giou on both heads, non-default weights and box weights: the net holds them, three iterations give
    finite losses that carry the weights."""
    from ampis_amd import synth
    from ampis_amd.data import DatasetCatalog, MetadataCatalog
    from ampis_amd.engine import DefaultTrainer
    ddicts = []
    for i in range(2):
        img, gt = synth.micrograph(i, 192, 256, seed=51)
        annos = [{"bbox": b.tolist(), "bbox_mode": 0, "segmentation": [p.tolist()], "category_id": 0} for b, p in list(zip(gt["boxes"], gt["polygons"]))[:50]]
        ddicts.append({"file_name": f"synthetic_{i}.png", "image_bgr": img, "height": 192, "width": 256, "image_id": i, "annotations": annos,
                       "mask_format": "polygonmask", "num_instances": len(annos)})
    DatasetCatalog.register("losscfg_Train", lambda: ddicts)
    MetadataCatalog.get("losscfg_Train").set(thing_classes=["particle"])
    try:
        cfg = _zoo_cfg()
        cfg.DATASETS.TRAIN, cfg.DATASETS.TEST = ("losscfg_Train",), ()
        cfg.MODEL.ROI_HEADS.NUM_CLASSES = 1
        r, h = cfg.MODEL.RPN, cfg.MODEL.ROI_BOX_HEAD
        r.BBOX_REG_LOSS_TYPE, r.LOSS_WEIGHT, r.BBOX_REG_LOSS_WEIGHT, r.SMOOTH_L1_BETA = "giou", 0.5, 2.0, 0.25
        h.BBOX_REG_LOSS_TYPE, h.BBOX_REG_LOSS_WEIGHT, h.SMOOTH_L1_BETA, h.BBOX_REG_WEIGHTS = "giou", 10.0, 0.75, [5.0, 5.0, 2.5, 2.5]
        cfg.SOLVER.IMS_PER_BATCH, cfg.SOLVER.MAX_ITER, cfg.SOLVER.CHECKPOINT_PERIOD = 1, 3, 100
        cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (192,), 256
        cfg.MODEL.WEIGHTS = ""
        cfg.OUTPUT_DIR = str(tmp_path / "out")
        trainer = DefaultTrainer(cfg)
        trainer.resume_or_load(resume=False)
        trainer.train()
        net = trainer.model.net
        assert net.loss_opts() == dict(rpn_loss_type="giou", rpn_smooth_l1_beta=0.25, rpn_loss_weight=0.5, rpn_bbox_reg_loss_weight=2.0,
                                       box_loss_type="giou", box_smooth_l1_beta=0.75, box_bbox_reg_loss_weight=10.0)
        assert list(net.cfg.bbox_reg_weights) == [5.0, 5.0, 2.5, 2.5]
        assert trainer.iter == 3
        for k in net.LOSS_NAMES:
            hist = [v for v, _ in trainer.storage.history(k)]
            print(f"trainer {k} over three iterations: {hist}")
            assert len(hist) == 3 and all(np.isfinite(v) for v in hist), (k, hist)
        # a GIoU loss lies in [0, 2] per box: at most 128 of 256 sampled anchors positive, every sampled RoI at most foreground
        assert all(0 < v <= 2.0 * 0.5 * 2.0 * 0.5 for v, _ in trainer.storage.history("loss_rpn_loc"))
        assert all(0 < v <= 2.0 * 10.0 for v, _ in trainer.storage.history("loss_box_reg"))
        # a refused key fails in the constructor, before the loader or the device is touched
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = "ciou"
        with pytest.raises(ValueError, match="MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE"):
            DefaultTrainer(cfg)
        trainer.close()
    finally:
        DatasetCatalog.remove("losscfg_Train")
        MetadataCatalog.remove("losscfg_Train")


BOX_W = (5.0, 5.0, 2.5, 2.5)


def _synth_image(rng, h, w):
    img = rng.normal(60, 12, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(6, 40)
        d = (yy - cy) ** 2 + (xx - cx) ** 2
        img = np.where(d < r * r, rng.normal(190, 15) - 40 * d / (r * r), img)
    img = np.clip(img + rng.normal(0, 4, (h, w)), 0, 255).astype(np.uint8)
    return np.repeat(img[:, :, None], 3, axis=2)


def test_default_predictor_honours_the_box_weights(tmp_path):
    """DefaultPredictor with MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS = (5, 5, 2.5, 2.5) against the oracle with cfg.bbox_reg_weights set to the
    same, through oracle/gate.py (on the parent commit the key was ignored: the detections were decoded with (10, 10, 5, 5))."""
    from ampis_amd import checkpoint, params as P, rle
    from ampis_amd.engine import DefaultPredictor
    from oracle import gate, maskrcnn as O
    K, H, W, D = 2, 224, 288, 60
    img = _synth_image(np.random.default_rng(5), H, W)
    npp = P.init_params(K, seed=3, style="spread")
    checkpoint.save_checkpoint(tmp_path / "w.pth", npp)
    cfg = _zoo_cfg()
    cfg.MODEL.WEIGHTS, cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.TEST.DETECTIONS_PER_IMAGE = str(tmp_path / "w.pth"), K, D
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = H, W           # no resize
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS = list(BOX_W)
    pred = DefaultPredictor(cfg)
    try:
        inst = pred(img)["instances"]
        assert list(pred._model.cfg.bbox_reg_weights) == list(BOX_W)
        ref = O.infer(img[None], O.to_torch_params(npp), O.Cfg(num_classes=K, detections_per_image=D, bbox_reg_weights=BOX_W))
        ref0 = O.infer(img[None], O.to_torch_params(npp), O.Cfg(num_classes=K, detections_per_image=D))
        assert len(ref[0]["boxes"]) != len(ref0[0]["boxes"]) or float((ref[0]["boxes"] - ref0[0]["boxes"]).abs().max()) > 1.0, "the weights matter here"
        hip = dict(boxes=inst.pred_boxes.tensor.numpy(), scores=inst.scores.numpy(), classes=inst.pred_classes.numpy(), masks=inst.pred_masks.rle)
        st = gate.check_image(hip, ref[0], H, W, lambda m: rle.decode({"size": [H, W], "counts": m["counts"]}).astype(bool))
        print("predictor gate:", gate.summary(gate.merge([st])))
        assert st["instances"] > 5 and st["identical"] + st["tie_masks"] == st["instances"]
    finally:
        pred.close()


def test_training_model_honours_the_box_weights(gpu_ctx):
    """A training model with bbox_reg_weights = (5, 5, 2.5, 2.5) against oracle/train.py with cfg.bbox_reg_weights the same: the losses and the
    box predictor's gradients (the tensors the weights reach first), and loss_box_reg differs from the default weights' value."""
    from ampis_amd import params as P
    from ampis_amd.model import MaskRCNN
    from oracle import maskrcnn as M, train as T
    case = dict(B=1, K=2, H=192, W=256, seed=24, ngt=40, sseed=7)
    imgs, gts = _gts(case)
    npp = P.init_params(2, seed=24, style="spread")
    cfg = T.TrainCfg(num_classes=2, seed=7, bbox_reg_weights=BOX_W)
    ref, ref_grads, names = reference_step(imgs, gts, npp, cfg, dict(box_smooth_l1_beta=0.5))
    plain = T.forward_losses(imgs, gts, M.to_torch_params(npp), T.TrainCfg(num_classes=2, seed=7))
    model = MaskRCNN(gpu_ctx, 2, max_batch=1, max_h=192, max_w=256, max_out_hw=256, train=True, max_gt=2048, max_poly_doubles=2048 * 64,
                     bbox_reg_weights=BOX_W, loss=dict(box_smooth_l1_beta=0.5))
    try:
        model.load_params(npp)
        got = model.forward_losses(imgs, gts, seed=7, backward=True)
        for k, v in ref.items():
            print(f"box weights: {k} {got[k]} reference {v}")
            assert got[k] == pytest.approx(v, rel=2e-4, abs=1e-6), (k, got[k], v)
        assert abs(float(plain["loss_box_reg"]) - got["loss_box_reg"]) > 0.05 * got["loss_box_reg"]
        for k in ("roi_heads.box_predictor.bbox_pred.weight", "roi_heads.box_predictor.bbox_pred.bias", "roi_heads.box_predictor.cls_score.weight"):
            g, r = model.get_tensor(k, grad=True), ref_grads[k]
            e = float(np.abs(g - r).max()) / float(np.abs(r).max())
            print(f"box weights: {k} gradient error {e:.3e}")
            assert e <= 2e-3, (k, e)
    finally:
        model.close()
    for bad in ((10, 10, 5), (10, 10, 5, 0), (10, 10, float("nan"), 5)):
        with pytest.raises(ValueError, match="bbox_reg_weights"):
            MaskRCNN(gpu_ctx, 1, max_h=64, max_w=64, bbox_reg_weights=bad)
