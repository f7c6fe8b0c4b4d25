"""The range guard of AMP_CONV_F16X3 at the model level: a model call whose operands left the fp16 range is run again on the fp32 MFMA and
returns exactly what the same model returns on an AMP_CONV_F32 context; a call whose operands stayed in range is never switched to fp32 --
not by the call before it, and not by a range flag some op-level call left on the context.

A layer's OUTPUT is pushed past 65520 by an exact power of two (FrozenBN weight and bias, or weight and bias, times 2^k) that its only
consumers undo (their weights times 2^-k): the network computes the same function, so the fp32 context stays a meaningful reference, and
every assertion is a counter (MaskRCNN.f32_reruns) or byte equality."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

K, B, H, W, D = 2, 2, 128, 160, 40
BB, RPN, BOX, MASK = "backbone.bottom_up.", "proposal_generator.rpn_head.", "roi_heads.box_head.", "roi_heads.mask_head."
# site -> (tensors times 2^k: the layer's output scales exactly, tensors times 2^-k: its only consumers)
SITES = {
    "stem": ([BB + "stem.conv1.norm.weight", BB + "stem.conv1.norm.bias"], [BB + "res2.0.conv1.weight", BB + "res2.0.shortcut.weight"]),
    "res2_conv1": ([BB + "res2.0.conv1.norm.weight", BB + "res2.0.conv1.norm.bias"], [BB + "res2.0.conv2.weight"]),
    "res4_conv2": ([BB + "res4.0.conv2.norm.weight", BB + "res4.0.conv2.norm.bias"], [BB + "res4.0.conv3.weight"]),
    "rpn_hidden": ([RPN + "conv.weight", RPN + "conv.bias"], [RPN + "objectness_logits.weight", RPN + "anchor_deltas.weight"]),
    "box_fc1": ([BOX + "fc1.weight", BOX + "fc1.bias"], [BOX + "fc2.weight"]),
    "mask_fcn1": ([MASK + "mask_fcn1.weight", MASK + "mask_fcn1.bias"], [MASK + "mask_fcn2.weight"]),
}


def scaled(base, site, k):
    up, down = SITES[site]
    p = dict(base)
    for n in up:
        p[n] = base[n] * np.float32(2.0 ** k)
        if n.endswith(".weight") and ".norm." not in n:      # a convolution's own weights must stay split operands (amp_model_finalize: |w| < 60000)
            assert float(np.abs(p[n]).max()) < 60000.0, (n, k)
    for n in down:
        p[n] = base[n] * np.float32(2.0 ** -k)
    return p


def same_bytes(a, b):
    """boxes, scores, classes and RLE strings of two infer() results, byte for byte"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if not all(x[f].tobytes() == y[f].tobytes() and x[f].shape == y[f].shape for f in ("boxes", "scores", "classes")):
            return False
        if [m["counts"] for m in x["masks"]] != [m["counts"] for m in y["masks"]] or [m["size"] for m in x["masks"]] != [m["size"] for m in y["masks"]]:
            return False
    return True


def _bn(p, name):
    import torch
    w, b, mu, var = (torch.from_numpy(p[name + ".norm." + f]).cuda() for f in ("weight", "bias", "running_mean", "running_var"))
    sc = w / torch.sqrt(var + 1e-5)
    return sc.view(1, -1, 1, 1), (b - mu * sc).view(1, -1, 1, 1)


def site_peak(m, p, site):
    """the largest value of the layer's output in the fp32 context's last call, computed with torch from the taps of the layer's inputs
    (the model taps stage outputs, not every layer).  It only has to place 2^k within three octaves."""
    import torch
    import torch.nn.functional as F
    nchw = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().permute(0, 3, 1, 2)
    wt = lambda n: torch.from_numpy(p[n]).cuda()
    if site == "stem":
        return float(m.tap("stem_pool").max())
    if site == "res2_conv1":
        sc, sh = _bn(p, BB + "res2.0.conv1")
        return float((F.conv2d(nchw(m.tap("stem_pool")), wt(BB + "res2.0.conv1.weight")) * sc + sh).max())
    if site == "res4_conv2":
        s1, h1 = _bn(p, BB + "res4.0.conv1")
        s2, h2 = _bn(p, BB + "res4.0.conv2")
        t = torch.relu(F.conv2d(nchw(m.tap("res3")), wt(BB + "res4.0.conv1.weight"), stride=2) * s1 + h1)      # R50: the block's stride is in its 1x1
        return float((F.conv2d(t, wt(BB + "res4.0.conv2.weight"), padding=1) * s2 + h2).max())
    if site == "rpn_hidden":
        return max(float(F.conv2d(nchw(m.tap(f)), wt(RPN + "conv.weight"), wt(RPN + "conv.bias"), padding=1).max()) for f in ("p2", "p3", "p4", "p5", "p6"))
    if site == "box_fc1":
        pooled, pc = m.tap("box_pooled"), m.tap("prop_count")
        rcap = pooled.shape[0] // B
        rows = np.concatenate([pooled[b * rcap: b * rcap + int(pc[b])] for b in range(B)])
        x = torch.from_numpy(rows).cuda().permute(0, 3, 1, 2).reshape(len(rows), -1)
        return float((x @ wt(BOX + "fc1.weight").t() + wt(BOX + "fc1.bias")).max())
    if site == "mask_fcn1":      # RoIAlign averages the pyramid: the convolution of the pyramid itself bounds what it makes of the pooled crops
        return max(float(F.conv2d(nchw(m.tap(f)), wt(MASK + "mask_fcn1.weight"), wt(MASK + "mask_fcn1.bias"), padding=1).max()) for f in ("p2", "p3", "p4", "p5"))
    raise KeyError(site)


def pow2_for(peak, top=19):
    """k with peak * 2^k in [2^top, 2^(top + 1))"""
    assert peak > 0
    return top - int(np.floor(np.log2(peak)))


class Pair:
    """the same network on a default (AMP_CONV_F16X3) context and on an AMP_CONV_F32 context, reused across the sites through load_params"""

    def __init__(self, train):
        from ampis_amd import ops, params as P, synth
        from ampis_amd.model import MaskRCNN
        self.train = train
        n = 1 if train else B
        self.imgs, gts = synth.batch(n, H, W, seed=31)
        self.gts = [dict(boxes=g["boxes"][:25], classes=g["classes"][:25], polygons=g["polygons"][:25]) for g in gts]
        self.base = P.init_params(K, seed=3, style="spread")
        kw = dict(max_batch=n, max_h=H, max_w=W, max_out_hw=max(H, W), detections_per_image=D)
        if train:
            kw.update(train=True, max_gt=512, max_poly_doubles=512 * 64)
        self.kw = kw
        self.ctx16, self.ctx32 = ops.torch_context(0), ops.torch_context(0)
        self.ctx32.conv_mode = "f32"
        assert self.ctx16.conv_mode == self.ctx16.CONV_F16X3
        self.m16, self.m32 = MaskRCNN(self.ctx16, K, **kw), MaskRCNN(self.ctx32, K, **kw)
        # what a fresh model on a fresh AMP_CONV_F16X3 context returns for the unscaled parameters
        ctx = ops.torch_context(0)
        m = MaskRCNN(ctx, K, **kw)
        m.load_params(self.base)
        self.fresh16 = self.step(m) if train else m.infer(self.imgs)
        assert m.f32_reruns == 0
        m.close()
        ctx.close()
        self._k = {}

    def step(self, m, seed=3):
        """(the five losses, the gradient of every trainable tensor) of one training step"""
        losses = m.forward_losses(self.imgs, self.gts, seed=seed, backward=True)
        return losses, {n: m.get_tensor(n, grad=True) for n in m.trainable_names()}

    def k(self, site):
        """the power of two of a site, from the fp32 context's inference taps on the unscaled parameters"""
        if not self._k:
            from ampis_amd.model import MaskRCNN
            kw = dict(self.kw, max_batch=B)
            for f in ("train", "max_gt", "max_poly_doubles"):
                kw.pop(f, None)
            from ampis_amd import synth
            imgs, _ = synth.batch(B, H, W, seed=31)
            m = MaskRCNN(self.ctx32, K, **kw)
            m.load_params(self.base)
            m.infer(imgs)
            for s in SITES:
                self._k[s] = pow2_for(site_peak(m, self.base, s))
            m.close()
        return self._k[site]

    def close(self):
        self.m16.close(); self.m32.close(); self.ctx16.close(); self.ctx32.close()


@pytest.fixture(scope="module")
def infer_pair():
    p = Pair(train=False)
    yield p
    p.close()


@pytest.fixture(scope="module")
def train_pair():
    p = Pair(train=True)
    yield p
    p.close()


def step_differences(a, b):
    """the names of the losses and gradients that differ in any bit"""
    (la, ga), (lb, gb) = a, b
    bad = [n for n in la if np.float32(la[n]).tobytes() != np.float32(lb[n]).tobytes()]
    bad += [n for n in ga if ga[n].tobytes() != gb[n].tobytes()]
    return bad


def raise_stale_flag(ctx):
    """one poisoned op-level convolution on the context, its flag left unread (read here WITHOUT clearing: it must be up)"""
    import torch
    import range_guard_cases as G
    import test_conv_exact_gpu as E
    c = next(q for q in G.GUARD_CASES if q["name"] == "f16x3_64_s2")
    inputs, kernel = E.planned(c)
    d = dict(E.operands(c, "I"))
    x = d["x"].copy()
    x[G.x_positions(c)[0][1]] = np.nan
    d["x"] = x
    t = E.upload(c, d, kernel)
    y = torch.empty(E.y_shape(c), device="cuda:0")
    E.launch(ctx, c, inputs, t, None, y)
    assert ctx.conv_range_flag(clear=False), "the op-level overflow did not raise the flag"


# ---- inference ----------------------------------------------------------------------------------------------------------------------------------
def test_in_range_call_is_not_rerun_and_is_deterministic(infer_pair):
    p = infer_pair
    p.m16.load_params(p.base)
    n0 = p.m16.f32_reruns
    out = p.m16.infer(p.imgs)
    assert p.m16.f32_reruns == n0
    assert sum(len(o["scores"]) for o in out) > 0
    assert same_bytes(out, p.fresh16)


@pytest.mark.parametrize("site", list(SITES))
def test_overflow_at_a_site_is_rerun_and_equals_the_fp32_context(infer_pair, site):
    p = infer_pair
    k = p.k(site)
    q = scaled(p.base, site, k)
    p.m32.load_params(q)
    ref = p.m32.infer(p.imgs)
    assert p.m32.f32_reruns == 0 and sum(len(o["scores"]) for o in ref) > 0
    p.m16.load_params(q)
    n0 = p.m16.f32_reruns
    got = p.m16.infer(p.imgs)
    assert p.m16.f32_reruns == n0 + 1, f"{site} (2^{k}): the call was re-run {p.m16.f32_reruns - n0} times"
    assert same_bytes(got, ref), f"{site}: the re-run differs from the AMP_CONV_F32 context's call"
    # the next call, in range again, is an AMP_CONV_F16X3 call like any other
    p.m16.load_params(p.base)
    again = p.m16.infer(p.imgs)
    assert p.m16.f32_reruns == n0 + 1, f"{site}: an in-range call after a re-run was re-run too"
    assert same_bytes(again, p.fresh16), f"{site}: the in-range call after a re-run differs from a fresh model's"


def test_stale_op_level_flag_does_not_switch_inference_to_fp32(infer_pair):
    p = infer_pair
    p.m16.load_params(p.base)
    raise_stale_flag(p.ctx16)
    n0 = p.m16.f32_reruns
    out = p.m16.infer(p.imgs)
    assert same_bytes(out, p.fresh16), "a range flag left by an earlier op-level call changed the model call's bytes"
    assert p.m16.f32_reruns == n0


def test_weights_beyond_the_range_leave_the_split_path_without_a_rerun(infer_pair):
    """one res3 weight of 61000 (compensated by 2^-16 in the layer's FrozenBN scale): amp_model_finalize takes the layer out of the split path"""
    from test_e2e_gpu import _relerr
    p = infer_pair
    name = BB + "res3.1.conv2"
    q = dict(p.base)
    w = q[name + ".weight"].copy()
    w[0, 0, 0, 0] = 61000.0
    q[name + ".weight"] = w
    q[name + ".norm.weight"] = p.base[name + ".norm.weight"] * np.float32(2.0 ** -16)
    p.m32.load_params(q)
    p.m32.infer(p.imgs)
    ref = p.m32.tap("res3")
    p.m16.load_params(q)
    n0 = p.m16.f32_reruns
    p.m16.infer(p.imgs)
    assert p.m16.f32_reruns == n0
    got = p.m16.tap("res3")
    assert np.isfinite(got).all() and np.abs(ref).max() > 0
    assert _relerr(got, ref) < 2e-5 * (1 + 2)          # the bound of tests/test_e2e_gpu.py::test_backbone_fpn_taps for res3
    p.m16.load_params(p.base)


# ---- training -----------------------------------------------------------------------------------------------------------------------------------
def test_stale_op_level_flag_does_not_switch_a_training_step_to_fp32(train_pair):
    p = train_pair
    p.m16.load_params(p.base)
    raise_stale_flag(p.ctx16)
    n0 = p.m16.f32_reruns
    got = p.step(p.m16)
    assert not step_differences(got, p.fresh16), "a range flag left by an earlier op-level call changed the step"
    assert p.m16.f32_reruns == n0


def test_fp32_context_steps_agree_bit_for_bit(train_pair):
    p = train_pair
    p.m32.load_params(p.base)
    a, b = p.step(p.m32), p.step(p.m32)
    assert not step_differences(a, b)
    assert all(np.isfinite(v) for v in a[0].values()) and any(np.abs(g).max() > 0 for g in a[1].values())


@pytest.mark.parametrize("site", ["res4_conv2", "box_fc1"])
def test_forward_overflow_in_training_is_rerun_and_equals_the_fp32_context(train_pair, site):
    p = train_pair
    q = scaled(p.base, site, p.k(site))
    p.m32.load_params(q)
    ref = p.step(p.m32)
    p.m16.load_params(q)
    n0 = p.m16.f32_reruns
    got = p.step(p.m16)
    assert p.m16.f32_reruns == n0 + 1
    bad = step_differences(got, ref)
    assert not bad, f"{site}: {len(bad)} losses / gradients of the re-run differ from the AMP_CONV_F32 context's step: {bad[:6]}"


def test_backward_only_overflow_is_rerun_and_training_goes_on(train_pair):
    """loss weights of 2^20 (any finite weight is accepted) leave the forward pass alone and lift the loss gradients, which the data-gradient
    convolutions split after another 2^16, beyond the range"""
    p = train_pair
    big = dict(rpn_loss_weight=2.0 ** 20, box_bbox_reg_loss_weight=2.0 ** 20)
    try:
        p.m32.load_params(p.base)
        p.m32.set_loss_opts(**big)
        ref = p.step(p.m32)
        p.m16.load_params(p.base)
        # the forward pass alone is in range
        p.m16.set_loss_opts(**big)
        n0 = p.m16.f32_reruns
        p.m16.forward_losses(p.imgs, p.gts, seed=3, backward=False)
        assert p.m16.f32_reruns == n0, "the forward pass must stay in range: the overflow is meant for the backward pass only"
        got = p.step(p.m16)
        assert p.m16.f32_reruns == n0 + 1
        bad = step_differences(got, ref)
        assert not bad, f"{len(bad)} losses / gradients of the re-run differ from the AMP_CONV_F32 context's step: {bad[:6]}"
    finally:
        p.m16.set_loss_opts()
        p.m32.set_loss_opts()
    # the re-run left usable gradients: the update works, and the next step, in range, runs in AMP_CONV_F16X3
    before = p.m16.get_tensor(BOX + "fc2.weight")
    p.m16.sgd_step(1e-3, 0.9, 1e-4, grad_scale=2.0 ** -20)
    assert not np.array_equal(before, p.m16.get_tensor(BOX + "fc2.weight"))
    n1 = p.m16.f32_reruns
    losses, grads = p.step(p.m16)
    assert p.m16.f32_reruns == n1
    assert all(np.isfinite(v) for v in losses.values()) and all(np.isfinite(g).all() for g in grads.values())
