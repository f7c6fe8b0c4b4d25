"""The loss kernels on the device against tests/train_fwd_ref.py through the C ABI: amp_rpn_sample_loss_ex (rpn_sample_loss_kernel<REG>),
amp_box_loss_ex (box_loss_kernel<REG>), amp_mask_target_loss[_fmt] (mask_target_loss_kernel, the polygon path) and amp_sigmoid_focal_loss.

The sampled sets are known from the reference, so predictions are shaped per row (tests/train_fwd_cases.py).  Checked per element:
* the structure of every gradient map bit for bit -- which cells are written, which stay zero, pad columns, unused rows;
* every value without a transcendental on its path bit for bit -- L1 gradients, the q = 0, 1 delta gradients, the pinned GIoU subgradient at
  a corner equal to the GT corner, the polygon mask targets;
* every other value within its own derived bound (train_fwd_ref.E: roundings and the ulp limits of expf / logf / log1pf / powf, node by
  node).  The worst error / bound of each comparison is printed; a correct kernel sits below 1.
Every output buffer lies between sentinel bands that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_fwd_cases as Cs
import train_fwd_ref as R
from train_fwd_cases import cases
from train_fwd_harness import BAND, DEV, Guarded, _abi, dev, levels_of, same

pytestmark = pytest.mark.gpu
F32 = np.float32


def _opts(d, head):
    from ampis_amd import _lib
    if head == "rpn":
        return _lib.loss_opts(dict(rpn_loss_type=d["ltype"], rpn_smooth_l1_beta=d["beta"], rpn_loss_weight=d["w_cls"], rpn_bbox_reg_loss_weight=d["w_loc"]))
    return _lib.loss_opts(dict(box_loss_type=d["ltype"], box_smooth_l1_beta=d["beta"], box_bbox_reg_loss_weight=d["w_reg"], rpn_loss_weight=0.25))


def check_map(got, gm, what, preset=None):
    """a gradient map against its GradMap: unwritten cells keep their preset bit for bit, written ones by R.check_bound"""
    got = np.asarray(got, F32).reshape(gm.v.shape)
    keep = ~gm.written
    want = np.zeros(gm.v.shape, F32) if preset is None else preset
    bad = keep & (R.bits(got) != R.bits(want))
    assert not bad.any(), (what, f"{int(bad.sum())} cells the kernel must not write differ", np.argwhere(bad)[:4].tolist())
    el = gm.as_e()
    w = gm.written
    return R.check_bound(got[w], R.E(el.v[w], el.e[w], el.f[w], el.x[w]), what)


# ---------------------------------------------------------------------------------------------------------------- RPN losses
@pytest.mark.parametrize("name", Cs.RPN_LOSS_NAMES)
def test_rpn_loss_per_element(gpu_ctx, name):
    from ampis_amd import ops
    d = cases("rpn_loss_cases")[name]
    R.E.unsafe.clear()
    partial_ref, maps = Cs.rpn_loss_ref_of(d)
    assert not R.E.unsafe, R.E.unsafe
    B, batch, N = 2, d["batch"], Cs.total(d["levels"], d["A"])
    preds = [torch.from_numpy(p).to(DEV).contiguous() for p in d["preds"]]
    lv = levels_of(d["levels"], d["sizes"], Cs.RATIOS, preds)
    assert lv.A == d["A"] and lv.ld == d["ld"]
    dp = [Guarded(4 * p.numel()) for p in preds]
    for g in dp:
        g.buf[BAND:BAND + g.words] = 0          # the caller zero-fills
    dp_arr = (C.c_void_p * 5)(*[g.ptr for g in dp])
    gt = np.concatenate(d["gt"])
    off = np.concatenate([[0], np.cumsum([len(g) for g in d["gt"]])]).astype(np.int32)
    t = [dev(gt), dev(off), torch.from_numpy(d["lab"]["label"]).to(DEV), dev(d["lab"]["match_idx"])]
    keys, sampled, counts, partial = Guarded(4 * B * N), Guarded(4 * B * batch), Guarded(8 * B), Guarded(8 * B)
    ops.check(_abi().amp_rpn_sample_loss_ex(gpu_ctx.handle, C.byref(lv), dp_arr, B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), keys.ptr,
                                            batch, d["pos_max"], d["seed"], sampled.ptr, counts.ptr, partial.ptr, C.byref(_opts(d, "rpn"))), "amp_rpn_sample_loss_ex")
    torch.cuda.synchronize()
    keys.host("keys")
    same(counts.host("counts", np.int32).reshape(B, 2), d["counts"], (name, "counts"))
    got_s = sampled.host("sampled", np.int32).reshape(B, batch)
    for b in range(B):
        n = int(d["counts"][b].sum())
        same(got_s[b, :n], d["sampled"][b, :n], (name, "sampled", b))
    worst = {}
    got_p = partial.host("partial", np.float32).reshape(B, 2)
    for b in range(B):
        for j, what in enumerate(("bce", "reg")):
            worst[what] = max(worst.get(what, 0.0), R.check_bound(got_p[b, j], partial_ref[b][j], (name, "partial", what, b)))
    for l, (g, gm) in enumerate(zip(dp, maps)):
        worst["dpred"] = max(worst.get("dpred", 0.0), check_map(g.host(f"dpred {l}", np.float32), gm, (name, "dpred", l)))
    print(f"{name}: worst error / bound {({k: round(v, 3) for k, v in worst.items()})}; exact cells {sum(int((m.written & m.x).sum()) for m in maps)} of "
          f"{sum(int(m.written.sum()) for m in maps)} written")


# ---------------------------------------------------------------------------------------------------------------- box losses
@pytest.mark.parametrize("name", Cs.BOX_LOSS_NAMES)
def test_box_loss_per_element(gpu_ctx, name):
    from ampis_amd import ops
    d = cases("box_loss_cases")[name]
    R.E.unsafe.clear()
    partial_ref, gm = Cs.box_loss_ref_of(d)
    assert not R.E.unsafe, R.E.unsafe
    assert gm.written.all()
    B, batch, K, ld = d["B"], d["batch"], d["K"], d["ld"]
    gt = np.concatenate([g.reshape(-1, 4) for g in d["roi"]["gt"]])
    off = np.concatenate([[0], np.cumsum([len(g) for g in d["roi"]["gt"]])]).astype(np.int32)
    t = [dev(d["pred"]), dev(d["rois"]), dev(d["roi_cls"]), dev(np.maximum(d["roi_gti"], 0)), dev(gt), dev(off)]
    dp, partial = Guarded(4 * B * batch * ld), Guarded(8 * B)          # dpred starts as the sentinel: every cell must be written
    w = (C.c_float * 4)(*d["w"])
    ops.check(_abi().amp_box_loss_ex(gpu_ctx.handle, B, batch, K, t[0].data_ptr(), ld, dp.ptr, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                     t[5].data_ptr(), w, d["total_rois"], partial.ptr, C.byref(_opts(d, "box"))), "amp_box_loss_ex")
    torch.cuda.synchronize()
    got = dp.host("dpred", np.float32).reshape(B * batch, ld)
    unused = (d["roi_cls"].reshape(-1) < 0)
    assert not R.bits(got[unused]).any(), (name, "an unused row holds a non-zero word")
    assert not R.bits(got[:, 5 * K + 1:]).any(), (name, "a pad column holds a non-zero word")
    worst = {"dpred": check_map(got, gm, (name, "dpred"))}
    got_p = partial.host("partial", np.float32).reshape(B, 2)
    for b in range(B):
        for j, what in enumerate(("ce", "reg")):
            worst[what] = max(worst.get(what, 0.0), R.check_bound(got_p[b, j], partial_ref[b][j], (name, "partial", what, b)))
    print(f"{name}: worst error / bound {({k: round(v, 3) for k, v in worst.items()})}; exact cells {int(gm.x.sum())} of {gm.x.size}")


# ---------------------------------------------------------------------------------------------------------------- mask targets
def test_polygon_mask_targets_bit_for_bit(gpu_ctx):
    """target_out against mask_target_ref('double') on every case, the ratio instances included; K = 3 with the class channel in the middle:
    the other channels' dlogits are exact zeros; several polygons per instance through amp_mask_target_loss_fmt"""
    from ampis_amd import ops
    mc = cases("mask_cases")
    N, K = len(mc), 3
    polys = [p for _, ps, _ in mc for p in ps]
    poff = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    ipoff = np.concatenate([[0], np.cumsum([len(ps) for _, ps, _ in mc])]).astype(np.int32)
    boxes = np.stack([b for _, _, b in mc]).astype(F32)
    rng = np.random.default_rng(9)
    logits = (rng.standard_normal((N, 28, 28, K)) * 2).astype(F32)
    t = [dev(logits), dev(boxes), dev(np.full(N, 1, np.int32)), dev(np.arange(N, dtype=np.int32)), torch.from_numpy(np.concatenate(polys)).to(DEV), dev(poff), dev(ipoff)]
    dl, partial, target = Guarded(4 * logits.size), Guarded(4 * N), Guarded(N * 784)
    ops.check(_abi().amp_mask_target_loss_fmt(gpu_ctx.handle, N, K, t[0].data_ptr(), dl.ptr, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                              t[5].data_ptr(), t[6].data_ptr(), None, None, partial.ptr, target.ptr), "amp_mask_target_loss_fmt")
    torch.cuda.synchronize()
    got = target.host("target_out", np.uint8).reshape(N, 28, 28)
    want = np.stack([R.mask_target_ref(ps, b, "double") for _, ps, b in mc])
    other = np.stack([R.mask_target_ref(ps, b, "float") for _, ps, b in mc])
    for i, (name, _, _) in enumerate(mc):
        bad = int((got[i] != want[i]).sum())
        assert bad == 0, (name, f"{bad} target pixels differ from the double-ratio reference", int((got[i] != other[i]).sum()))
    assert sum(int((want[i] != other[i]).any()) for i in range(N)) >= 6
    assert set(np.unique(got).tolist()) <= {0, 1}
    g = dl.host("dlogits", np.float32).reshape(N, 28, 28, K)
    assert not R.bits(g[..., 0]).any() and not R.bits(g[..., 2]).any(), "a channel that is not the RoI's class has a gradient"
    # the class channel: per-element bound on the gradient, the per-RoI sums through the 64-lane strided accumulation and tree
    x = logits[..., 1].reshape(N, 784)
    loss, grad = R.bce_ref(x, want.reshape(N, 784).astype(F32))
    inv = F32(1.0) / (F32(N) * F32(28) * F32(28))
    worst_g = R.check_bound(g[..., 1].reshape(N, 784), grad * inv, "mask dlogits")
    acc = R.E.of(np.zeros((N, 64), F32))
    for i0 in range(0, 784, 64):
        part = loss[:, i0:i0 + 64]
        n = part.v.shape[1]
        s = acc[:, :n] + part
        first = i0 == 0
        s = part if first else s
        acc = R.E(np.concatenate([s.v, acc.v[:, n:]], 1), np.concatenate([s.e, acc.e[:, n:]], 1), np.concatenate([s.f, acc.f[:, n:]], 1), np.concatenate([s.x, acc.x[:, n:]], 1))
    o = 32
    while o:
        acc = acc[:, :o] + acc[:, o:2 * o]
        o //= 2
    worst_p = R.check_bound(partial.host("partial", np.float32), acc[:, 0], "mask partial")
    print(f"mask targets: {N} instances, 0 differing pixels; worst error / bound dlogits {worst_g:.3f}, per-RoI sums {worst_p:.3f}")
    # the single-polygon entry point gives the same targets on the single-polygon instances
    single = [i for i, (_, ps, _) in enumerate(mc) if len(ps) == 1]
    sp = [mc[i][1][0] for i in single]
    t2 = [dev(logits[single]), dev(boxes[single]), dev(np.full(len(single), 1, np.int32)), dev(np.arange(len(single), dtype=np.int32)),
          torch.from_numpy(np.concatenate(sp)).to(DEV), dev(np.concatenate([[0], np.cumsum([len(p) for p in sp])]).astype(np.int32))]
    partial2, target2 = Guarded(4 * len(single)), Guarded(len(single) * 784)
    ops.check(_abi().amp_mask_target_loss(gpu_ctx.handle, len(single), K, t2[0].data_ptr(), None, t2[1].data_ptr(), t2[2].data_ptr(), t2[3].data_ptr(),
                                          t2[4].data_ptr(), t2[5].data_ptr(), partial2.ptr, target2.ptr), "amp_mask_target_loss")
    torch.cuda.synchronize()
    same(target2.host("target_out", np.uint8).reshape(-1, 28, 28), want[single].astype(np.uint8), "single-polygon entry point")
    same(partial2.host("partial", np.float32), partial.host("partial", np.float32)[single], "single-polygon partial sums")


# ---------------------------------------------------------------------------------------------------------------- focal loss
@pytest.mark.parametrize("name", Cs.FOCAL_NAMES)
def test_focal_loss_per_element(gpu_ctx, name):
    from ampis_amd import ops
    x, labels, K, alpha, gamma, scale = cases("focal_cases")[name]
    loss, grad = R.focal_ref(x, labels, K, alpha, gamma, scale)
    N = len(labels)
    total = N * K
    grid = max(1, min(2048, (total + 255) // 256))
    t = [dev(x), dev(labels)]
    dl, partial, out = Guarded(4 * total), Guarded(4 * grid), Guarded(4)
    ops.check(_abi().amp_sigmoid_focal_loss(gpu_ctx.handle, N, K, t[0].data_ptr(), t[1].data_ptr(), float(F32(alpha)), float(F32(gamma)), float(F32(scale)), dl.ptr,
                                            partial.ptr, grid, out.ptr), "amp_sigmoid_focal_loss")
    torch.cuda.synchronize()
    g = dl.host("dlogits", np.float32).reshape(N, K)
    assert not R.bits(g[labels < 0]).any(), "an ignored row has a gradient"
    worst_g = R.check_bound(g, grad, (name, "dlogits"))
    # a workgroup's partial: thread t adds its elements t, t + 256 * grid, ... (one each here), then the 256-slot tree
    assert total <= 256 * grid
    flat = R.E(loss.v.reshape(-1), loss.e.reshape(-1), loss.f.reshape(-1), loss.x.reshape(-1))
    got_p = partial.host("partial", np.float32)
    worst_p, parts = 0.0, []
    for b in range(grid):
        parts.append(R.tree_sum(flat[b * 256:min((b + 1) * 256, total)], 256))
        worst_p = max(worst_p, R.check_bound(got_p[b], parts[-1], (name, "partial", b)))
    s = parts[0]
    for p in parts[1:]:
        s = s + p
    worst_l = R.check_bound(out.host("loss", np.float32)[0], s * F32(scale), (name, "loss"))
    if name.startswith("single"):          # one live element per workgroup: its partial IS that element's loss
        live = np.flatnonzero(labels >= 0)
        assert (live % 256 == 0).all() and len(live) == grid
    assert np.isfinite(g).all() and np.isfinite(got_p).all()
    print(f"{name}: worst error / bound dlogits {worst_g:.3f}, partial {worst_p:.3f}, loss {worst_l:.3f}")
