"""Anchor labelling and the two seeded samplers on the device, bit for bit against tests/train_fwd_ref.py through the C ABI:
amp_anchor_labels (anchor_match_kernel, anchor_label_kernel), amp_rpn_sample_loss_ex (rpn_sample_select_kernel and the selection of
rpn_sample_loss_kernel on both dispatch paths) and amp_roi_sample (roi_sample_kernel), with the top-k selection of select.h under all three.

No tolerance.  The cases (tests/train_fwd_cases.py) are the smallest at which the work is cut differently: the 256-GT LDS tile, the 64-lane
ballot chunk, the wave bounding boxes, the 49 152-anchor sample chunk and the rule that chooses between the chunked and the one-workgroup
selection; tests/test_train_fwd_ref.py asserts on the CPU that each case holds its edge and which seeded defect it catches.  Every output and
scratch buffer lies between sentinel bands that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_fwd_cases as Cs
import train_fwd_ref as R
from train_fwd_cases import cases
from train_fwd_harness import AMP_OK, DEV, SENTINEL, Guarded, _abi, dev, levels_of, same

pytestmark = pytest.mark.gpu
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- anchor labels
@pytest.mark.parametrize("name", Cs.LABEL_NAMES)
def test_anchor_labels_bit_for_bit(gpu_ctx, name):
    from ampis_amd import ops
    c = cases("label_cases")[name]
    want = R.anchor_labels_ref(c["levels"], c["cells"], c["gt"], c["lo"], c["hi"])
    lv = levels_of(c["levels"], c["sizes"], c["ratios"])
    for l, cell in enumerate(ops.cell_anchors(sizes=[list(s) if hasattr(s, "__len__") else [s] for s in c["sizes"]], ratios=list(c["ratios"]))):
        same(np.asarray(cell, F32)[:len(c["cells"][l])], c["cells"][l], (name, "cell anchors", l))
    B, N = want["label"].shape
    gt = np.concatenate([np.asarray(g, F32).reshape(-1, 4) for g in c["gt"]])
    off = np.concatenate([[0], np.cumsum([len(g) for g in c["gt"]])]).astype(np.int32)
    d_gt, d_off = dev(gt), dev(off)
    mv, mi, best, lab = Guarded(4 * B * N), Guarded(4 * B * N), Guarded(4 * max(len(gt), 1)), Guarded(B * N)
    assert (B * N) % 4 == 0
    ops.check(_abi().amp_anchor_labels(gpu_ctx.handle, C.byref(lv), B, d_gt.data_ptr(), d_off.data_ptr(), len(gt), float(F32(c["lo"])), float(F32(c["hi"])),
                                       mv.ptr, mi.ptr, best.ptr, lab.ptr), "amp_anchor_labels")
    torch.cuda.synchronize()
    same(mv.host("match_val", np.float32), want["match_val"], (name, "match_val"))
    same(mi.host("match_idx", np.int32), want["match_idx"], (name, "match_idx"))
    same(best.host("gt_best")[:len(gt)], want["gt_best"], (name, "gt_best"))
    same(lab.host("label", np.int8), want["label"], (name, "label"))


# ---------------------------------------------------------------------------------------------------------------- RPN sampler
_PRED = {}


def _zero_preds(levels, B, ld):
    """the prediction maps the loss half of the kernel reads: zeros, one set per shape (the largest: 2 x 65 536 x 16 floats on p2)"""
    key = (levels, B, ld)
    if key not in _PRED:
        _PRED[key] = [torch.zeros((B, h * w, ld), device=DEV) for h, w, _ in levels]
    return _PRED[key]


def run_rpn_sample(ctx, c):
    from ampis_amd import _lib, ops
    L = _abi()
    B, batch, N = c["B"], c["batch"], Cs.total(c["levels"])
    preds = _zero_preds(c["levels"], B, 16)
    lv = levels_of(c["levels"], (32, 64, 128, 256, 512), Cs.RATIOS, preds)
    d_gt, d_off = dev(np.tile(np.asarray([[0, 0, 32, 32]], F32), (B, 1))), dev(np.arange(B + 1, dtype=np.int32))
    d_lab, d_mi = torch.from_numpy(c["label"]).to(DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV)
    keys, sampled, counts, partial = Guarded(4 * B * N), Guarded(4 * B * batch), Guarded(8 * B), Guarded(8 * B)
    st = L.amp_rpn_sample_loss_ex(ctx.handle, C.byref(lv), None, B, d_gt.data_ptr(), d_off.data_ptr(), d_lab.data_ptr(), d_mi.data_ptr(), keys.ptr, batch,
                                  c["pos_max"], c["seed"], sampled.ptr, counts.ptr, partial.ptr, C.byref(_lib.loss_opts({})))
    ops.check(st, "amp_rpn_sample_loss_ex")
    torch.cuda.synchronize()
    keys.host("keys scratch")
    partial.host("partial")
    return sampled.host("sampled", np.int32).reshape(B, batch), counts.host("counts", np.int32).reshape(B, 2), L.amp_debug_last_rpn_sample_path(ctx.handle)


@pytest.mark.parametrize("name", Cs.RPN_SAMPLE_NAMES)
def test_rpn_sampler_bit_for_bit(gpu_ctx, name):
    c = cases("rpn_sample_cases")[name]
    want_s, want_c = R.rpn_sample_ref(c["label"], c["seed"], c["batch"], c["pos_max"])
    path, nch = R.rpn_sample_path_ref(Cs.total(c["levels"]), c["B"], c["batch"])
    got_s, got_c, got_path = run_rpn_sample(gpu_ctx, c)
    assert got_path == (1 if path == "chunked" else 0), (name, path, nch, got_path)
    same(got_c, want_c, (name, "counts"))
    for b in range(c["B"]):
        n = int(want_c[b].sum())
        same(got_s[b, :n], want_s[b, :n], (name, "sampled", b))
        assert (got_s[b, n:].view(np.uint32) == SENTINEL).all(), (name, "a slot behind the counted prefix was written")


# ---------------------------------------------------------------------------------------------------------------- RoI sampler
def run_roi_sample(ctx, d, **over):
    from ampis_amd import ops
    a = dict(d)
    a.update(over)
    B, Pcap, batch = a["B"], a["Pcap"], a["batch"]
    gt = np.concatenate([g.reshape(-1, 4) for g in a["gt"]]) if sum(len(g) for g in a["gt"]) else np.zeros((0, 4), F32)
    cls = np.concatenate(a["cls"]).astype(np.int32) if len(gt) else np.zeros(0, np.int32)
    off = np.concatenate([[0], np.cumsum([len(g) for g in a["gt"]])]).astype(np.int32)
    ncap = Pcap + max(len(g) for g in a["gt"])          # P + G <= ncap
    t = [dev(a["prop"]), dev(a["count"]), dev(gt), dev(cls), dev(off), dev(a["anchor"])]
    keys, csc, gsc = Guarded(4 * B * ncap), Guarded(4 * B * ncap), Guarded(4 * B * ncap)
    rois, rcls, rgti, counts = Guarded(16 * B * batch), Guarded(4 * B * batch), Guarded(4 * B * batch), Guarded(8 * B)
    st = _abi().amp_roi_sample(ctx.handle, B, t[0].data_ptr(), t[1].data_ptr(), Pcap, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), a["K"], batch,
                               a["fg_max"], float(F32(a["thresh"])), a["seed"], keys.ptr, csc.ptr, gsc.ptr, ncap, rois.ptr, rcls.ptr, rgti.ptr, counts.ptr,
                               t[5].data_ptr(), a["num_anchors"])
    if st != AMP_OK:          # a refused call has written nothing
        torch.cuda.synchronize()
        for g in (keys, csc, gsc, rois, rcls, rgti, counts):
            assert (g.host("refused call") == SENTINEL).all()
        return st, None
    torch.cuda.synchronize()
    for g, what in ((keys, "keys scratch"), (csc, "class scratch"), (gsc, "gt scratch")):
        g.host(what)
    return st, (rois.host("rois", np.float32).reshape(B, batch, 4), rcls.host("roi_cls", np.int32).reshape(B, batch),
                rgti.host("roi_gti", np.int32).reshape(B, batch), counts.host("counts", np.int32).reshape(B, 2))


@pytest.mark.parametrize("name", Cs.ROI_SAMPLE_NAMES)
def test_roi_sampler_bit_for_bit(gpu_ctx, name):
    d = cases("roi_sample_cases")[name]
    want = Cs.roi_ref_of(d)
    st, got = run_roi_sample(gpu_ctx, d)
    assert st == AMP_OK
    same(got[3], want[3], (name, "counts"))
    same(got[0], want[0], (name, "rois"))          # the zero boxes behind the counted prefix included
    same(got[1], want[1], (name, "roi_cls"))       # ... and the -1 slots
    for b in range(d["B"]):
        n = int(want[3][b].sum())
        same(got[2][b, :n], want[2][b, :n], (name, "roi_gti", b))
        assert (got[2][b, n:].view(np.uint32) == SENTINEL).all(), (name, "roi_gti behind the counted prefix was written")


# ---------------------------------------------------------------------------------------------------------------- refusals (host side)
def test_refusals_return_before_any_launch(gpu_ctx):
    """AMP_REQUIRE checks: batch 513, num_pos_max > batch, ld < 5 A, num_fg_max > batch, RoI batch 2049 -- a status, and nothing written"""
    from ampis_amd import _lib
    L = _abi()
    c = dict(cases("rpn_sample_cases")["180/scarce"])
    B, N = c["B"], Cs.total(c["levels"])
    preds = _zero_preds(c["levels"], B, 16)
    d_gt, d_off = dev(np.tile(np.asarray([[0, 0, 32, 32]], F32), (B, 1))), dev(np.arange(B + 1, dtype=np.int32))
    d_lab, d_mi = torch.from_numpy(c["label"]).to(DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV)
    for batch, pos_max, ld in ((513, 128, 16), (256, 257, 16), (256, 128, 14)):
        lv = levels_of(c["levels"], (32, 64, 128, 256, 512), Cs.RATIOS, preds, ld=ld)
        keys, sampled, counts, partial = Guarded(4 * B * N), Guarded(4 * B * 520), Guarded(8 * B), Guarded(8 * B)
        st = L.amp_rpn_sample_loss_ex(gpu_ctx.handle, C.byref(lv), None, B, d_gt.data_ptr(), d_off.data_ptr(), d_lab.data_ptr(), d_mi.data_ptr(), keys.ptr, batch,
                                      pos_max, 1, sampled.ptr, counts.ptr, partial.ptr, C.byref(_lib.loss_opts({})))
        torch.cuda.synchronize()
        assert st != AMP_OK, (batch, pos_max, ld)
        for g in (keys, sampled, counts, partial):
            assert (g.host("refused call") == SENTINEL).all()
    d = cases("roi_sample_cases")["iou-edges"]
    assert run_roi_sample(gpu_ctx, d, fg_max=d["batch"] + 1)[0] != AMP_OK
    assert run_roi_sample(gpu_ctx, d, batch=2049, fg_max=16)[0] != AMP_OK
    torch.cuda.synchronize()
