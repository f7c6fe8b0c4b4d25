"""Per-stage entry points of libampis_hip.so on torch CUDA tensors (torch = device memory + stream only).

Used by the parity tests and by tools; the end-to-end path (ampis_amd.engine) calls amp_infer instead.
Every function launches on the stream of the Context it is given and never falls back to torch math.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, check, lib, ptr


def torch_context(device=0):
    """Context bound to torch's current HIP stream on `device` (so torch ops and ours are ordered)."""
    if not torch.cuda.is_available():
        raise _lib.AmpError("no HIP device visible: the ampis_amd hot path has no CPU fallback")
    with torch.cuda.device(device):
        return _lib.Context(device, borrow_stream=torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()), "need contiguous fp32 CUDA tensor"
    return t


FMT_X_SPLIT, FMT_Y_SPLIT, FMT_RES_SPLIT = 1, 2, 4


def split_rows(ctx, t):
    """fp32 tensor [..., C] (C % 32 == 0) -> the same bytes in the split hi|lo' row format (amp_split_weights)."""
    _f32c(t)
    out = torch.empty_like(t)
    check(lib().amp_split_weights(ctx.handle, ptr(t), t.numel() // t.shape[-1], t.shape[-1], ptr(out)), "amp_split_weights")
    return out


def unsplit_rows(ctx, t):
    """the inverse: rows of hi|lo' halves -> fp32 (exact)."""
    _f32c(t)
    out = torch.empty_like(t)
    check(lib().amp_unsplit_rows(ctx.handle, ptr(t), t.numel() // t.shape[-1], t.shape[-1], ptr(out)), "amp_unsplit_rows")
    return out


def conv2d_nhwc(ctx, x, w, scale=None, shift=None, res=None, stride=1, pad=0, relu=False, res_mode=None,
                deconv2x2=False, mask=None, scatter2=False, out=None, fmt=0):
    """x [B,H,W,Cin], w [Cout,KH,KW,Cin] -> y [B,Ho,Wo,Cout] (or [B,2Ho,2Wo,Cout/4] when deconv2x2).
    fmt: FMT_* bits -- x / res arrive in, y leaves in the split row format (AMP_CONV_F16X3 only)."""
    _f32c(x), _f32c(w), _f32c(scale), _f32c(shift), _f32c(res)
    B, H, W, Cin = x.shape
    Cout, KH, KW, Cin2 = w.shape
    assert Cin == Cin2
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    if res_mode is None:
        res_mode = 0 if res is None else 1
    d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride, pad, int(relu), int(res_mode), 2 if scatter2 else int(deconv2x2))
    if out is not None:
        y = out
    elif deconv2x2:
        y = torch.empty((B, 2 * Ho, 2 * Wo, Cout // 4), device=x.device, dtype=torch.float32)
    elif scatter2:
        y = torch.zeros((B, 2 * Ho, 2 * Wo, Cout), device=x.device, dtype=torch.float32)
    else:
        y = torch.empty((B, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    if fmt:
        assert mask is None
        check(lib().amp_conv2d_nhwc_fmt(ctx.handle, C.byref(d), ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(res), ptr(y), int(fmt)),
              "amp_conv2d_nhwc_fmt")
        return y
    check(lib().amp_conv2d_nhwc_ex(ctx.handle, C.byref(d), ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(res), ptr(_f32c(mask)), ptr(y)),
          "amp_conv2d_nhwc_ex")
    return y


def bottleneck64_tail(ctx, x_split, w2, scale2, shift2, w3, scale3, shift3, res_split):
    """conv2 (3x3, 64 -> 64) + FrozenBN + ReLU + conv3 (1x1, 64 -> C3) + FrozenBN + shortcut + ReLU of a res2 block in one launch
    (amp_bottleneck64_tail); x_split [B,H,W,64] and res_split [B,H,W,C3] split rows, w2 [64,3,3,64] / w3 [C3,1,1,64] fp32 -> y split rows."""
    _f32c(x_split), _f32c(w2), _f32c(w3), _f32c(res_split)
    B, H, W, _ = x_split.shape
    C3 = w3.shape[0]
    w2s, w3s = split_rows(ctx, w2.reshape(64, 576)), split_rows(ctx, w3.reshape(C3, 64))
    y = torch.empty((B, H, W, C3), device=x_split.device, dtype=torch.float32)
    check(lib().amp_bottleneck64_tail(ctx.handle, B, H, W, ptr(x_split), ptr(w2s), ptr(_f32c(scale2)), ptr(_f32c(shift2)), ptr(w3s), ptr(_f32c(scale3)),
                                      ptr(_f32c(shift3)), C3, ptr(res_split), ptr(y)), "amp_bottleneck64_tail")
    return y


def conv2d_grouped_nhwc(ctx, x, w, groups, scale=None, shift=None, res=None, stride=1, pad=0, relu=False, fmt=0):
    """Grouped conv (ResNeXt conv2): x [B,H,W,C], w [C,KH,KW,C/groups] (grouped OHWI) -> y [B,Ho,Wo,C].
    fmt: FMT_* bits (split-format x / y / res, AMP_CONV_F16X3 only)."""
    _f32c(x), _f32c(w), _f32c(scale), _f32c(shift), _f32c(res)
    B, H, W, Cin = x.shape
    Cout, KH, KW, cpg = w.shape
    assert Cin == Cout and cpg * groups == Cin
    w_win = torch.empty((Cout, KH, KW, 64), device=x.device, dtype=torch.float32)
    check(lib().amp_group_expand_weights(ctx.handle, ptr(w), Cout, KH, KW, cpg, ptr(w_win)), "amp_group_expand_weights")
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride, pad, int(relu), 0 if res is None else 1, 0)
    y = torch.empty((B, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    if fmt:
        check(lib().amp_conv2d_grouped_nhwc_fmt(ctx.handle, C.byref(d), int(groups), ptr(x), ptr(w_win), ptr(scale), ptr(shift), ptr(res), ptr(y), int(fmt)),
              "amp_conv2d_grouped_nhwc_fmt")
        return y
    check(lib().amp_conv2d_grouped_nhwc(ctx.handle, C.byref(d), int(groups), ptr(x), ptr(w_win), ptr(scale), ptr(shift), ptr(res), ptr(y)),
          "amp_conv2d_grouped_nhwc")
    return y


def resize_bilinear_u8(ctx, img, h, w):
    """img uint8 ndarray [H,W,3] (host) -> resized uint8 ndarray [h,w,3]; PIL-exact bilinear on the device (amp_resize_bilinear_u8)."""
    import numpy as np
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W, _ = img.shape
    src = torch.from_numpy(img).to("cuda:%d" % ctx.device)
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device=src.device)
    tmp = torch.empty(int(lib().amp_resize_scratch_bytes(H, W, h, w)), dtype=torch.uint8, device=src.device)
    torch.cuda.synchronize()
    check(lib().amp_resize_bilinear_u8(ctx.handle, ptr(src), H, W, ptr(dst), h, w, ptr(tmp)), "amp_resize_bilinear_u8")
    check(lib().amp_sync(ctx.handle), "amp_sync")
    return dst.cpu().numpy()


def conv2d_wgrad(ctx, x, dy, w_shape, stride=1, pad=0, scale=None, grad=None, dy_shift=0, x_shift=0, x_split=False, bias_grad=None,
                 bias_accumulate=False):
    """x [B,H,W,Cin], dy [B,Ho,Wo,Cout] -> dW [Cout,KH,KW,Cin] (accumulated into `grad` when given).  x_split: x is in the split
    hi|lo' row format (split_rows / a conv with FMT_Y_SPLIT); x_split = 3: dy as well, ALREADY multiplied by 2**dy_shift.  bias_grad [Cout]: also receives (or accumulates) the column sums of dy."""
    _f32c(x), _f32c(dy)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w_shape
    d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride, pad, 0, 0, 0)
    n = lib().amp_conv_wgrad_scratch_floats(C.byref(d))
    scratch = torch.empty(n, device=x.device)
    acc = grad is not None
    if grad is None:
        grad = torch.empty(w_shape, device=x.device)
    check(lib().amp_conv2d_wgrad_fmt(ctx.handle, C.byref(d), ptr(x), ptr(dy), ptr(scale), ptr(scratch), ptr(grad), int(acc),
                                     int(dy_shift), int(x_shift), int(x_split), ptr(bias_grad), int(bool(bias_accumulate))), "amp_conv2d_wgrad")
    return grad


def dgrad_weights(ctx, w, scale=None):
    Cout, KH, KW, Cin = w.shape
    wt = torch.empty((Cin, KH, KW, Cout), device=w.device)
    check(lib().amp_dgrad_weights(ctx.handle, ptr(_f32c(w)), ptr(scale), Cout, KH, KW, Cin, ptr(wt)), "amp_dgrad_weights")
    return wt


def dgrad_weights_split(ctx, w, scale=None):
    """the data-gradient form of w in the split row format, in one pass (= split_rows(dgrad_weights(w, scale)) bit for bit)."""
    Cout, KH, KW, Cin = w.shape
    wt = torch.empty((Cin, KH, KW, Cout), device=w.device)
    check(lib().amp_dgrad_weights_split(ctx.handle, ptr(_f32c(w)), ptr(scale), Cout, KH, KW, Cin, ptr(wt)), "amp_dgrad_weights_split")
    return wt


def _colsum_out(dy, out, accumulate):
    """(M, N, scratch, out) of a column-sum call on dy [M, N]: the wrapper owns the scratch of ceil(M / 512) slices."""
    M, N = dy.shape
    scratch = torch.empty((max((M + 511) // 512, 1), N), device=dy.device)
    if out is None:
        assert not accumulate, "accumulate needs the tensor to add to"
        out = torch.empty(N, device=dy.device)
    assert _f32c(out).shape == (N,)
    return M, N, scratch, out


def _rows_ptr(t, spare):
    """Pointer of a [M, N] operand; an empty one (M == 0: no row is read or written) stands on `spare`, since the library refuses NULL."""
    return ptr(t if t.numel() else spare)


def colsum(ctx, dy, out=None, accumulate=False):
    """out[n] (= or +=) sum over the rows of dy [M, N] (N % 4 == 0, M >= 0), fixed summation order (amp_colsum)."""
    M, N, scratch, out = _colsum_out(_f32c(dy), out, accumulate)
    check(lib().amp_colsum(ctx.handle, _rows_ptr(dy, scratch), M, N, ptr(scratch), ptr(out), int(bool(accumulate))), "amp_colsum")
    return out


def colsum_split(ctx, dy, shift=0, out=None, accumulate=False):
    """colsum that also returns dy * 2**shift as split rows (amp_colsum_split; N % 32 == 0): (out, dy_split)."""
    M, N, scratch, out = _colsum_out(_f32c(dy), out, accumulate)
    dy_split = torch.empty_like(dy)
    check(lib().amp_colsum_split(ctx.handle, _rows_ptr(dy, scratch), M, N, ptr(scratch), ptr(out), int(bool(accumulate)), _rows_ptr(dy_split, scratch),
                                 int(shift)), "amp_colsum_split")
    return out, dy_split


def colsum_of_split(ctx, dy_split, shift=0, out=None, accumulate=False):
    """The column sums of a dy given as split rows of dy * 2**shift (amp_colsum_of_split; N % 32 == 0)."""
    M, N, scratch, out = _colsum_out(_f32c(dy_split), out, accumulate)
    check(lib().amp_colsum_of_split(ctx.handle, _rows_ptr(dy_split, scratch), M, N, ptr(scratch), ptr(out), int(bool(accumulate)), int(shift)),
          "amp_colsum_of_split")
    return out


def colsum_finish(ctx, partial, out=None, accumulate=False):
    """out[n] (= or +=) the sum of partial [parts, N] over its parts (parts >= 1), the second pass of the column sums (amp_colsum_finish)."""
    parts, N = _f32c(partial).shape
    if out is None:
        assert not accumulate, "accumulate needs the tensor to add to"
        out = torch.empty(N, device=partial.device)
    assert _f32c(out).shape == (N,)
    check(lib().amp_colsum_finish(ctx.handle, ptr(partial), parts, N, ptr(out), int(bool(accumulate))), "amp_colsum_finish")
    return out


# ------------------------------------------------------------------------------------------------------------------
# Backward and pointwise kernels between the convolutions of a training step (train_bwd.hip, pointwise.hip).  Gradient maps are
# NHWC fp32 or split rows; `shift`: a split gradient holds value * 2**shift.  In-place functions return the tensor they changed.
# ------------------------------------------------------------------------------------------------------------------
def _half(n):
    return (n - 1) // 2 + 1


def upsample2_bwd(ctx, dfine, dcoarse, init=False):
    """dcoarse [B,Hc,Wc,C] += the 2x2 sums of dfine [B,2Hc,2Wc,C] (amp_upsample2_bwd); init: dcoarse = the sums, its content is not read
    (amp_upsample2_bwd_init)."""
    B, Hc, Wc, Cc = _f32c(dcoarse).shape
    assert _f32c(dfine).shape == (B, 2 * Hc, 2 * Wc, Cc)
    fn = lib().amp_upsample2_bwd_init if init else lib().amp_upsample2_bwd
    check(fn(ctx.handle, ptr(dfine), ptr(dcoarse), B, Hc, Wc, Cc), "amp_upsample2_bwd_init" if init else "amp_upsample2_bwd")
    return dcoarse


def subsample2_bwd(ctx, dy, dx):
    """dx [B,H,W,C][:, ::2, ::2] += dy [B,ceil(H/2),ceil(W/2),C] (amp_subsample2_bwd)."""
    B, H, W, Cc = _f32c(dx).shape
    assert _f32c(dy).shape == (B, _half(H), _half(W), Cc)
    check(lib().amp_subsample2_bwd(ctx.handle, ptr(dy), ptr(dx), B, H, W, Cc), "amp_subsample2_bwd")
    return dx


def subsample2_bwd_split(ctx, dy_split, dx, shift=0):
    """dx[:, ::2, ::2] += decode(dy_split) * 2**-shift (amp_subsample2_bwd_split; C % 32 == 0)."""
    B, H, W, Cc = _f32c(dx).shape
    assert _f32c(dy_split).shape == (B, _half(H), _half(W), Cc)
    check(lib().amp_subsample2_bwd_split(ctx.handle, ptr(dy_split), ptr(dx), B, H, W, Cc, int(shift)), "amp_subsample2_bwd_split")
    return dx


def accumulate_split(ctx, dy_split, dx, shift=0):
    """dx += decode(dy_split) * 2**-shift, same shape [..., C], C % 32 == 0 (amp_accumulate_split)."""
    assert _f32c(dy_split).shape == _f32c(dx).shape
    Cc = dx.shape[-1]
    check(lib().amp_accumulate_split(ctx.handle, ptr(dy_split), ptr(dx), dx.numel() // Cc, Cc, int(shift)), "amp_accumulate_split")
    return dx


def scatter2_rows(ctx, src, H, W, out=None):
    """up [B,H,W,C] with up[:, ::2, ::2] = src [B,ceil(H/2),ceil(W/2),C] as raw bytes and +0.0 everywhere else (amp_scatter2_rows)."""
    B, Ho, Wo, Cc = _f32c(src).shape
    assert (Ho, Wo) == (_half(H), _half(W))
    up = torch.empty((B, H, W, Cc), device=src.device) if out is None else _f32c(out)
    assert up.shape == (B, H, W, Cc)
    check(lib().amp_scatter2_rows(ctx.handle, ptr(src), ptr(up), B, H, W, Cc), "amp_scatter2_rows")
    return up


def relu_mask(ctx, g, act):
    """g = act > 0 ? g : 0 in place (amp_relu_mask; numel % 4 == 0)."""
    assert _f32c(g).shape == _f32c(act).shape
    check(lib().amp_relu_mask(ctx.handle, ptr(g), ptr(act), g.numel()), "amp_relu_mask")
    return g


def relu_mask_split(ctx, g, act_split):
    """the same with act [..., C] as split rows, C % 32 == 0 (amp_relu_mask_split)."""
    assert _f32c(g).shape == _f32c(act_split).shape
    check(lib().amp_relu_mask_split(ctx.handle, ptr(g), ptr(act_split), g.numel(), g.shape[-1]), "amp_relu_mask_split")
    return g


def relu_mask_to_split(ctx, g, act_split, shift=0):
    """split rows of 2**shift * (act > 0 ? g : 0) with act [..., C] as split rows (amp_relu_mask_to_split)."""
    assert _f32c(g).shape == _f32c(act_split).shape
    out = torch.empty_like(g)
    check(lib().amp_relu_mask_to_split(ctx.handle, ptr(g), ptr(act_split), ptr(out), g.numel(), g.shape[-1], int(shift)), "amp_relu_mask_to_split")
    return out


def small_k_dgrad(ctx, dl, w, act=None):
    """dx [npix, C] = act > 0 ? dl[:, :K] @ w : 0 for dl [npix, ld], w [K, C], K <= ld (amp_small_k_dgrad); act None: no mask."""
    (npix, ld), (K, Cc) = _f32c(dl).shape, _f32c(w).shape
    assert act is None or _f32c(act).shape == (npix, Cc)
    dx = torch.empty((npix, Cc), device=dl.device)
    check(lib().amp_small_k_dgrad(ctx.handle, ptr(dl), ld, K, ptr(w), Cc, ptr(act), ptr(dx), npix), "amp_small_k_dgrad")
    return dx


def small_k_dgrad_split(ctx, dl, w, act, shift=0, act_split=True, rows16=False, colsum_out=None, accumulate=False):
    """The same product as split rows of dx * 2**shift, plus colsum_out[c] (= or +=) the column sums of dx: (dx_split, colsum_out).
    act_split: act is split rows (amp_small_k_dgrad_split_ld; rows16: the entry for dl rows of 16 floats, amp_small_k_dgrad_split), else
    fp32 rows (amp_small_k_dgrad_split_f32act).  dl [npix, ld], ld in (4, 8, 12, 16), w [K, C], C % 32 == 0."""
    (npix, ld), (K, Cc) = _f32c(dl).shape, _f32c(w).shape
    assert _f32c(act).shape == (npix, Cc)
    dx = torch.empty((npix, Cc), device=dl.device)
    scratch = torch.empty(((npix + 511) // 512, Cc), device=dl.device)
    if colsum_out is None:
        assert not accumulate, "accumulate needs the tensor to add to"
        colsum_out = torch.empty(Cc, device=dl.device)
    assert _f32c(colsum_out).shape == (Cc,)
    tail = (ptr(w), Cc, ptr(act), ptr(dx), npix, int(shift), ptr(scratch), ptr(colsum_out), int(bool(accumulate)))
    if rows16:
        assert act_split and ld == 16
        check(lib().amp_small_k_dgrad_split(ctx.handle, ptr(dl), K, *tail), "amp_small_k_dgrad_split")
    elif act_split:
        check(lib().amp_small_k_dgrad_split_ld(ctx.handle, ptr(dl), ld, K, *tail), "amp_small_k_dgrad_split_ld")
    else:
        check(lib().amp_small_k_dgrad_split_f32act(ctx.handle, ptr(dl), ld, K, *tail), "amp_small_k_dgrad_split_f32act")
    return dx, colsum_out


def deconv_grad_transpose(ctx, grad_in, out=None, accumulate=False):
    """out [T, C2, Cin] (= or +=) grad_in [Cin, T, C2] transposed: the ConvTranspose weight gradient from its wgrad form
    (amp_deconv_grad_transpose)."""
    Cin, T, C2 = _f32c(grad_in).shape
    if out is None:
        assert not accumulate, "accumulate needs the tensor to add to"
        out = torch.empty((T, C2, Cin), device=grad_in.device)
    assert _f32c(out).shape == (T, C2, Cin)
    check(lib().amp_deconv_grad_transpose(ctx.handle, ptr(grad_in), ptr(out), Cin, T, C2, int(bool(accumulate))), "amp_deconv_grad_transpose")
    return out


def sgd_update(ctx, p, g, v, lr, momentum=0.9, weight_decay=1e-4, grad_scale=1.0):
    """torch.optim.SGD in place on flat tensors: g' = grad_scale * g + wd * p; v = mu * v + g'; p -= lr * v (amp_sgd_update)."""
    assert _f32c(p).shape == _f32c(g).shape == _f32c(v).shape
    check(lib().amp_sgd_update(ctx.handle, ptr(p), ptr(g), ptr(v), p.numel(), float(lr), float(momentum), float(weight_decay), float(grad_scale)),
          "amp_sgd_update")
    return p, v


def preprocess(ctx, img_bgr, Hp, Wp, mean, std, img_hw=None):
    """uint8 BGR [B,H,W,3] -> fp32 [B,Hp,Wp,4] = (x - mean) / std, zero in the padding, in the 4th channel and beyond img_hw[b] = (h, w)
    (int32 [B,2] on the device, optional) (amp_preprocess)."""
    assert img_bgr.is_cuda and img_bgr.dtype == torch.uint8 and img_bgr.is_contiguous() and img_bgr.shape[3] == 3
    assert img_hw is None or (img_hw.is_cuda and img_hw.dtype == torch.int32 and img_hw.is_contiguous() and img_hw.shape == (img_bgr.shape[0], 2))
    B, H, W, _ = img_bgr.shape
    out = torch.empty((B, Hp, Wp, 4), device=img_bgr.device)
    check(lib().amp_preprocess(ctx.handle, ptr(img_bgr), B, H, W, int(Hp), int(Wp), (C.c_float * 3)(*mean), (C.c_float * 3)(*std), ptr(img_hw), ptr(out)),
          "amp_preprocess")
    return out


def maxpool3x3s2(ctx, x):
    """max_pool2d(kernel 3, stride 2, padding 1) of x [B,H,W,C], C % 4 == 0 (amp_maxpool3x3s2)."""
    B, H, W, Cc = _f32c(x).shape
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), device=x.device)
    check(lib().amp_maxpool3x3s2(ctx.handle, ptr(x), B, H, W, Cc, ptr(y)), "amp_maxpool3x3s2")
    return y


def subsample2(ctx, x):
    """x[:, ::2, ::2] of x [B,H,W,C], C % 4 == 0 (amp_subsample2)."""
    B, H, W, Cc = _f32c(x).shape
    y = torch.empty((B, _half(H), _half(W), Cc), device=x.device)
    check(lib().amp_subsample2(ctx.handle, ptr(x), B, H, W, Cc, ptr(y)), "amp_subsample2")
    return y


# ------------------------------------------------------------------------------------------------------------------
# Selection / pooling / mask stages (device tensors in, device tensors out). Integer tensors are int32.
# ------------------------------------------------------------------------------------------------------------------
def _i32(*shape, device="cuda:0"):
    return torch.empty(shape, dtype=torch.int32, device=device)


def _u64(*shape, device="cuda:0"):
    return torch.empty(shape, dtype=torch.int64, device=device)   # same bits; viewed as u64 by the library


def make_rpn_levels(preds, shapes, strides=(4, 8, 16, 32, 64), sizes=(32, 64, 128, 256, 512), ratios=None):
    """sizes: one number per level (with ratios None: the ratios 0.5, 1, 2 -- A = 3) or one list per level; ratios: one list for every level or
    one list per level (MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS).  preds may hold None (host-only use: amp_cell_anchors)."""
    lv = _lib.RpnLevels()
    per_level = any(hasattr(s, "__len__") for s in sizes)
    A = 3
    if per_level or ratios is not None:
        from .model import anchor_lists
        sz = [list(s) if hasattr(s, "__len__") else [s] for s in sizes]
        sz = sz + [sz[-1]] * (5 - len(sz))
        rt = [[0.5, 1.0, 2.0]] if ratios is None else ([list(ratios)] if not hasattr(ratios[0], "__len__") else [list(r) for r in ratios])
        s5, r5 = anchor_lists(sz, rt)
        _lib.fill_anchors(lv, s5, r5)
        A = len(s5[0]) * len(r5[0])
    lv.nlevels, lv.A = len(preds), A
    lv.ld = preds[0].shape[-1] if preds[0] is not None else 16 * ((5 * A + 15) // 16)
    for i, (p, (h, w)) in enumerate(zip(preds, shapes)):
        if p is not None:
            _f32c(p)
            lv.pred[i] = p.data_ptr()
        lv.h[i], lv.w[i], lv.stride[i] = h, w, strides[i]
        lv.anchor_size[i] = 0 if hasattr(sizes[i], "__len__") else int(sizes[i])
    return lv


def cell_anchors(sizes=(32, 64, 128, 256, 512), ratios=None):
    """The cell anchors the kernels use (amp_cell_anchors; host only): list of five float32 arrays [A, 4]."""
    lv = make_rpn_levels([None] * 5, [(1, 1)] * 5, sizes=sizes, ratios=ratios)
    out = []
    for l in range(5):
        buf = np.zeros((9, 4), np.float32)
        n = C.c_int()
        check(lib().amp_cell_anchors(C.byref(lv), l, buf.ctypes.data_as(C.c_void_p), 9, C.byref(n)), "amp_cell_anchors")
        out.append(buf[:n.value].copy())
    return out


def rpn_topk(ctx, preds, shapes, B, k, sizes=(32, 64, 128, 256, 512), ratios=None):
    """preds: per level [B, h*w, ld]. Returns sel_idx [B,L,k] i32, sel_logit [B,L,k] f32, sel_count [B,L] i32."""
    lv = make_rpn_levels(preds, shapes, sizes=sizes, ratios=ratios)
    L = len(preds)
    dev = preds[0].device
    max_n = max(h * w * lv.A for h, w in shapes)
    scratch = torch.empty((B * L * max_n,), dtype=torch.int32, device=dev)
    sel_idx, sel_logit, sel_count = _i32(B, L, k, device=dev), torch.zeros((B, L, k), device=dev), _i32(B, L, device=dev)
    check(lib().amp_rpn_topk(ctx.handle, C.byref(lv), B, k, ptr(scratch), max_n, ptr(sel_idx), ptr(sel_logit), ptr(sel_count)),
          "amp_rpn_topk")
    return sel_idx, sel_logit, sel_count


def rpn_decode(ctx, preds, shapes, B, k, sel_idx, sel_logit, sel_count, img_h, img_w, sizes=(32, 64, 128, 256, 512), ratios=None):
    lv = make_rpn_levels(preds, shapes, sizes=sizes, ratios=ratios)
    cap = len(preds) * k
    dev = preds[0].device
    boxes, keys = torch.empty((B, cap, 4), device=dev), _u64(B, cap, device=dev)
    check(lib().amp_rpn_decode(ctx.handle, C.byref(lv), B, k, ptr(sel_idx), ptr(sel_logit), ptr(sel_count), img_h, img_w, cap,
                               ptr(boxes), ptr(keys), None), "amp_rpn_decode")
    return boxes, keys


def sort_gather(ctx, keys, boxes_in, box_stride=None, n_used=None):
    B, cap = keys.shape
    dev = keys.device
    sb, ss, sc, cnt, pos = torch.empty((B, cap, 4), device=dev), torch.empty((B, cap), device=dev), _i32(B, cap, device=dev), \
        _i32(B, device=dev), _i32(B, cap, device=dev)
    check(lib().amp_sort_gather_n(ctx.handle, B, cap, box_stride or boxes_in.shape[1], ptr(keys), ptr(boxes_in), ptr(sb), ptr(ss),
                                  ptr(sc), ptr(cnt), ptr(pos), None, None, ptr(n_used) if n_used is not None else None), "amp_sort_gather")
    return sb, ss, sc, cnt, pos


def nms(ctx, boxes, cats, counts, thresh, max_keep):
    """boxes [B,cap,4] sorted by descending score, cats [B,cap] i32, counts [B] i32 -> keep_idx [B,max_keep], keep_count [B]."""
    B, cap, _ = boxes.shape
    dev = boxes.device
    W = (cap + 63) // 64
    mask = _u64(B * cap * W, device=dev)
    keep, kc = _i32(B, max_keep, device=dev), _i32(B, device=dev)
    check(lib().amp_nms(ctx.handle, B, cap, ptr(boxes), ptr(cats), ptr(counts), float(thresh), max_keep, ptr(mask), ptr(keep),
                        ptr(kc)), "amp_nms")
    return keep, kc


def rpn_nms_levels(ctx, cand_boxes, cand_keys, sel_count, k, thresh, max_keep, payload=None):
    """Per-level NMS of amp_rpn_decode's candidates + merge: (boxes [B,max_keep,4], logits, levels, count [B], payload or None)."""
    B, cap, _ = cand_boxes.shape
    L = sel_count.shape[1]
    dev = cand_boxes.device
    scratch = _u64(lib().amp_rpn_nms_scratch_words(B, L, k), device=dev)
    pb, ps = torch.empty((B, max_keep, 4), device=dev), torch.empty((B, max_keep), device=dev)
    pl, pc = _i32(B, max_keep, device=dev), _i32(B, device=dev)
    po = _i32(B, max_keep, device=dev) if payload is not None else None
    check(lib().amp_rpn_nms_levels(ctx.handle, B, L, k, cap, ptr(cand_boxes), ptr(cand_keys), ptr(sel_count), float(thresh), max_keep,
                                   ptr(scratch), ptr(pb), ptr(ps), ptr(pl), ptr(pc), ptr(payload) if payload is not None else None,
                                   ptr(po) if po is not None else None), "amp_rpn_nms_levels")
    return pb, ps, pl, pc, po


def make_fpn_feats(feats, strides=(4, 8, 16, 32)):
    f = _lib.FpnFeats()
    for i, t in enumerate(feats):
        _f32c(t)
        f.feat[i] = t.data_ptr()
        f.h[i], f.w[i], f.stride[i] = t.shape[1], t.shape[2], strides[i]
    f.C = feats[0].shape[3]
    return f


def roi_align(ctx, feats, rois, batch_idx, P, fmt=0):
    """feats: [p2..p5] NHWC; rois [R,4]; batch_idx [R] i32 -> ([R,P,P,C], level [R] i32).
    fmt: FMT_X_SPLIT = the feature maps are split rows, FMT_Y_SPLIT = write the pooled tensor as split rows."""
    f = make_fpn_feats(feats)
    R = rois.shape[0]
    out = torch.empty((R, P, P, f.C), device=rois.device)
    lvl = _i32(R, device=rois.device)
    if fmt:
        check(lib().amp_roi_align_fmt(ctx.handle, C.byref(f), ptr(_f32c(rois)), ptr(batch_idx), None, R, P, ptr(out), ptr(lvl), int(fmt)),
              "amp_roi_align_fmt")
    else:
        check(lib().amp_roi_align(ctx.handle, C.byref(f), ptr(_f32c(rois)), ptr(batch_idx), None, R, P, ptr(out), ptr(lvl)),
              "amp_roi_align")
    return out, lvl


def roi_align_bwd(ctx, dfeats, strides, rois, batch_idx, P, dout, B=0):
    """dfeats[l] [B,h,w,256] += RoIAlign-backward(dout [R,P,P,256]) (amp_roi_align_bwd_batched; B = 0: derived from batch_idx)."""
    import ctypes as C_
    ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in dfeats])
    fh = (C_.c_int * 4)(*[f.shape[1] for f in dfeats])
    fw = (C_.c_int * 4)(*[f.shape[2] for f in dfeats])
    st = (C_.c_int * 4)(*strides)
    check(lib().amp_roi_align_bwd_batched(ctx.handle, ptrs, fh, fw, st, dfeats[0].shape[3], ptr(_f32c(rois)), ptr(batch_idx), rois.shape[0], P,
                                          ptr(_f32c(dout)), int(B)), "amp_roi_align_bwd_batched")


def sgd_step_tensors(ctx, p, g, v, offsets, sizes, is_bias, lr, momentum=0.9, weight_decay=1e-4, grad_scale=1.0, *, nesterov=False,
                     bias_lr_factor=1.0, weight_decay_bias=None, clip=None):
    """The general SGD step (amp_sgd_step_tensors; MaskRCNN.sgd_step documents the arithmetic and the keyword arguments) on three flat
    float32 device arenas p / g / v: tensor t is floats [offsets[t], offsets[t] + sizes[t]) (offset % 4 == 0), is_bias[t] puts it in the
    bias group.  p and v are updated in place.  Returns (norms, coefs): float32 arrays [ntensors], N and k of every tensor (0 and 1
    unless clip=("norm", ...))."""
    import numpy as np
    for t in (p, g, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1 and t.numel() == p.numel()
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = np.ascontiguousarray(sizes, dtype=np.uint64)
    bias = np.ascontiguousarray(is_bias, dtype=np.uint8)
    assert off.shape == n.shape == bias.shape and off.ndim == 1
    if len(off) and int((off + n).max()) > p.numel():
        raise ValueError("sgd_step_tensors: a tensor ends beyond the arena")
    o = _lib.sgd_opts(lr, momentum, weight_decay, grad_scale, nesterov, bias_lr_factor, weight_decay_bias, clip)
    norms, coefs = np.empty(len(off), np.float32), np.empty(len(off), np.float32)
    torch.cuda.synchronize()       # the arenas were written on torch's stream
    check(lib().amp_sgd_step_tensors(ctx.handle, ptr(p), ptr(g), ptr(v), ptr(off), ptr(n), ptr(bias), len(off), C.byref(o), ptr(norms), ptr(coefs)),
          "amp_sgd_step_tensors")
    return norms, coefs


def _i32c(t):
    assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda, "expected a contiguous int32 CUDA tensor"
    return t


def box_candidates(ctx, pred, proposals, prop_count, K, score_thresh, img_h, img_w, weights=(10., 10., 5., 5.), ccap=8192, img_hw=None):
    """pred [B*Rcap, ld] or [B, Rcap, ld], proposals [B,Rcap,4], prop_count [B] i32; img_hw: optional device int32 [B,2], the (h, w) every
    image's boxes are clipped to instead of img_h / img_w (amp_box_candidates_sized).
    Returns (dense_boxes [B,Rcap*K,4], keys [B,ccap] sort words, cand_count [B] (may exceed ccap), overflow [1])."""
    B, Rcap, _ = proposals.shape
    dev = pred.device
    assert pred.numel() == B * Rcap * pred.shape[-1] and pred.shape[-1] >= 5 * K + 1 and prop_count.numel() == B
    dense = torch.empty((B, Rcap * K, 4), device=dev)
    keys, cnt, ovf = _u64(B, ccap, device=dev), _i32(B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    w = (C.c_float * 4)(*weights)
    if img_hw is not None:
        assert tuple(img_hw.shape) == (B, 2)
    check(lib().amp_box_candidates_sized(ctx.handle, ptr(_f32c(pred)), pred.shape[-1], ptr(_f32c(proposals)), ptr(_i32c(prop_count)), B, Rcap,
                                         K, w, float(score_thresh), img_h, img_w, ptr(_i32c(img_hw)) if img_hw is not None else None,
                                         ptr(dense), ptr(keys), ccap, ptr(cnt), ptr(ovf)), "amp_box_candidates")
    return dense, keys, cnt, ovf


def gather_dets(ctx, sboxes, sscores, scats, keep_idx, keep_count, payload=None):
    """amp_gather_dets: sorted candidates sboxes [B,cap,4] / sscores [B,cap] / scats [B,cap] i32 (/ payload [B,cap] i32), keep_idx [B,D] i32
    positions in [0, cap), keep_count [B] i32 -> (det_boxes [B,D,4], det_scores [B,D], det_classes [B,D], payload [B,D] or None); the rows
    from keep_count[b] on are zeros, class and payload -1."""
    B, cap, _ = sboxes.shape
    D = keep_idx.shape[1]
    dev = sboxes.device
    assert tuple(sscores.shape) == (B, cap) and tuple(scats.shape) == (B, cap) and keep_idx.shape[0] == B and keep_count.numel() == B
    assert payload is None or tuple(payload.shape) == (B, cap)
    db, ds, dc = torch.empty((B, D, 4), device=dev), torch.empty((B, D), device=dev), _i32(B, D, device=dev)
    po = _i32(B, D, device=dev) if payload is not None else None
    check(lib().amp_gather_dets(ctx.handle, B, cap, D, ptr(_f32c(sboxes)), ptr(_f32c(sscores)), ptr(_i32c(scats)), ptr(_i32c(keep_idx)),
                                ptr(_i32c(keep_count)), ptr(db), ptr(ds), ptr(dc), ptr(_i32c(payload)) if payload is not None else None,
                                ptr(po) if po is not None else None), "amp_gather_dets")
    return db, ds, dc, po


def compact_dets(ctx, det_count, det_boxes, det_scores, det_classes, out=None):
    """amp_compact_dets: det_boxes [B,D,4], det_scores [B,D], det_classes [B,D] i32, det_count [B] i32 (device; clamped to D) -> the first
    min(det_count[b], D) rows of every image in image order: (boxes [B*D,4], scores [B*D], classes [B*D], batch [B*D]), of which the first
    sum(min(det_count, D)) rows are written.  out: the four tensors to write into (rows beyond the total keep their contents)."""
    B, D = det_scores.shape
    dev = det_boxes.device
    assert tuple(det_boxes.shape) == (B, D, 4) and tuple(det_classes.shape) == (B, D) and det_count.numel() == B
    if out is None:
        out = (torch.zeros((B * D, 4), device=dev), torch.zeros((B * D,), device=dev), _i32(B * D, device=dev).zero_(),
               _i32(B * D, device=dev).zero_())
    boxes, scores, classes, batch = out
    assert tuple(boxes.shape) == (B * D, 4) and scores.numel() == B * D and classes.numel() == B * D and batch.numel() == B * D
    check(lib().amp_compact_dets(ctx.handle, B, D, ptr(_i32c(det_count)), ptr(_f32c(det_boxes)), ptr(_f32c(det_scores)), ptr(_i32c(det_classes)),
                                 ptr(_f32c(boxes)), ptr(_f32c(scores)), ptr(_i32c(classes)), ptr(_i32c(batch))), "amp_compact_dets")
    return boxes, scores, classes, batch


def mask_prob(ctx, logits, classes):
    """amp_mask_prob: logits [N,28,28,K], classes [N] i32 -> sigmoid of channel classes[n], [N,28,28] (a class outside [0, K): channel 0)."""
    N, K = logits.shape[0], logits.shape[-1]
    assert tuple(logits.shape) == (N, 28, 28, K) and classes.numel() == N
    prob = torch.empty((N, 28, 28), device=logits.device)
    check(lib().amp_mask_prob(ctx.handle, ptr(_f32c(logits)), ptr(_i32c(classes)), N, K, ptr(prob)), "amp_mask_prob")
    return prob


def paste_rle(ctx, prob, det_boxes, det_batch, out_h, out_w, in_h, in_w, threshold=0.5, pool_counts=1 << 22, in_hw=None, pos_scratch=False,
              return_overflow=False, return_pool=False):
    """prob [N,28,28], det_boxes [N,4], det_batch [N] i32, out_h/out_w [B] i32 (device) (amp_paste_rle_sized).
    in_hw: optional device int32 [B,2], the network-input (h, w) of each image instead of in_h / in_w.
    pos_scratch: the transition positions go to a second pool of pool_counts words and the first holds the run lengths only.
    Returns (out_boxes [N,4], valid [N], list of uint32 run-length arrays); a full pool is an assertion unless return_overflow, which
    appends the overflow flag (the masks that did not fit have no runs).  return_pool appends dict(used, pos_used, off [N], len [N])."""
    N = prob.shape[0]
    dev = prob.device
    B = out_h.numel()
    assert tuple(prob.shape) == (N, 28, 28) and tuple(det_boxes.shape) == (N, 4) and det_batch.numel() == N and out_w.numel() == B
    assert in_hw is None or tuple(in_hw.shape) == (B, 2)
    ob, valid = torch.empty((N, 4), device=dev), _i32(N, device=dev)
    pool = torch.empty((pool_counts,), dtype=torch.int32, device=dev)
    used, off, ln = torch.zeros(1, dtype=torch.int64, device=dev), _u64(N, device=dev), _i32(N, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    pos = torch.empty((pool_counts,), dtype=torch.int32, device=dev) if pos_scratch else None
    pos_used = torch.zeros(1, dtype=torch.int64, device=dev) if pos_scratch else None
    max_hw = int(max(out_h.max().item(), out_w.max().item()))
    check(lib().amp_paste_rle_sized(ctx.handle, ptr(_f32c(prob)), ptr(_f32c(det_boxes)), ptr(_i32c(det_batch)), N, ptr(_i32c(out_h)),
                                    ptr(_i32c(out_w)), max_hw, in_h, in_w, ptr(_i32c(in_hw)) if in_hw is not None else None, float(threshold),
                                    ptr(ob), ptr(valid), ptr(pool), pool_counts, ptr(used), ptr(off), ptr(ln), ptr(ovf),
                                    ptr(pos) if pos_scratch else None, pool_counts if pos_scratch else 0,
                                    ptr(pos_used) if pos_scratch else None), "amp_paste_rle")
    torch.cuda.synchronize()
    overflow = int(ovf.item())
    assert return_overflow or overflow == 0, "RLE pool overflow"
    pool_h = pool.cpu().numpy().view("uint32")
    off_h, ln_h = off.cpu().numpy(), ln.cpu().numpy()
    runs = [pool_h[int(o): int(o) + int(l)].copy() for o, l in zip(off_h, ln_h)]
    ret = (ob, valid, runs)
    if return_overflow:
        ret += (overflow,)
    if return_pool:
        ret += (dict(used=int(used.item()), pos_used=int(pos_used.item()) if pos_scratch else None, off=off_h, len=ln_h),)
    return ret


def rle_strings_device(ctx, pool, off, ln):
    """COCO counts strings of many masks, encoded on the device (amp_rle_strings_device): pool uint32 run lengths (int32 / uint32 tensor on
    the device), mask i = pool[off[i] : off[i] + ln[i]].  Returns the list of bytes objects."""
    import torch
    n = int(off.numel())
    dev = pool.device
    off = off.to(dev).to(torch.int64).contiguous()
    ln = ln.to(dev).to(torch.int32).contiguous()
    pool = pool.contiguous()
    cap = 7 * int(pool.numel()) + 8
    buf = torch.empty(cap, dtype=torch.uint8, device=dev)
    soff = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    slen = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().amp_rle_strings_device(ctx.handle, C.c_void_p(pool.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()), n,
                                       C.c_void_p(buf.data_ptr()), C.c_ulonglong(cap), C.c_void_p(soff.data_ptr()),
                                       C.c_void_p(slen.data_ptr()), C.c_void_p(total.data_ptr())), "amp_rle_strings_device")
    torch.cuda.synchronize()
    t = int(total.item())
    assert t <= cap
    raw = bytes(buf[:t].cpu().numpy().tobytes())
    so, sl = soff.cpu().tolist(), slen.cpu().tolist()
    return [raw[so[i]: so[i] + sl[i]] for i in range(n)]
