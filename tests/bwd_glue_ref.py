"""Shared by tests/test_bwd_glue_ref.py and tests/test_bwd_glue_gpu.py: plain NumPy references of the small kernels a training step strings
between its convolutions (train_bwd.hip, the column sums of wgrad.hip, pointwise.hip), written from the wording of include/ampis_hip.h.

Tensors are NHWC float32 arrays.  Where the header specifies individually rounded fp32 operations (or pure data movement) the reference
computes in float32, one NumPy operation per rounded operation, and its result is THE result: the device tests compare bit patterns.
Reductions whose order the header leaves open (the 2x2 sums, the column sums) are returned as float64 sums; the device tests compare them
exactly on inputs for which every order is exact, and within a derived bound otherwise."""
import numpy as np

F32 = np.float32
LO_SCALE = F32(2048.0)           # lo' = (x - hi) * 2^11
LO_INV = F32(2.0 ** -11)


def _pow2(shift):
    return F32(2.0 ** int(shift))


# ---- the split hi|lo' row format (include/ampis_hip.h, "The split operand format as a tensor format") ----
def split_halves(b):
    """split rows [..., C] (float32 container) -> (hi, lo') float16 arrays [..., C]: per 32 channels 64 B of hi, then 64 B of lo'."""
    b = np.ascontiguousarray(b, dtype=F32)
    C = b.shape[-1]
    assert C % 32 == 0
    h = b.view(np.float16).reshape(b.shape[:-1] + (C // 32, 2, 32))
    return h[..., 0, :].reshape(b.shape), h[..., 1, :].reshape(b.shape)


def join_halves(hi, lo):
    """the inverse of split_halves"""
    C = hi.shape[-1]
    assert C % 32 == 0 and hi.shape == lo.shape and hi.dtype == lo.dtype == np.float16
    h = np.empty(hi.shape[:-1] + (C // 32, 2, 32), np.float16)
    h[..., 0, :] = hi.reshape(hi.shape[:-1] + (C // 32, 32))
    h[..., 1, :] = lo.reshape(lo.shape[:-1] + (C // 32, 32))
    return h.reshape(hi.shape[:-1] + (2 * C,)).view(F32)


def split_rows_ref(x, shift=0):
    """fp32 [..., C] (C % 32 == 0) -> the split rows of x * 2^shift: hi = float16(x) (round to nearest even, inf beyond the f16 range),
    lo' = float16((x - float32(hi)) * 2048)."""
    x = np.ascontiguousarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xs = x * _pow2(shift)
        hi = xs.astype(np.float16)
        lo = ((xs - hi.astype(F32)) * LO_SCALE).astype(np.float16)
    return join_halves(hi, lo)


def unsplit_rows_ref(b):
    """split rows -> float32(hi) + float32(lo') * 2^-11"""
    hi, lo = split_halves(b)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return hi.astype(F32) + lo.astype(F32) * LO_INV


def split_positive(act_split):
    """the mask of the split kernels: what the split kept of the activation is positive"""
    with np.errstate(invalid="ignore"):
        return unsplit_rows_ref(act_split) > 0


# ---- masks ----
def relu_mask_ref(g, act):
    """where(act > 0, g, 0): a select -- an inf or NaN in g under a masked-out cell gives 0; a NaN activation is not positive"""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(act, F32) > 0, np.asarray(g, F32), F32(0))


def relu_mask_split_ref(g, act_split):
    return np.where(split_positive(act_split), np.asarray(g, F32), F32(0))


def relu_mask_to_split_ref(g, act_split, shift=0):
    return split_rows_ref(relu_mask_split_ref(g, act_split), shift)


# ---- stride-2 maps and the FPN top-down sum ----
def upsample2_bwd_ref(dfine, dcoarse=None):
    """dcoarse + the 2x2 sums of dfine [B, 2Hc, 2Wc, C], in float64 (the order of the five-term sum is the kernel's)"""
    f = np.asarray(dfine, np.float64)
    s = f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2]
    return s if dcoarse is None else s + np.asarray(dcoarse, np.float64)


def upsample2_bwd_abs_ref(dfine, dcoarse=None):
    """the sum of the magnitudes of the same terms (the scale of the rounding bound)"""
    return upsample2_bwd_ref(np.abs(dfine), None if dcoarse is None else np.abs(dcoarse))


def subsample2_ref(x):
    return np.ascontiguousarray(np.asarray(x)[:, ::2, ::2])


def subsample2_bwd_ref(dy, dx):
    """dx[:, ::2, ::2] += dy (one rounded add per element); every other cell of dx keeps its bits"""
    out = np.array(dx, dtype=F32, copy=True)
    out[:, ::2, ::2] = out[:, ::2, ::2] + np.asarray(dy, F32)
    return out


def subsample2_bwd_split_ref(dy_split, dx, shift=0):
    """dx[:, ::2, ::2] += decode(dy_split) * 2^-shift"""
    out = np.array(dx, dtype=F32, copy=True)
    out[:, ::2, ::2] = out[:, ::2, ::2] + unsplit_rows_ref(dy_split) * _pow2(-shift)
    return out


def accumulate_split_ref(dy_split, dx, shift=0):
    """dx + decode(dy_split) * 2^-shift"""
    return np.asarray(dx, F32) + unsplit_rows_ref(dy_split) * _pow2(-shift)


def scatter2_rows_ref(src_bits, H, W):
    """uint32 patterns [B, ceil(H/2), ceil(W/2), C] -> [B, H, W, C]: the source chunks at the even positions, +0.0 bits elsewhere"""
    src_bits = np.asarray(src_bits)
    assert src_bits.dtype == np.uint32
    B, Ho, Wo, C = src_bits.shape
    assert (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    up = np.zeros((B, H, W, C), np.uint32)
    up[:, ::2, ::2] = src_bits
    return up


# ---- the small-K data gradient ----
def small_k_dgrad_ref(dl, K, w, keep=None, unmasked=None):
    """dx[p][c] = keep[p][c] ? sum_k dl[p][k] * w[k][c] : 0 -- the sum over k in index order starting from +0, the multiply and the add
    each rounded in float32.  dl [npix, ld >= K], w [K, C]; keep: boolean [npix, C] or None.  unmasked: this function's result for
    keep = None on the same dl, K and w, to mask it again without summing again."""
    dl, w = np.asarray(dl, F32), np.asarray(w, F32)
    assert w.shape[0] == K <= dl.shape[1]
    acc = unmasked
    if acc is None:
        acc = np.zeros((dl.shape[0], w.shape[1]), F32)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for k in range(K):
                acc = acc + dl[:, k:k + 1] * w[k][None, :]
    return acc if keep is None else np.where(keep, acc, F32(0))


def small_k_dgrad_split_ref(dl, K, w, keep, shift=0, unmasked=None):
    """(split rows of that value * 2^shift, the float64 column sums of that value)"""
    dx = small_k_dgrad_ref(dl, K, w, keep, unmasked)
    return split_rows_ref(dx, shift), dx.astype(np.float64).sum(0)


# ---- column sums ----
def colsum_ref(dy):
    return np.asarray(dy, np.float64).sum(0)


def colsum_split_ref(dy, shift=0):
    """(float64 column sums of dy, split rows of dy * 2^shift)"""
    return colsum_ref(dy), split_rows_ref(dy, shift)


def colsum_of_split_ref(dy_split, shift=0):
    """float64 column sums of the values the split rows hold, times 2^-shift"""
    return unsplit_rows_ref(dy_split).astype(np.float64).sum(0) * 2.0 ** -int(shift)


def colsum_finish_ref(partial):
    return np.asarray(partial, np.float64).sum(0)


# ---- the rest ----
def deconv_grad_transpose_ref(grad_in, out=None):
    """[Cin][T][C2] -> [T][C2][Cin], added to `out` when given"""
    t = np.ascontiguousarray(np.asarray(grad_in, F32).transpose(1, 2, 0))
    return t if out is None else np.asarray(out, F32) + t


def sgd_update_ref(p, g, v, lr, momentum, weight_decay, grad_scale):
    """g' = grad_scale * g + wd * p;  v = mu * v + g';  p -= lr * v -- every product, sum and difference rounded in float32: (p, v)"""
    p, g, v = np.asarray(p, F32), np.asarray(g, F32), np.asarray(v, F32)
    gp = g * F32(grad_scale) + F32(weight_decay) * p
    vn = F32(momentum) * v + gp
    return p - F32(lr) * vn, vn


def preprocess_ref(img_bgr, Hp, Wp, mean, std, img_hw=None):
    """uint8 [B, H, W, 3] -> float32 [B, Hp, Wp, 4]: (float32(p) - mean) / std in float32 inside each image's (h, w) = img_hw[b] (the
    whole frame without img_hw), zeros outside it, in the padding and in the fourth channel"""
    img = np.asarray(img_bgr)
    assert img.dtype == np.uint8
    B, H, W, _ = img.shape
    v = (img.astype(F32) - np.asarray(mean, F32)) / np.asarray(std, F32)
    out = np.zeros((B, Hp, Wp, 4), F32)
    for b in range(B):
        h, w = (H, W) if img_hw is None else (int(img_hw[b][0]), int(img_hw[b][1]))
        out[b, :h, :w, :3] = v[b, :h, :w]
    return out


def maxpool3x3s2_ref(x):
    """max_pool2d(kernel 3, stride 2, padding 1): the padding never wins (it acts as -inf)"""
    x = np.asarray(x, F32)
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((B, H + 2, W + 2, C), -np.inf, F32)
    xp[:, 1:-1, 1:-1] = x
    out = np.full((B, Ho, Wo, C), -np.inf, F32)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2])
    return out
