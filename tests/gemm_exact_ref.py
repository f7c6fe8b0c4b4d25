"""Shared by tests/test_gemm_exact_ref.py, tests/test_conv_exact_gpu.py and tests/test_wgrad_exact_gpu.py: float64 NumPy references of the
convolution and weight-gradient entry points, written from the wording of include/ampis_hip.h, and the operand classes on which BOTH
convolution arithmetics (AMP_CONV_F32, AMP_CONV_F16X3) are exact, so that the device tests compare bit patterns with no tolerance.

Class I   integers of {-2, ..., 2}, about half of them zero; residual / shift small integers; scale of {+-0.5, +-1, +-2}.  Every product and
          every partial sum is an integer below 2^24 in any summation order; in the split arithmetic hi = x and lo' = 0.
Class L   (AMP_CONV_F16X3 only) one operand is h + l / 2048 with h of {+-5, +-6, +-7} and l of {-3, ..., 3}: float16(h + l / 2048) == h (the
          spacing of float16 in [4, 8) is 2^-8 and |l| / 2048 < 2^-9), so it splits to exactly hi = h, lo' = l; the other operand is an
          integer of {-1, 0, 1} (lo' = 0).  The dropped lo * lo term is zero, and the two accumulators of the kernels (hi * hi, and the two
          cross terms) are each an exact integer sum: the result acc + acx * 2^-11 is exact.  What class I cannot see -- a cross-term MFMA
          left out, the fold -- shows here.
Shifted   a class I / L value times 2^-shift with the entry's dy_shift / in_shift = shift: the kernels multiply by 2^shift first (exact).

Exactness is a condition on the INPUTS, asserted here on the CPU for every case (the *_ref functions raise AssertionError): the sum, the
value after scale, after shift, after the residual (a weight-gradient: the slab bound) must each be an fp32 value, a split-row output must
be a split-row value, and sum |x||w| < 2^24 so that every partial sum in every order is exact too.  They are not tolerances."""
import numpy as np

from bwd_glue_ref import split_rows_ref, unsplit_rows_ref      # noqa: F401  (re-exported: the split row format has one reference)

F32, F64 = np.float32, np.float64
SCALES = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
CONV_DEFECTS = ("border_tap", "last_kstep", "last_row", "swap_kykx", "cross_term", "res_last_ntile")
WGRAD_DEFECTS = ("border_tap", "last_kstep", "last_row", "swap_kykx", "cross_term")


# ---- operand generators (float32 arrays; no negative zeros) -------------------------------------------------------------------
def class_i(rng, shape, zero=0.5):
    """integers of {-2, -1, 1, 2}, a fraction `zero` of them replaced by 0"""
    v = rng.choice(np.array([-2, -1, 1, 2]), size=shape)
    return np.where(rng.random(shape) < zero, 0, v).astype(F32)


def class_l_low(rng, shape):
    """h + l / 2048: the operand of class L whose low half is live"""
    h = rng.choice(np.array([-7, -6, -5, 5, 6, 7]), size=shape).astype(F64)
    l = rng.integers(-3, 4, size=shape).astype(F64)
    v = (h + l / 2048.0).astype(F32)
    assert np.array_equal(v.astype(np.float16).astype(F64), h) and np.array_equal((v.astype(F64) - h) * 2048.0, l)      # splits to exactly (h, l)
    return v


def class_l_int(rng, shape, zero=0.5):
    """integers of {-1, 0, 1}: the other operand of class L (lo' = 0)"""
    v = rng.choice(np.array([-1, 1]), size=shape)
    return np.where(rng.random(shape) < zero, 0, v).astype(F32)


def shifted(v, shift):
    """v * 2^-shift (exact: a power of two on small values), what a scaled loss gradient holds before the entry's 2^shift"""
    out = (v.astype(F64) * 2.0 ** -int(shift)).astype(F32)
    assert np.array_equal(out.astype(F64) * 2.0 ** int(shift), v.astype(F64))
    return out


def scales(rng, n):
    return rng.choice(SCALES, size=n).astype(F32)


def small_ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, size=shape).astype(F32)


def thin(rng, w, keep):
    """keep a fraction of the non-zero weights (large K: until the representability assertions hold)"""
    return np.where(rng.random(w.shape) < keep, w, 0).astype(F32)


# ---- representability ----------------------------------------------------------------------------------------------------------
def assert_f32(a, what):
    a = np.asarray(a, F64)
    bad = a.astype(F32).astype(F64) != a
    assert not bad.any(), f"{what}: {int(bad.sum())} values are not fp32 values (first {a[bad][0]!r})"


def assert_split_value(a, what):
    """every value of a (last dimension % 32 == 0) survives the split row format"""
    a32 = np.asarray(a, F64).astype(F32)
    back = unsplit_rows_ref(split_rows_ref(a32))
    bad = back != a32
    assert not bad.any(), f"{what}: {int(bad.sum())} values are not split-row values (first {a32[bad][0]!r})"


def assert_sum_bound(amax_a, amax_b, K, what):
    """sum |a||b| over K products < 2^24 (times 2^11 where a low half is live the fold still holds 24 bits: checked on the result)"""
    assert float(amax_a) * float(amax_b) * K < 2.0 ** 24, f"{what}: sum |a||b| may reach 2^24 ({amax_a} x {amax_b} x {K})"


def assert_conv_sum_bound(x, w, in_shift, stride, pad, groups, check=True):
    """sum |x||w| < 2^24 at every output: from the largest |x| and |w| and K where that already shows it, else from the convolution of the
    magnitudes (a single element near the edge of the f16 range among small ones).  A non-finite operand (check=False only: a poisoned
    tensor has no exact sum) is left out of the bound."""
    ax, aw = np.abs(np.asarray(x, F64)) * 2.0 ** in_shift, np.abs(np.asarray(w, F64))
    if not check:
        ax, aw = np.where(np.isfinite(ax), ax, 0.0), np.where(np.isfinite(aw), aw, 0.0)
    assert np.isfinite(ax).all() and np.isfinite(aw).all(), "conv: a non-finite operand has no exact reference"
    if ax.max() * aw.max() * (w.shape[1] * w.shape[2] * w.shape[3]) < 2.0 ** 24:
        return
    worst = conv_sum(ax, aw, stride, pad, groups).max()
    assert worst < 2.0 ** 24, f"conv: sum |x||w| reaches {worst} >= 2^24 at some output"


def out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _f16_part(a):
    return np.asarray(a, F32).astype(np.float16).astype(F64)


# ---- convolution -------------------------------------------------------------------------------------------------------------
def conv_sum(x, w, stride=1, pad=0, groups=1, defect=None):
    """sum over (ky, kx, c) of x[b, oy * stride + ky - pad, ox * stride + kx - pad, c] * w[n, ky, kx, c], zero outside the image; float64.
    x [B,H,W,Cin], w [Cout,KH,KW,Cin/groups] -> [B,Ho,Wo,Cout]."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    B, H, W, Cin = x.shape
    Cout, KH, KW, cpg = w.shape
    assert cpg * groups == Cin and Cout % groups == 0
    if defect == "swap_kykx":
        assert KH == KW and KH > 1
        w = w.transpose(0, 2, 1, 3)
    if defect == "last_kstep":          # the last 32 channels of the K order (ky, kx, c) never multiplied
        w = w.copy()
        w[:, KH - 1, KW - 1, max(0, cpg - 32):] = 0
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, Ho, Wo, Cout), F64)
    opg = Cout // groups
    for ky in range(KH):
        for kx in range(KW):
            src = xp
            if defect == "border_tap" and ky == 0 and kx == 0:      # the pixel up-left of (0, 0) read as if it were inside
                assert pad > 0
                src = xp.copy()
                src[:, pad - 1, pad - 1] = x[:, 0, 0]
            patch = src[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            for g in range(groups):
                y[..., g * opg:(g + 1) * opg] += patch[..., g * cpg:(g + 1) * cpg] @ w[g * opg:(g + 1) * opg, ky, kx].T
    if defect == "last_row":
        y[B - 1, Ho - 1, Wo - 1] = 0
    return y


def conv_ref(x, w, scale=None, shift=None, res=None, mask=None, *, stride=1, pad=0, groups=1, relu=False, res_mode=0, out_mode=0, in_shift=0,
             y_split=False, low=None, defect=None, check=True):
    """amp_conv2d_nhwc(_ex / _fmt / grouped): y = act(conv(x, w) * scale[c] + shift[c] (+ res)), then y = mask > 0 ? y : 0.
    x, res, mask: the VALUES (decode split rows first).  in_shift: the kernel multiplies x by 2^in_shift and the sum by 2^-in_shift (a split
    input then HOLDS x * 2^in_shift); pass the true x here, the shift only enters the bound on the partial sums.
    res_mode 1: res [B,Ho,Wo,Cout]; 2: res [B,Ho/2,Wo/2,Cout] nearest-upsampled x2.
    out_mode 0: [B,Ho,Wo,Cout]; 1: Cout = 4 * C2 ordered (ky, kx, co) -> [B,2Ho,2Wo,C2]; 2: [B,2Ho,2Wo,Cout] written at (2oy, 2ox), zero elsewhere.
    mask is indexed like y.  low: None (class I), 'x' or 'w' (class L: which operand carries the low half).  check=False skips the
    representability assertions (a reference with a seeded defect).  Returns float32."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    Cout = w.shape[0]
    f32_check = assert_f32 if check else (lambda a, what: None)
    assert_conv_sum_bound(x, w, in_shift, stride, pad, groups, check)
    xs, ws = x, w
    if defect == "cross_term":
        assert low in ("x", "w")
        xs, ws = (_f16_part(x), w) if low == "x" else (x, _f16_part(w))
    s = conv_sum(xs, ws, stride, pad, groups, defect) + 0.0      # the accumulators start at +0: an exact zero sum is +0
    f32_check(s, "conv sum")
    B, Ho, Wo, _ = s.shape
    t = s * (np.asarray(scale, F64) if scale is not None else 1.0)
    f32_check(t, "after scale")
    t = t + (np.asarray(shift, F64) if shift is not None else 0.0)
    f32_check(t, "after shift")
    if res_mode:
        r = np.asarray(res, F64)
        if defect == "res_last_ntile":
            r = r.copy()
            r[..., Cout - min(64, Cout):] = 0
        if res_mode == 2:
            assert Ho % 2 == 0 and Wo % 2 == 0 and r.shape == (B, Ho // 2, Wo // 2, Cout)
            r = r.repeat(2, axis=1).repeat(2, axis=2)
        assert r.shape == t.shape
        t = t + r
        f32_check(t, "after the residual")
    if relu:
        t = np.maximum(t, 0.0)
    if out_mode == 1:
        C2 = Cout // 4
        t = t.reshape(B, Ho, Wo, 2, 2, C2).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C2)
    elif out_mode == 2:
        z = np.zeros((B, 2 * Ho, 2 * Wo, Cout), F64)
        z[:, ::2, ::2] = t
        t = z
    if mask is not None:
        m = np.asarray(mask, F64)
        assert m.shape == t.shape
        t = np.where(m > 0, t, 0.0)
    if y_split and check:
        assert_split_value(t, "split output")
    return t.astype(F32)


def group_window_weights(w, cpg):
    """grouped weights [Cout][KH][KW][cpg] -> the window layout [Cout][KH][KW][64] of amp_group_expand_weights: slot j of output channel n is
    input channel (n & ~63) + j, zero outside n's group"""
    w = np.asarray(w, F32)
    Cout, KH, KW, _ = w.shape
    out = np.zeros((Cout, KH, KW, 64), F32)
    for n in range(Cout):
        j0 = (n // cpg) * cpg - (n & ~63)
        out[n, :, :, j0:j0 + cpg] = w[n]
    return out


# ---- weight gradient -------------------------------------------------------------------------------------------------------
def wgrad_sum(x, dy, KH, KW, stride=1, pad=0, defect=None):
    """dW[n][ky][kx][c] = sum over pixels m = (b, oy, ox) of dy[m][n] * x[b, oy * stride + ky - pad, ox * stride + kx - pad, c]; float64"""
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    B, H, W, Cin = x.shape
    _, Ho, Wo, N = dy.shape
    assert (Ho, Wo) == out_hw(H, W, KH, KW, stride, pad)
    if defect in ("last_row", "last_kstep"):        # the last pixel / the last 32-pixel step of the sum over m never added
        dy = dy.copy().reshape(-1, N)
        M = dy.shape[0]
        dy[M - (1 if defect == "last_row" else ((M - 1) % 32) + 1):] = 0
        dy = dy.reshape(B, Ho, Wo, N)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    g = np.zeros((N, KH, KW, Cin), F64)
    d2 = dy.reshape(-1, N)
    for ky in range(KH):
        for kx in range(KW):
            src = xp
            if defect == "border_tap" and ky == 0 and kx == 0:
                assert pad > 0
                src = xp.copy()
                src[:, pad - 1, pad - 1] = x[:, 0, 0]
            patch = src[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            g[:, ky, kx] = d2.T @ patch.reshape(-1, Cin)
    if defect == "swap_kykx":
        assert KH == KW and KH > 1
        g = g.transpose(0, 2, 1, 3)
    return g


def wgrad_ref(x, dy, KH, KW, scale=None, grad=None, bias_grad=None, *, stride=1, pad=0, dy_shift=0, want_bias=False, low=None, defect=None, check=True):
    """amp_conv2d_wgrad(_scaled / _fmt): dW (= or +=, when `grad` is given) scale[n] * wgrad(dy, x); with want_bias also the column sums of dy
    (= or += `bias_grad`).  x, dy: the VALUES (unscaled, decoded).  Returns float32 (dW, bias or None)."""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    f32_check = assert_f32 if check else (lambda a, what: None)      # check=False: a reference with a seeded defect
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    # the bound is on the values the kernel multiplies: dy * 2^dy_shift
    if not float(np.abs(x).max()) * float(np.abs(dy).max()) * 2.0 ** dy_shift * M < 2.0 ** 24:
        # a single element near the edge of the f16 range among small ones: the bound from the sums of the magnitudes themselves
        worst = wgrad_sum(np.abs(x), np.abs(dy) * 2.0 ** dy_shift, KH, KW, stride, pad).max()
        assert worst < 2.0 ** 24, f"wgrad slab: sum |x||dy| reaches {worst} >= 2^24"
    xs, ds = x, dy
    if defect == "cross_term":
        assert low in ("x", "dy")
        xs, ds = (_f16_part(x), dy) if low == "x" else (x, _f16_part(dy))
    g = wgrad_sum(xs, ds, KH, KW, stride, pad, defect) + 0.0      # the accumulators start at +0; scale[n] * (+0) keeps scale's sign, as IEEE has it
    f32_check(g, "wgrad sum")
    if scale is not None:
        g = g * np.asarray(scale, F64)[:, None, None, None]
        f32_check(g, "wgrad after scale")
    if grad is not None:
        g = g + np.asarray(grad, F64)
        f32_check(g, "wgrad accumulated")
    b = None
    if want_bias:
        b = np.asarray(dy, F64).sum((0, 1, 2))
        f32_check(b, "bias sums")
        if bias_grad is not None:
            b = b + np.asarray(bias_grad, F64)
            f32_check(b, "bias sums accumulated")
        b = (b + 0.0).astype(F32)
    return g.astype(F32), b


def grouped_wgrad_ref(x, dy, KH, KW, cpg, scale=None, *, stride=1, pad=0, dy_shift=0, defect=None, check=True):
    """amp_conv2d_grouped_wgrad(_fmt): the weight gradient in the window layout [C][KH][KW][64] -- slot j of output channel n is input channel
    (n & ~63) + j -- times scale[n], exact zeros outside n's group.  Returns (float32 window gradient, bool array of the in-group slots)."""
    g, _ = wgrad_ref(x, dy, KH, KW, scale, stride=stride, pad=pad, dy_shift=dy_shift, defect=defect, check=check)
    C = g.shape[0]
    win = np.zeros((C, KH, KW, 64), F32)
    inside = np.zeros((C, KH, KW, 64), bool)
    for n in range(C):
        base = n & ~63
        j0 = (n // cpg) * cpg - base
        win[n, :, :, j0:j0 + cpg] = g[n, :, :, base + j0:base + j0 + cpg]
        inside[n, :, :, j0:j0 + cpg] = True
    return win, inside


def dgrad_weights_ref(w, scale=None):
    """amp_dgrad_weights: wt[c][KH-1-ky][KW-1-kx][n] = w[n][ky][kx][c] * scale[n] (one fp32 product)"""
    w = np.asarray(w, F32)
    if scale is not None:
        w = w * np.asarray(scale, F32)[:, None, None, None]
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


# ---- wgrad slab counts (csrc/wgrad.hip pick_nsplit / pick_nsplit_ring), for choosing M ------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pick_nsplit(M, tiles, per_round=512, overhead=12):
    smax = max(1, min(256, M // 256))
    best, best_s = -1, 1
    for s in range(1, smax + 1):
        steps = _cdiv(_cdiv(M, s), 32)
        cost = _cdiv(tiles * s, per_round) * (steps + overhead)
        if best < 0 or cost < best:
            best, best_s = cost, s
    return best_s


def pick_nsplit_ring(M, tiles):
    return pick_nsplit(M, tiles, 256, 10)


def wgrad_slab_counts(M, Cout, Kp):
    """(slabs of wgrad_f16x3_kernel / wgrad_mfma_kernel on 128 x 128 tiles, slabs of wgrad_split_kernel on 128 x 256 tiles)"""
    return pick_nsplit(M, _cdiv(Cout, 128) * _cdiv(Kp, 128)), pick_nsplit_ring(M, (Cout // 128) * _cdiv(Kp, 256))


def first_difference(got_bits, ref_bits, row_len, tile_m=128, tile_n=64):
    """a failure message: how many 32-bit words differ, the first one, and where it sits (row, column, M tile, N tile)"""
    got_bits, ref_bits = np.asarray(got_bits).reshape(-1), np.asarray(ref_bits).reshape(-1)
    bad = np.flatnonzero(got_bits != ref_bits)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    m, n = divmod(i, row_len)
    return (f"{bad.size} of {got_bits.size} words differ; first at flat index {i}: row {m} (tile {m // tile_m}, row {m % tile_m} of it), column {n} "
            f"(N tile {n // tile_n}, 32-channel step {n // 32}); got 0x{int(got_bits[i]) & 0xffffffff:08x}, want 0x{int(ref_bits[i]) & 0xffffffff:08x}")
