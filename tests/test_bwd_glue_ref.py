"""CPU tests of tests/bwd_glue_ref.py, the NumPy references tests/test_bwd_glue_gpu.py holds the backward and pointwise kernels to:
each reference against torch on the CPU where torch has the operation, and the properties of the split hi|lo' row format the device
tests rely on (include/ampis_hip.h, "The split operand format as a tensor format")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bwd_glue_ref as R

F32 = np.float32


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- against torch ----
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 8)])
def test_upsample2_bwd_ref_is_the_gradient_of_nearest_upsampling(shape):
    rng = np.random.default_rng(1)
    B, Hc, Wc, C = shape
    dfine, dcoarse = rng.standard_normal((B, 2 * Hc, 2 * Wc, C)), rng.standard_normal(shape)
    x = torch.zeros((B, C, Hc, Wc), dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(_nchw(dfine))
    want = _nhwc(x.grad)
    assert np.allclose(R.upsample2_bwd_ref(dfine), want, rtol=1e-13, atol=1e-13)
    assert np.allclose(R.upsample2_bwd_ref(dfine, dcoarse), want + dcoarse, rtol=1e-13, atol=1e-13)
    assert np.array_equal(R.upsample2_bwd_abs_ref(dfine, dcoarse), R.upsample2_bwd_ref(np.abs(dfine), np.abs(dcoarse)))


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 7), (6, 8), (7, 6)])
def test_subsample2_refs_are_the_slice_and_its_gradient(hw):
    rng = np.random.default_rng(2)
    H, W = hw
    x = torch.from_numpy(rng.standard_normal((2, H, W, 4)).astype(F32)).requires_grad_()
    y = x[:, ::2, ::2]
    assert np.array_equal(R.subsample2_ref(x.detach().numpy()), y.detach().numpy())
    dy = rng.standard_normal(tuple(y.shape)).astype(F32)
    y.backward(torch.from_numpy(dy))
    assert np.array_equal(_bits(R.subsample2_bwd_ref(dy, np.zeros((2, H, W, 4), F32))), _bits(x.grad.numpy()))
    # += on a prefilled map: the touched cells add, the others keep their bits (NaN payloads included)
    dx = rng.integers(0, 2 ** 32, (2, H, W, 4), dtype=np.uint32).view(F32)
    dx[:, ::2, ::2] = 1.0
    got = R.subsample2_bwd_ref(dy, dx)
    assert np.array_equal(got[:, ::2, ::2], dy + F32(1.0))
    keep = np.ones((H, W), bool)
    keep[::2, ::2] = False
    assert np.array_equal(_bits(got)[:, keep], _bits(dx)[:, keep])
    # the split variants on a split of dy: the same cells, decode * 2^-shift
    dy32 = rng.standard_normal((2,) + tuple(y.shape[1:3]) + (32,)).astype(F32)
    dx32 = np.zeros((2, H, W, 32), F32)
    got = R.subsample2_bwd_split_ref(R.split_rows_ref(dy32, 3), dx32, 3)
    assert np.array_equal(got[:, ::2, ::2], R.unsplit_rows_ref(R.split_rows_ref(dy32, 3)) * F32(0.125)) and not got[:, 1::2].any() and not got[:, :, 1::2].any()
    assert np.array_equal(R.accumulate_split_ref(R.split_rows_ref(dy32, 3), dy32, 3), dy32 + R.unsplit_rows_ref(R.split_rows_ref(dy32, 3)) * F32(0.125))
    up = R.scatter2_rows_ref(_bits(dy), H, W)
    assert np.array_equal(up[:, ::2, ::2], _bits(dy)) and not up[:, 1::2].any() and not up[:, :, 1::2].any()


def test_relu_mask_ref_is_the_gradient_of_relu():
    rng = np.random.default_rng(3)
    act, g = rng.standard_normal((3, 5, 7, 8)), rng.standard_normal((3, 5, 7, 8))
    x = torch.from_numpy(act).requires_grad_()
    torch.relu(x).backward(torch.from_numpy(g))
    got = R.relu_mask_ref(g.astype(F32), act.astype(F32))
    assert np.array_equal(got, x.grad.numpy().astype(F32))
    # a select, not a product: non-finite gradients under masked-out cells give 0; NaN, -0.0 and 0.0 activations are not positive
    a = np.array([0.0, -0.0, -1.0, np.nan, 2.0 ** -149, 1.0], F32)
    gg = np.array([np.inf, np.nan, -np.inf, np.inf, 3.0, np.nan], F32)
    out = R.relu_mask_ref(gg, a)
    assert np.array_equal(_bits(out[:5]), _bits(np.array([0, 0, 0, 0, 3.0], F32))) and np.isnan(out[5])


@pytest.mark.parametrize("K,ld,C,npix", [(1, 4, 32, 1), (5, 8, 96, 37), (16, 16, 64, 50), (80, 80, 32, 9)])
def test_small_k_dgrad_ref_is_the_gradient_of_a_1x1_convolution(K, ld, C, npix):
    rng = np.random.default_rng(4)
    dl = rng.standard_normal((npix, ld)).astype(F32)
    w = rng.standard_normal((K, C)).astype(F32)
    act = rng.standard_normal((npix, C)).astype(F32)
    x = torch.from_numpy(act.astype(np.float64)).t().reshape(1, C, npix, 1).requires_grad_()
    y = F.conv2d(torch.relu(x), torch.from_numpy(w.astype(np.float64)).reshape(K, C, 1, 1))
    y.backward(torch.from_numpy(dl[:, :K].astype(np.float64)).t().reshape(1, K, npix, 1))
    want = x.grad.reshape(C, npix).t().numpy()
    got = R.small_k_dgrad_ref(dl, K, w, act > 0)
    # K products of relative error 2^-24 pass through at most K additions of relative error 2^-24 each
    bound = (K + 1) * 2.0 ** -24 * (np.abs(dl[:, :K].astype(np.float64)) @ np.abs(w.astype(np.float64)))
    assert (np.abs(got - want) <= bound).all()
    assert np.array_equal((got == 0), ~(act > 0) | (want == 0))
    nomask = R.small_k_dgrad_ref(dl, K, w)
    assert np.array_equal(nomask[act > 0], got[act > 0])
    sp, sums = R.small_k_dgrad_split_ref(dl, K, w, act > 0, 4)
    assert np.array_equal(_bits(sp), _bits(R.split_rows_ref(got * F32(16.0)))) and np.array_equal(sums, got.astype(np.float64).sum(0))


@pytest.mark.parametrize("hw", [(1, 1), (7, 9), (8, 6), (2, 2)])
def test_maxpool_ref_is_max_pool2d_bit_for_bit(hw):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2,) + hw + (8,)).astype(F32)
    x[..., 3] = -np.abs(x[..., 3]) - 1.0          # negative everywhere: a zero padding would win at every border
    want = _nhwc(F.max_pool2d(_nchw(x), 3, 2, 1))
    got = R.maxpool3x3s2_ref(x)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)) and (got[..., 3] < 0).all()


def test_preprocess_ref_is_the_oracles_normalisation():
    from oracle import maskrcnn as O
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (2, 37, 45, 3), dtype=np.uint8)
    cfg = O.Cfg(num_classes=1)
    cfg.pixel_std = (57.375, 57.12, 58.395)
    want = O.preprocess(img, cfg)
    want = (want[0] if isinstance(want, (tuple, list)) else want).permute(0, 2, 3, 1).numpy()
    Hp, Wp = want.shape[1:3]
    assert Hp == 64 and Wp == 64
    got = R.preprocess_ref(img, Hp, Wp, cfg.pixel_mean, cfg.pixel_std)
    assert np.array_equal(_bits(got[..., :3]), _bits(want)) and not got[..., 3].any()
    # a smaller second image: zeros, not (0 - mean) / std, between its size and the frame
    hw = np.array([[37, 45], [20, 31]], np.int32)
    got2 = R.preprocess_ref(img, Hp, Wp, cfg.pixel_mean, cfg.pixel_std, hw)
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1, :20, :31], got[1, :20, :31])
    assert not got2[1, 20:].any() and not got2[1, :, 31:].any() and got[1, 20:37, :45, :3].all()


def test_sgd_update_ref_is_one_step_of_torch_sgd():
    rng = np.random.default_rng(7)
    n, lr, mu, wd = 1000, 0.02, 0.9, 1e-4
    p, g, v = (rng.standard_normal(n).astype(F32) for _ in range(3))
    # torch in float64 on the same float32 values and float32 hyper-parameters; the momentum buffer is set in the optimiser's state
    tp = torch.from_numpy(p.astype(np.float64)).requires_grad_()
    opt = torch.optim.SGD([tp], lr=float(F32(lr)), momentum=float(F32(mu)), weight_decay=float(F32(wd)))
    opt.state[tp]["momentum_buffer"] = torch.from_numpy(v.astype(np.float64)).clone()
    for gs in (1.0, 0.5):
        tp.data.copy_(torch.from_numpy(p.astype(np.float64)))
        opt.state[tp]["momentum_buffer"].copy_(torch.from_numpy(v.astype(np.float64)))
        tp.grad = torch.from_numpy(g.astype(np.float64) * gs)
        opt.step()
        pn, vn = R.sgd_update_ref(p, g, v, lr, mu, wd, gs)
        assert pn.dtype == vn.dtype == F32
        v64 = opt.state[tp]["momentum_buffer"].numpy()
        # seven rounded operations, each within 2^-24 of its result; the magnitudes below bound every intermediate
        vmag = np.abs(g * gs) + wd * np.abs(p) + mu * np.abs(v)
        assert (np.abs(vn - v64) <= 4 * 2.0 ** -24 * vmag).all()
        assert (np.abs(pn - tp.detach().numpy()) <= 2.0 ** -24 * (np.abs(p) + 6 * lr * vmag) + 2.0 ** -24 * np.abs(pn)).all()


# ---- the split format ----
def test_split_layout_and_round_trip_of_22_bit_values():
    rng = np.random.default_rng(8)
    n = rng.integers(-(2 ** 22) + 1, 2 ** 22, (64, 96))
    n[0, :4] = [2 ** 22 - 1, -(2 ** 22) + 1, 1, 0]
    x = (n * 2.0 ** -12).astype(F32)
    assert np.array_equal(x.astype(np.float64), n * 2.0 ** -12)
    b = R.split_rows_ref(x)
    assert b.shape == x.shape and b.dtype == F32
    # the bytes: per 32 channels 64 B of hi halves, then 64 B of lo' halves
    raw = b.view(np.float16).reshape(64, 3, 64)
    hi = x.astype(np.float16)
    assert np.array_equal(raw[:, :, :32].reshape(64, 96), hi)
    assert np.array_equal(raw[:, :, 32:].reshape(64, 96), ((x - hi.astype(F32)) * F32(2048)).astype(np.float16))
    h2, l2 = R.split_halves(b)
    assert np.array_equal(h2, hi) and np.array_equal(_bits(R.join_halves(h2, l2)), _bits(b))
    # 22 significant bits survive: decode(split(x)) == x bit for bit
    assert np.array_equal(_bits(R.unsplit_rows_ref(b)), _bits(x))
    # with a shift: the split of x * 2^shift
    assert np.array_equal(_bits(R.split_rows_ref(x * F32(2.0 ** -16), 16)), _bits(b))


def test_lo_half_carries_information_for_almost_every_20_bit_value():
    rng = np.random.default_rng(9)
    x = (rng.integers(-(2 ** 20) + 1, 2 ** 20, (4096, 32)) * 2.0 ** -12).astype(F32)
    _, lo = R.split_halves(R.split_rows_ref(x))
    # lo' == 0 iff |n| fits 11 bits times a power of two: all 2^11 values below 2^11 and 2^10 of every binade [2^k, 2^(k+1)), k = 11..19,
    # i.e. 11 * 2^10 of 2^20 = 1.07 %.  131072 samples: the standard deviation of the fraction is 0.0003.
    assert abs((lo != 0).mean() - (1 - 11 / 1024)) < 0.002          # about 99 %: a mask or a sum that ignores lo' is wrong almost everywhere


def test_split_range_ends():
    x = np.zeros((1, 32), F32)
    # at and beyond the f16 range: 65504 is the largest f16, the tie 65520 rounds to the even 65536 = inf
    x[0, :6] = [65504.0, 65519.996, 65520.0, 1e5, -65520.0, -1e5]
    hi, lo = R.split_halves(R.split_rows_ref(x))
    assert hi[0, 0] == 65504 and lo[0, 0] == 0 and hi[0, 1] == 65504 and np.isfinite(lo[0, 1])
    assert np.array_equal(hi[0, 2:6], np.array([np.inf, np.inf, -np.inf, -np.inf], np.float16))
    assert np.array_equal(lo[0, 2:6], np.array([-np.inf, -np.inf, np.inf, np.inf], np.float16))      # (x - inf) * 2048
    # the same through a shift: |g * 2^shift| beyond the range
    hi, _ = R.split_halves(R.split_rows_ref(x * F32(2.0 ** -24), 24))
    assert np.isinf(hi[0, 2:6]).all() and np.isfinite(hi[0, :2]).all()


def test_floor_of_the_split_mask():
    a = np.zeros((1, 32), F32)
    a[0, :8] = [2.0 ** -35, 2.0 ** -36, 2.0 ** -40, 2.0 ** -149, 0.0, -0.0, 2.0 ** -30, -(2.0 ** -30)]
    b = R.split_rows_ref(a)
    hi, lo = R.split_halves(b)
    # 2^-35: hi = 0 and lo' = 2^-24, the smallest f16 subnormal: still positive
    assert hi[0, 0] == 0 and lo[0, 0] == np.float16(2.0 ** -24) and R.unsplit_rows_ref(b)[0, 0] == F32(2.0 ** -35)
    # 2^-36 (the tie between 0 and 2^-24 rounds to even) and below: all zeros
    assert not hi[0, 1:6].any() and not lo[0, 1:6].any()
    assert hi[0, 6] == 0 and lo[0, 6] == np.float16(2.0 ** -19)
    keep = R.split_positive(b)[0, :8]
    assert keep.tolist() == [True, False, False, False, False, False, True, False]
    # the fp32 mask keeps what the split drops, and -0.0 is positive for neither
    g = np.full((1, 32), 7.0, F32)
    assert (R.relu_mask_ref(g, a)[0, :8] != 0).tolist() == [True, True, True, True, False, False, True, False]
    assert np.array_equal(R.relu_mask_split_ref(g, b)[0, :8] != 0, keep)
    nan = R.split_rows_ref(np.full((1, 32), np.nan, F32))
    assert not R.split_positive(nan).any()
    out = R.relu_mask_to_split_ref(np.full((1, 32), np.inf, F32), nan, 16)
    assert not out.view(np.uint32).any()          # masked-out inf: all-zero halves


# ---- sums and the rest ----
def test_column_sum_refs():
    rng = np.random.default_rng(10)
    dy = (rng.integers(-128, 129, (513, 32)) * 2.0 ** -5).astype(F32)
    want = dy.astype(np.float64).sum(0)
    assert np.array_equal(R.colsum_ref(dy), want) and R.colsum_ref(np.zeros((0, 32), F32)).tolist() == [0.0] * 32
    s, b = R.colsum_split_ref(dy, 8)
    assert np.array_equal(s, want) and np.array_equal(_bits(b), _bits(R.split_rows_ref(dy, 8)))
    assert np.array_equal(R.colsum_of_split_ref(b, 8), want)
    assert np.array_equal(R.colsum_finish_ref(dy.reshape(27, 19, 32).sum(1)), want)


def test_deconv_grad_transpose_ref():
    rng = np.random.default_rng(11)
    g = rng.standard_normal((3, 4, 5)).astype(F32)
    t = R.deconv_grad_transpose_ref(g)
    assert t.shape == (4, 5, 3) and all(t[k, co, ci] == g[ci, k, co] for ci in range(3) for k in range(4) for co in range(5))
    base = rng.standard_normal((4, 5, 3)).astype(F32)
    assert np.array_equal(R.deconv_grad_transpose_ref(g, base), base + t)
