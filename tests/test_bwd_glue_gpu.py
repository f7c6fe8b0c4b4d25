"""The non-GEMM backward and pointwise kernels (train_bwd.hip, the column sums of wgrad.hip, pointwise.hip) against the NumPy references of
tests/bwd_glue_ref.py, on the device.

No tolerance here is measured.  Elementwise and data-movement kernels are specified with individually rounded fp32 operations: the result
is unique and the comparison is equality of the bit patterns.  Reductions get NARROW inputs -- small integers times a power of two, for
which every partial sum in every order is exact (the test checks sum |x| < 2^24 units per output from the inputs before it launches) -- and
must equal the integer sum bit for bit: a dropped or doubled row shows whatever the summation order.  On WIDE inputs (randn, 22-bit
values) their split outputs still compare bit for bit, their sums against float64 within d * 2^-24 * sum |terms|, d = the number of
additions an addend can pass through in any order.  That bound is loose by construction (a correct kernel sits orders of magnitude
inside it); it only says the wide data went through the same path, and a second identical call must reproduce the bits.

Shapes are the smallest at which each kernel can go wrong: one element, odd map edges, every channel width the column loops treat
differently, and one case just above each launch's grid cap (4096 x 256 threads of one float4 in train_bwd.hip, 2048 x 256 in
pointwise.hip) with a ragged tail."""
import numpy as np
import pytest
import torch

import bwd_glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SHIFTS = (0, 16, 24)
CAP_BWD, CAP_PW = 4096 * 256, 2048 * 256            # float4 elements one sweep of the grid covers
SPLIT_C = (32, 96, 256, 288)                        # one group, not a power of two, the model's width, a ragged second 256-column sweep
F32_C = (4, 64, 256)
MAPS = [(1, 1), (1, 7), (5, 7), (6, 8), (7, 6)]


def dev(a):
    """host array -> device tensor with the same bits (float32 and uint32 patterns both arrive as float32 tensors)"""
    a = np.ascontiguousarray(a)
    if a.dtype in (np.float32, np.uint32):
        return torch.from_numpy(a.view(np.int32)).to(DEV).view(torch.float32)
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.view(torch.int32).cpu().numpy().view(F32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.astype(F32, copy=False).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, (what, f"{bad.size} of {g.size} words differ", bad[:6].tolist(), g.reshape(-1)[bad[:6]].tolist(), w.reshape(-1)[bad[:6]].tolist())


def exact_f32(x64):
    """a float64 result that float32 holds exactly (the narrow cases)"""
    x32 = np.asarray(x64, np.float64).astype(F32)
    assert np.array_equal(x32.astype(np.float64), x64)
    return x32


def within(got, ref64, bound, what):
    err = np.abs(got.astype(np.float64) - ref64)
    print(f"{what}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max(initial=0.0)):.3g}")
    assert (err <= bound).all(), (what, float(err.max()), float(bound[err > bound].min()))


def ints(rng, lo, hi, shape, unit):
    """small integers times a power of two"""
    return (rng.integers(lo, hi + 1, shape) * unit).astype(F32)


def random_bits(rng, shape):
    """every uint32 pattern: infinities, NaN payloads and subnormals included"""
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint32)


def dyadic22(rng, shape):
    """22-bit values n * 2^-12, |n| < 2^22: the split format holds them exactly"""
    return (rng.integers(-(2 ** 22) + 1, 2 ** 22, shape) * 2.0 ** -12).astype(F32)


SPECIAL_ACT = np.array([0.0, -0.0, -1.5, 2.0 ** -149, np.nan, 2.0 ** -30, 2.0 ** -36, 0.75], F32)


def split_keep(act):
    return R.split_positive(R.split_rows_ref(act))


def mask_inputs(rng, shape, keep_fn, gscale=1.0):
    """(act, g, keep): ordinary activations with the special values spread among them -- +0.0, -0.0, a negative, the smallest subnormal,
    NaN, 2^-30 (hi = 0, lo' != 0), 2^-36 (below the split floor) -- and a gradient that holds inf / NaN / -inf under masked-out cells"""
    act = rng.standard_normal(shape, dtype=F32)
    flat = act.reshape(-1)
    m = min(flat.size, 8 * len(SPECIAL_ACT))
    flat[rng.choice(flat.size, m, replace=False)] = SPECIAL_ACT[np.arange(m) % len(SPECIAL_ACT)]
    keep = keep_fn(act)
    g = rng.standard_normal(shape, dtype=F32) * F32(gscale)
    off = np.flatnonzero(~keep.reshape(-1))
    gf = g.reshape(-1)
    gf[off[0::4]], gf[off[1::4]], gf[off[2::4]] = np.inf, np.nan, -np.inf
    assert off.size and keep.any()
    return act, g, keep


# ---- masks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4), (5, 4), (5, 64), (5, 256), (CAP_BWD + 333, 4)])
def test_relu_mask(gpu_ctx, shape):
    from ampis_amd import ops
    rng = np.random.default_rng(100 + shape[0])
    act, g, keep = mask_inputs(rng, shape, lambda a: a > 0)
    if act.size >= 64:
        assert keep.reshape(-1)[np.flatnonzero(act.reshape(-1) == F32(2.0 ** -149))].all()      # the fp32 mask keeps a subnormal
    got = host(ops.relu_mask(gpu_ctx, dev(g), dev(act)))
    same_bits(got, R.relu_mask_ref(g, act), f"relu_mask {shape}")


SPLIT_ROWS = [(1, 32), (5, 32), (5, 96), (5, 256), (5, 288), (131072 + 41, 32)]


@pytest.mark.parametrize("rows,C", SPLIT_ROWS)
def test_relu_mask_split(gpu_ctx, rows, C):
    from ampis_amd import ops
    assert rows < 100 or rows * (C // 4) > CAP_BWD
    rng = np.random.default_rng(200 + rows + C)
    act, g, keep = mask_inputs(rng, (rows, C), split_keep)
    a = act.reshape(-1)
    assert keep.reshape(-1)[a == F32(2.0 ** -30)].all() and not keep.reshape(-1)[(a == F32(2.0 ** -36)) | (a == F32(2.0 ** -149))].any()
    act_split = R.split_rows_ref(act)
    got = host(ops.relu_mask_split(gpu_ctx, dev(g), dev(act_split)))
    same_bits(got, R.relu_mask_split_ref(g, act_split), f"relu_mask_split {rows}x{C}")


@pytest.mark.parametrize("rows,C", SPLIT_ROWS)
def test_relu_mask_to_split(gpu_ctx, rows, C):
    from ampis_amd import ops
    rng = np.random.default_rng(300 + rows + C)
    for shift in (SHIFTS if rows < 100 else (16,)):
        act, g, keep = mask_inputs(rng, (rows, C), split_keep, gscale=2.0 ** -shift)
        kept = np.flatnonzero(keep.reshape(-1))
        assert kept.size >= 2
        # two kept values beyond the f16 range after the shift: the reference's +-inf halves, not a clamp and not a NaN
        g.reshape(-1)[kept[:2]] = [70000.0 * 2.0 ** -shift, -1e5 * 2.0 ** -shift]
        act_split = R.split_rows_ref(act)
        want = R.relu_mask_to_split_ref(g, act_split, shift)
        hi, lo = R.split_halves(want)
        assert hi.reshape(-1)[kept[:2]].tolist() == [np.inf, -np.inf] and lo.reshape(-1)[kept[:2]].tolist() == [-np.inf, np.inf]
        got = host(ops.relu_mask_to_split(gpu_ctx, dev(g), dev(act_split), shift))
        same_bits(got, want, f"relu_mask_to_split {rows}x{C} shift {shift}")


@pytest.mark.parametrize("rows,C", SPLIT_ROWS)
def test_accumulate_split(gpu_ctx, rows, C):
    from ampis_amd import ops
    rng = np.random.default_rng(400 + rows + C)
    for shift in (SHIFTS if rows < 100 else (24,)):
        dy_split = R.split_rows_ref(rng.standard_normal((rows, C), dtype=F32) * F32(2.0 ** -shift), shift)
        dx = rng.standard_normal((rows, C), dtype=F32) * F32(2.0 ** -shift)
        got = host(ops.accumulate_split(gpu_ctx, dev(dy_split), dev(dx), shift))
        same_bits(got, R.accumulate_split_ref(dy_split, dx, shift), f"accumulate_split {rows}x{C} shift {shift}")


# ---- stride-2 maps -------------------------------------------------------------------------------------------------------------------
def _half(n):
    return (n - 1) // 2 + 1


def _prefilled(rng, shape, scale=1.0):
    """a gradient map whose even cells hold ordinary values and whose other cells hold random bits, which must survive"""
    dx = random_bits(rng, shape).view(F32)
    dx[:, ::2, ::2] = rng.standard_normal(dx[:, ::2, ::2].shape, dtype=F32) * F32(scale)
    return dx


def _stride2_fp32(ctx, rng, B, H, W, C):
    from ampis_amd import ops
    what = f"{(B, H, W, C)}"
    x = random_bits(rng, (B, H, W, C))
    same_bits(host(ops.subsample2(ctx, dev(x))), R.subsample2_ref(x), "subsample2 " + what)
    dy = rng.standard_normal((B, _half(H), _half(W), C), dtype=F32)
    dx = _prefilled(rng, (B, H, W, C))
    same_bits(host(ops.subsample2_bwd(ctx, dev(dy), dev(dx))), R.subsample2_bwd_ref(dy, dx), "subsample2_bwd " + what)


def _scatter2(ctx, rng, B, H, W, C):
    from ampis_amd import ops
    src = random_bits(rng, (B, _half(H), _half(W), C))          # raw 16-byte chunks: NaN payloads must arrive unchanged
    up = dev(random_bits(rng, (B, H, W, C)))
    same_bits(host(ops.scatter2_rows(ctx, dev(src), H, W, out=up)), R.scatter2_rows_ref(src, H, W), f"scatter2_rows {(B, H, W, C)}")


def _stride2_split(ctx, rng, B, H, W, C, shift):
    from ampis_amd import ops
    dy_split = R.split_rows_ref(rng.standard_normal((B, _half(H), _half(W), C), dtype=F32) * F32(2.0 ** -shift), shift)
    dx = _prefilled(rng, (B, H, W, C), 2.0 ** -shift)
    got = host(ops.subsample2_bwd_split(ctx, dev(dy_split), dev(dx), shift))
    same_bits(got, R.subsample2_bwd_split_ref(dy_split, dx, shift), f"subsample2_bwd_split {(B, H, W, C)} shift {shift}")


@pytest.mark.parametrize("H,W", MAPS)
def test_stride2_maps(gpu_ctx, H, W):
    rng = np.random.default_rng(500 + 10 * H + W)
    for C in F32_C:
        _stride2_fp32(gpu_ctx, rng, 2, H, W, C)
    for C in sorted(set(F32_C + SPLIT_C)):
        _scatter2(gpu_ctx, rng, 2, H, W, C)
    for i, C in enumerate(SPLIT_C):
        _stride2_split(gpu_ctx, rng, 2, H, W, C, SHIFTS[(i + H) % 3])


def test_stride2_maps_one_element_and_grid_tails(gpu_ctx):
    rng = np.random.default_rng(599)
    _stride2_fp32(gpu_ctx, rng, 1, 1, 1, 4)
    _scatter2(gpu_ctx, rng, 1, 1, 1, 4)
    _stride2_split(gpu_ctx, rng, 1, 1, 1, 32, 16)
    # just above the caps, odd edges: 2 x 65 x 66 x 64 float4 for subsample2, 2 x 91 x 92 x 64 for the train_bwd.hip launches
    B, H, W, C = 2, 129, 131, 256
    assert CAP_PW < B * _half(H) * _half(W) * (C // 4) < CAP_PW + 2048 * 256
    x = random_bits(rng, (B, H, W, C))
    from ampis_amd import ops
    same_bits(host(ops.subsample2(gpu_ctx, dev(x))), R.subsample2_ref(x), "subsample2 above the cap")
    B, H, W, C = 2, 181, 183, 256
    assert CAP_BWD < B * _half(H) * _half(W) * (C // 4) < 2 * CAP_BWD
    _stride2_fp32(gpu_ctx, rng, B, H, W, C)
    _scatter2(gpu_ctx, rng, B, H, W, C)
    B, H, W, C = 1, 1, 2 * (131072 + 41) - 1, 32
    assert B * _half(H) * _half(W) * (C // 4) > CAP_BWD
    _stride2_split(gpu_ctx, rng, B, H, W, C, 16)


# ---- the FPN top-down sum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 64), (2, 3, 5, 256), (2, 67, 129, 256)])
def test_upsample2_bwd(gpu_ctx, shape):
    from ampis_amd import ops
    B, Hc, Wc, C = shape
    fine = (B, 2 * Hc, 2 * Wc, C)
    assert Hc < 10 or CAP_BWD < B * Hc * Wc * (C // 4) < 2 * CAP_BWD
    rng = np.random.default_rng(600 + Hc + C)
    nan = np.full(shape, np.nan, F32)

    def run(dfine, dcoarse, init=False):
        return host(ops.upsample2_bwd(gpu_ctx, dev(dfine), dev(dcoarse), init=init))

    # narrow: integers / 64 -- five terms of at most 64 units each
    dfine, dcoarse = ints(rng, -64, 64, fine, 2.0 ** -6), ints(rng, -64, 64, shape, 2.0 ** -6)
    sums, mags = R.upsample2_bwd_ref(dfine), R.upsample2_bwd_abs_ref(dfine)
    assert ((mags + np.abs(dcoarse)) * 64 < 2 ** 24).all()
    same_bits(run(dfine, dcoarse), exact_f32(sums + dcoarse), f"upsample2_bwd narrow {shape}")
    same_bits(run(dfine, nan, init=True), exact_f32(sums), f"upsample2_bwd_init narrow {shape}")
    # wide: an addend passes through at most 4 additions ((v00 + v01) + (v10 + v11), + dcoarse, in any order of the five)
    dfine, dcoarse = rng.standard_normal(fine, dtype=F32), rng.standard_normal(shape, dtype=F32)
    sums, mags = R.upsample2_bwd_ref(dfine), R.upsample2_bwd_abs_ref(dfine)
    got = run(dfine, dcoarse)
    within(got, sums + dcoarse, 4 * 2.0 ** -24 * (mags + np.abs(dcoarse)), f"upsample2_bwd wide {shape}")
    same_bits(run(dfine, dcoarse), got, "upsample2_bwd: a second call")
    got0 = run(dfine, np.zeros(shape, F32))
    within(got0, sums, 4 * 2.0 ** -24 * mags, f"upsample2_bwd wide on zeros {shape}")
    # the init entry never reads dcoarse and leaves what the += entry leaves in a zero-filled map, bit for bit
    same_bits(run(dfine, nan, init=True), got0, f"upsample2_bwd_init {shape}")


# ---- the small-K data gradient -------------------------------------------------------------------------------------------------------
SMALL_K = [(1, 4, 32, 1), (2, 4, 256, 784), (15, 16, 256, 700), (16, 16, 256, 513), (5, 8, 96, 1030), (3, 12, 288, 511), (15, 16, 256, 16889)]


def _small_k_act(rng, npix, C):
    """fp32 activations with the special values, their split rows, and the two masks"""
    act = rng.standard_normal((npix, C), dtype=F32)
    flat = act.reshape(-1)
    m = min(flat.size, 8 * len(SPECIAL_ACT))
    flat[rng.choice(flat.size, m, replace=False)] = SPECIAL_ACT[np.arange(m) % len(SPECIAL_ACT)]
    act_split = R.split_rows_ref(act)
    with np.errstate(invalid="ignore"):
        return act, act_split, act > 0, R.split_positive(act_split)


def _variants(ld):
    v = [("split_ld", dict(act_split=True)), ("split_f32act", dict(act_split=False))]
    return v + [("split", dict(act_split=True, rows16=True))] if ld == 16 else v


@pytest.mark.parametrize("case", range(len(SMALL_K)))
def test_small_k_dgrad_narrow(gpu_ctx, case):
    """Integer data: the products, the sums over k and the column sums are exact in every order, so a dropped or doubled row or slice shows
    in the bias sums bit for bit."""
    from ampis_amd import ops
    K, ld, C, npix = SMALL_K[case]
    shift = SHIFTS[case % 3]
    rng = np.random.default_rng(700 + case)
    unit = 2.0 ** -(4 + shift)
    dl = ints(rng, -4, 4, (npix, ld), 2.0 ** -(2 + shift))          # the pad columns k >= K hold finite values as well
    w = ints(rng, -4, 4, (K, C), 0.25)
    act, act_split, keep32, keeps = _small_k_act(rng, npix, C)
    assert ((np.abs(dl[:, :K]).astype(np.float64) @ np.abs(w).astype(np.float64)).sum(0) / unit).max() + 4096 < 2 ** 24
    raw = R.small_k_dgrad_ref(dl, K, w)
    same_bits(host(ops.small_k_dgrad(gpu_ctx, dev(dl), dev(w), dev(act))), R.small_k_dgrad_ref(dl, K, w, keep32, raw), f"small_k_dgrad {SMALL_K[case]}")
    same_bits(host(ops.small_k_dgrad(gpu_ctx, dev(dl), dev(w))), raw, f"small_k_dgrad without act {SMALL_K[case]}")
    base = ints(rng, -4096, 4096, (C,), unit)
    for name, kw in _variants(ld):
        what = f"small_k_dgrad_{name} {SMALL_K[case]} shift {shift}"
        a, keep = (act_split, keeps) if kw["act_split"] else (act, keep32)
        want_dx, want_sum = R.small_k_dgrad_split_ref(dl, K, w, keep, shift, raw)
        # accumulate = 0: colsum_out is written, not read
        dx, cs = ops.small_k_dgrad_split(gpu_ctx, dev(dl), dev(w), dev(a), shift, colsum_out=dev(np.full(C, np.nan, F32)), **kw)
        same_bits(host(dx), want_dx, what + ": dx_split")
        same_bits(host(cs), exact_f32(want_sum), what + ": bias sums")
        dx, cs = ops.small_k_dgrad_split(gpu_ctx, dev(dl), dev(w), dev(a), shift, colsum_out=dev(base), accumulate=True, **kw)
        same_bits(host(dx), want_dx, what + ": dx_split (accumulate)")
        same_bits(host(cs), exact_f32(want_sum + base), what + ": bias sums (accumulate)")


@pytest.mark.parametrize("case", range(len(SMALL_K)))
def test_small_k_dgrad_wide(gpu_ctx, case):
    from ampis_amd import ops
    K, ld, C, npix = SMALL_K[case]
    shift = SHIFTS[(case + 1) % 3]
    rng = np.random.default_rng(800 + case)
    dl = rng.standard_normal((npix, ld), dtype=F32) * F32(2.0 ** -shift)
    w = rng.standard_normal((K, C), dtype=F32)
    act, act_split, keep32, keeps = _small_k_act(rng, npix, C)
    raw = R.small_k_dgrad_ref(dl, K, w)
    for name, kw in _variants(ld):
        what = f"small_k_dgrad_{name} {SMALL_K[case]} shift {shift}"
        a, keep = (act_split, keeps) if kw["act_split"] else (act, keep32)
        dx_ref = R.small_k_dgrad_ref(dl, K, w, keep, raw)
        want_dx, want_sum = R.small_k_dgrad_split_ref(dl, K, w, keep, shift, raw)
        dx, cs = ops.small_k_dgrad_split(gpu_ctx, dev(dl), dev(w), dev(a), shift, **kw)
        dx, cs = host(dx), host(cs)
        same_bits(dx, want_dx, what + ": dx_split")
        # "the same sums in the same order" as amp_small_k_dgrad: its value under the same mask, scaled and split
        plain = host(ops.small_k_dgrad(gpu_ctx, dev(dl), dev(w), dev(R.unsplit_rows_ref(act_split) if kw["act_split"] else act)))
        same_bits(dx, R.split_rows_ref(plain, shift), what + ": against amp_small_k_dgrad")
        # a column of npix rows: an addend passes through at most npix additions (loose by construction)
        within(cs, want_sum, npix * 2.0 ** -24 * np.abs(dx_ref).astype(np.float64).sum(0), what + ": bias sums")
        dx2, cs2 = ops.small_k_dgrad_split(gpu_ctx, dev(dl), dev(w), dev(a), shift, **kw)
        same_bits(host(dx2), dx, what + ": dx_split, a second call")
        same_bits(host(cs2), cs, what + ": bias sums, a second call")
        if not kw["act_split"] and K < ld:
            # _f32act does not read the values of the pad columns: NaN there changes nothing
            dl_nan = dl.copy()
            dl_nan[:, K:] = np.nan
            dx3, cs3 = ops.small_k_dgrad_split(gpu_ctx, dev(dl_nan), dev(w), dev(a), shift, **kw)
            dx3, cs3 = host(dx3), host(cs3)
            assert np.isfinite(R.unsplit_rows_ref(dx3)).all() and np.isfinite(cs3).all(), what
            same_bits(dx3, dx, what + ": NaN in the pad columns")
            same_bits(cs3, cs, what + ": NaN in the pad columns, bias sums")


def test_small_k_dgrad_many_classes_and_no_mask(gpu_ctx):
    from ampis_amd import ops
    K, ld, C, npix = 80, 80, 256, 100
    rng = np.random.default_rng(880)
    dl, w = rng.standard_normal((npix, ld), dtype=F32), rng.standard_normal((K, C), dtype=F32)
    act, _, keep32, _ = _small_k_act(rng, npix, C)
    same_bits(host(ops.small_k_dgrad(gpu_ctx, dev(dl), dev(w))), R.small_k_dgrad_ref(dl, K, w), "small_k_dgrad K = 80, act = NULL")
    same_bits(host(ops.small_k_dgrad(gpu_ctx, dev(dl), dev(w), dev(act))), R.small_k_dgrad_ref(dl, K, w, keep32), "small_k_dgrad K = 80")
    # K < ld with fp32 rows of 80: the columns k >= K are not read
    dl[:, 77:] = np.nan
    same_bits(host(ops.small_k_dgrad(gpu_ctx, dev(dl), dev(w[:77].copy()), dev(act))), R.small_k_dgrad_ref(dl, 77, w[:77], keep32), "small_k_dgrad K = 77 of 80")


# ---- column sums ---------------------------------------------------------------------------------------------------------------------
COLSUM = [(0, 32), (1, 4), (513, 12), (10000, 16), (700, 1028), (16889, 32)]
COLSUM_SPLIT = [(0, 32), (1, 32), (513, 96), (1030, 256), (700, 288), (16889, 32)]


def _colsum_narrow(rng, M, N, shift=0):
    dy = ints(rng, -128, 128, (M, N), 2.0 ** -(5 + shift))
    base = ints(rng, -4096, 4096, (N,), 2.0 ** -(5 + shift))
    base[base == 0] = F32(2.0 ** -(5 + shift))          # no zero: out + (+0) keeps out only when out is not -0
    assert M * 128 + 4096 < 2 ** 24
    return dy, base


@pytest.mark.parametrize("M,N", COLSUM)
def test_colsum(gpu_ctx, M, N):
    from ampis_amd import ops
    rng = np.random.default_rng(900 + M + N)
    dy, base = _colsum_narrow(rng, M, N)
    want = R.colsum_ref(dy)
    same_bits(host(ops.colsum(gpu_ctx, dev(dy), out=dev(np.full(N, np.nan, F32)))), exact_f32(want), f"colsum narrow {M}x{N}")
    same_bits(host(ops.colsum(gpu_ctx, dev(dy), out=dev(base), accumulate=True)), exact_f32(want + base), f"colsum narrow accumulate {M}x{N}")
    if M == 0:
        assert not want.any()
        return
    dy = rng.standard_normal((M, N), dtype=F32)
    got = host(ops.colsum(gpu_ctx, dev(dy)))
    within(got, R.colsum_ref(dy), M * 2.0 ** -24 * np.abs(dy).astype(np.float64).sum(0), f"colsum wide {M}x{N}")
    same_bits(host(ops.colsum(gpu_ctx, dev(dy))), got, "colsum: a second call")


@pytest.mark.parametrize("case", range(len(COLSUM_SPLIT)))
def test_colsum_split_and_of_split(gpu_ctx, case):
    from ampis_amd import ops
    M, N = COLSUM_SPLIT[case]
    shift = SHIFTS[case % 3]
    rng = np.random.default_rng(1000 + case)
    dy, base = _colsum_narrow(rng, M, N, shift)          # at most 4 * 2^-shift: inside the f16 range after the shift, 8 significant bits
    want, want_split = R.colsum_split_ref(dy, shift)
    what = f"{M}x{N} shift {shift}"
    out, sp = ops.colsum_split(gpu_ctx, dev(dy), shift, out=dev(np.full(N, np.nan, F32)))
    same_bits(host(out), exact_f32(want), "colsum_split narrow " + what)
    same_bits(host(sp), want_split, "colsum_split narrow: dy_split " + what)
    out, _ = ops.colsum_split(gpu_ctx, dev(dy), shift, out=dev(base), accumulate=True)
    same_bits(host(out), exact_f32(want + base), "colsum_split narrow accumulate " + what)
    assert np.array_equal(R.colsum_of_split_ref(want_split, shift), want)
    same_bits(host(ops.colsum_of_split(gpu_ctx, dev(want_split), shift, out=dev(np.full(N, np.nan, F32)))), exact_f32(want), "colsum_of_split narrow " + what)
    same_bits(host(ops.colsum_of_split(gpu_ctx, dev(want_split), shift, out=dev(base), accumulate=True)), exact_f32(want + base),
              "colsum_of_split narrow accumulate " + what)
    if M == 0:
        return
    # wide: 22-bit values (the split holds them exactly, so both kernels sum the same numbers) and randn
    for kind, dy in (("22-bit", dyadic22(rng, (M, N)) * F32(2.0 ** -(10 + shift))), ("randn", rng.standard_normal((M, N), dtype=F32) * F32(2.0 ** -shift))):
        want, want_split = R.colsum_split_ref(dy, shift)
        bound = M * 2.0 ** -24 * np.abs(dy).astype(np.float64).sum(0)
        out, sp = ops.colsum_split(gpu_ctx, dev(dy), shift)
        out, sp = host(out), host(sp)
        same_bits(sp, want_split, f"colsum_split {kind}: dy_split " + what)
        within(out, want, bound, f"colsum_split {kind} " + what)
        out2, sp2 = ops.colsum_split(gpu_ctx, dev(dy), shift)
        same_bits(host(out2), out, "colsum_split: a second call")
        same_bits(host(sp2), sp, "colsum_split: dy_split, a second call")
        held = R.unsplit_rows_ref(want_split).astype(np.float64) * 2.0 ** -shift
        if kind == "22-bit":
            assert np.array_equal(held, dy.astype(np.float64))
        got = host(ops.colsum_of_split(gpu_ctx, dev(want_split), shift))
        within(got, R.colsum_of_split_ref(want_split, shift), M * 2.0 ** -24 * np.abs(held).sum(0), f"colsum_of_split {kind} " + what)
        same_bits(host(ops.colsum_of_split(gpu_ctx, dev(want_split), shift)), got, "colsum_of_split: a second call")


@pytest.mark.parametrize("parts", [1, 8, 9, 33])
def test_colsum_finish(gpu_ctx, parts):
    from ampis_amd import ops
    rng = np.random.default_rng(1100 + parts)
    for N in (4, 12, 32, 288, 1028):
        part, base = _colsum_narrow(rng, parts, N)
        want = R.colsum_finish_ref(part)
        same_bits(host(ops.colsum_finish(gpu_ctx, dev(part), out=dev(np.full(N, np.nan, F32)))), exact_f32(want), f"colsum_finish narrow {parts}x{N}")
        same_bits(host(ops.colsum_finish(gpu_ctx, dev(part), out=dev(base), accumulate=True)), exact_f32(want + base), f"colsum_finish accumulate {parts}x{N}")
        part = rng.standard_normal((parts, N), dtype=F32)
        got = host(ops.colsum_finish(gpu_ctx, dev(part)))
        within(got, R.colsum_finish_ref(part), parts * 2.0 ** -24 * np.abs(part).astype(np.float64).sum(0), f"colsum_finish wide {parts}x{N}")
        same_bits(host(ops.colsum_finish(gpu_ctx, dev(part))), got, "colsum_finish: a second call")


# ---- transpose, SGD, and the backbone's pointwise kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,T,C2", [(256, 4, 256), (3, 4, 5)])
def test_deconv_grad_transpose(gpu_ctx, Cin, T, C2):
    from ampis_amd import ops
    rng = np.random.default_rng(1200 + Cin)
    g = rng.standard_normal((Cin, T, C2), dtype=F32)
    base = rng.standard_normal((T, C2, Cin), dtype=F32)
    same_bits(host(ops.deconv_grad_transpose(gpu_ctx, dev(g), out=dev(np.full((T, C2, Cin), np.nan, F32)))), R.deconv_grad_transpose_ref(g), "deconv_grad_transpose")
    same_bits(host(ops.deconv_grad_transpose(gpu_ctx, dev(g), out=dev(base), accumulate=True)), R.deconv_grad_transpose_ref(g, base),
              "deconv_grad_transpose accumulate")


@pytest.mark.parametrize("n", [1, 1000, CAP_BWD + 5])
def test_sgd_update(gpu_ctx, n):
    from ampis_amd import ops
    rng = np.random.default_rng(1300 + n % 97)
    p, g, v = (rng.standard_normal(n, dtype=F32) for _ in range(3))
    lr, mu, wd, gs = 0.02, 0.9, 1e-4, 1.0 / 3.0
    pd, vd = dev(p), dev(v)
    ops.sgd_update(gpu_ctx, pd, dev(g), vd, lr, mu, wd, gs)
    want_p, want_v = R.sgd_update_ref(p, g, v, lr, mu, wd, gs)
    same_bits(host(vd), want_v, f"sgd_update v, n = {n}")
    same_bits(host(pd), want_p, f"sgd_update p, n = {n}")


MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)


@pytest.mark.parametrize("B,H,W,Hp,Wp,hw", [(1, 1, 1, 1, 1, None), (2, 5, 7, 8, 12, None), (2, 5, 7, 8, 12, [[5, 7], [3, 4]]),
                                            (2, 515, 511, 520, 512, [[515, 511], [300, 257]])])
def test_preprocess(gpu_ctx, B, H, W, Hp, Wp, hw):
    from ampis_amd import ops
    assert H < 10 or CAP_PW < B * Hp * Wp < 2 * CAP_PW
    rng = np.random.default_rng(1400 + H)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    hw = None if hw is None else np.array(hw, np.int32)
    got = host(ops.preprocess(gpu_ctx, dev(img), Hp, Wp, MEAN, STD, None if hw is None else dev(hw)))
    want = R.preprocess_ref(img, Hp, Wp, MEAN, STD, hw)
    assert hw is None or not want[1, hw[1, 0]:].any() and want[1, :hw[1, 0], :hw[1, 1], :3].all()
    same_bits(got, want, f"preprocess {(B, H, W, Hp, Wp)}")


@pytest.mark.parametrize("B,H,W,Cs", [(1, 1, 1, (4,)), (2, 7, 9, F32_C), (2, 8, 6, F32_C), (2, 129, 131, (256,))])
def test_maxpool3x3s2(gpu_ctx, B, H, W, Cs):
    from ampis_amd import ops
    rng = np.random.default_rng(1500 + H)
    for C in Cs:
        assert H < 10 or CAP_PW < B * _half(H) * _half(W) * (C // 4) < 2 * CAP_PW
        x = rng.standard_normal((B, H, W, C), dtype=F32)
        x[..., 1] = -np.abs(x[..., 1]) - 1.0          # one channel negative everywhere: the padding must act as -inf, 0 would win at the borders
        want = R.maxpool3x3s2_ref(x)
        assert (want[..., 1] < 0).all()
        same_bits(host(ops.maxpool3x3s2(gpu_ctx, dev(x))), want, f"maxpool3x3s2 {(B, H, W, C)}")
