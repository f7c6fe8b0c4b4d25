"""The range guard of the split arithmetic (AMP_CONV_F16X3), kernel by kernel: a call never returns a wrong answer with a clear flag.

Every launch family of conv_run that multiplies split operands is given ONE operand element beyond the fp16 range -- at the positions of
tests/range_guard_cases.py, each shown on the CPU to be read by a valid output -- and must raise the context's range flag; with an
element of +-65504, the largest fp16 value, the flag stays clear and the result equals the float64 reference bit for bit.  The same for
the epilogues that WRITE split rows (an output past 65520 is stored with a non-finite half, never saturated, and raises the flag in its
consumer), the fused epilogues amp_debug_conv_run cannot reach, and the weight-gradient kernels.  No assertion has a tolerance, and no
kernel indexes memory by the poisoned data."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_exact_ref as R                      # noqa: E402
import range_guard_cases as G                   # noqa: E402
import test_conv_exact_gpu as E                 # noqa: E402
import test_wgrad_exact_gpu as WG               # noqa: E402

pytestmark = pytest.mark.gpu


# ---- one element of a device tensor replaced, and put back from an untouched copy -----------------------------------------------------------
def split_slot(ch):
    """the positions of (hi, lo') of channel / k index ch inside a row of split halves"""
    return (ch // 32) * 64 + ch % 32, (ch // 32) * 64 + ch % 32 + 32


class Poke:
    """t: a device tensor whose last dimension is channels (fp32 values, or fp32 containers of split halves); t0: its untouched copy"""

    def __init__(self, t, split):
        import torch
        self.split = bool(split)
        self.t = t.view(torch.float16) if split else t
        self.t0 = self.t.clone()

    def values(self):
        return G.SPLIT_POISONS if self.split else G.FP32_POISONS

    def put(self, idx, v):
        *row, ch = idx
        row = tuple(row)
        if self.split:
            i_hi, i_lo = split_slot(ch)
            self.t[row + (i_hi,)] = float(v[0])
            self.t[row + (i_lo,)] = float(v[1])
        else:
            self.t[row + (ch,)] = float(v)

    def restore(self, idx):
        *row, ch = idx
        row = tuple(row)
        for i in (split_slot(ch) if self.split else (ch,)):
            self.t[row + (i,)] = self.t0[row + (i,)]

    def untouched(self):
        import torch
        return torch.equal(self.t.view(torch.int16 if self.split else torch.int32), self.t0.view(torch.int16 if self.split else torch.int32))


def bands_dirty(buf, g):
    n = buf.numel() - 2 * g
    return int((buf[:g] != E.SENTINEL).sum() + (buf[g + n:] != E.SENTINEL).sum())


def say(v):
    return f"(hi {float(v[0])}, lo' {float(v[1])})" if isinstance(v, tuple) else repr(v)


# ---- 2a. every split convolution launch raises the flag ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GUARD_CASES, ids=G.GUARD_IDS)
def test_poisoned_operand_raises_the_flag(gpu_ctx, c):
    inputs, kernel = E.planned(c)
    d = E.operands(c, "I")
    t = E.upload(c, d, kernel)
    assert len(t["w_forms"]) == 2
    buf, y, g = E.guarded(E.y_shape(c), zero_fill=c["out_mode"] == 2)
    px = Poke(t["x"], c["fmt"] & E.X_SPLIT)
    pw = Poke(t["w"], False)
    w_split = t["w_forms"][1][1]
    pws = Poke(w_split.view(c["Cout"], -1), True)
    taps_w = t["w"].shape[3]                       # channels per tap of the array the device holds (64 in the window layout of a grouped case)
    missed, launches = [], 0
    for why, op, idx in G.poisons(c):
        for form, ws in t["w_forms"]:
            if op == "x":
                poke, at = px, idx
            elif ws is None:                      # the fp32 weights conv_run splits per call
                poke, at = pw, G.w_window_index(c, idx)
            else:                                 # the rows split beforehand: [Cout][K], k = (ky, kx, slot)
                n, ky, kx, slot = G.w_window_index(c, idx)
                poke, at = pws, (n, (ky * c["KW"] + kx) * taps_w + slot)
            for v in poke.values():
                poke.put(at, v)
                gpu_ctx.conv_range_flag()                                   # read and clear
                E.launch(gpu_ctx, c, inputs, t, ws, y)
                launches += 1
                raised, again = gpu_ctx.conv_range_flag(), gpu_ctx.conv_range_flag()
                poke.restore(at)
                assert not again, "the flag must read clear after it was read and cleared"
                assert bands_dirty(buf, g) == 0, f"{c['name']} [{why}] {say(v)}, {form}: words written outside y"
                if not raised:
                    missed.append(f"[{why}] {say(v)}, {form}")
    assert px.untouched() and pw.untouched() and pws.untouched()
    assert not missed, f"{c['name']} ({c['kernel']}, epilogue {c['epi']}): {len(missed)} of {launches} poisoned launches left the flag clear: " + "; ".join(missed[:8])
    # and the operands are back: an unpoisoned launch leaves it clear
    E.launch(gpu_ctx, c, inputs, t, None, y)
    assert not gpu_ctx.conv_range_flag()


# ---- 2b. the in-range edge: +-65504 is an operand like any other ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.EDGE_CASES, ids=[c["name"] for c in G.EDGE_CASES])
def test_largest_fp16_operand_is_exact_and_leaves_the_flag_clear(gpu_ctx, c):
    d, _ = G.edge_operands(c)
    E.run_case(gpu_ctx, c, "I", d)          # both weight forms against the float64 reference, the sentinel bands, and the flag clear at the end


@pytest.mark.parametrize("c", G.F32_FROM_F16X3_CTX, ids=[c["name"] for c in G.F32_FROM_F16X3_CTX])
def test_fp32_kernels_of_an_f16x3_context_have_no_range(gpu_ctx, c):
    """MFMA_64 (Cin % 32 != 0) and a forced fp32 launch: an element of 7e4 is an fp32 value like any other"""
    d = dict(E.operands(c, "I"))
    x = d["x"].copy()
    (_, p0), (_, p1) = G.x_positions(c)[0], G.x_positions(c)[-1]
    x[p0], x[p1] = 7e4, -7e4
    d["x"] = x
    assert c["kernel"] in ("MFMA_64", "GLDS_64")
    E.run_case(gpu_ctx, c, "I", d)


# ---- 2c. the producers of split rows ----------------------------------------------------------------------------------------------------------
# one case per epilogue that writes split rows: (case, how one output is carried past 65520)
PRODUCERS = [
    ("f16x3s_64", "res"),              # conv_epilogue_rows8 (LDS-staged, 8 channels per lane): a residual element of 65504 on top of a sum >= 16
    ("f16x3s_64_p0_mask", "shift"),    # conv_epilogue_rows with a split y (the output mask takes the other LDS-staged epilogue)
    ("f16x3s_128", "shift"),
    ("split_128x256", "shift"),        # conv_epilogue_direct_rows: the ring kernels
    ("split_256x128", "shift"),
    ("split_tall64", "shift"),
    ("nloop", "shift"),
    ("nloop_scatter", "shift"),
    ("c64_patch", "shift"),
    ("c64_patch_diag_cpg8", "shift"),
    ("patch256", "shift"),
]


def producer_operands(c, how):
    """the class I operands with one shift value (a whole output column) or one residual element changed so that outputs leave the fp16 range
    while every accumulator stays small; returns (operands, expected values, bool array of the outputs beyond the range)"""
    d = dict(E.operands(c, "I"))
    base = E.reference(c, "I", d)                                   # exact, every assertion of the reference on
    rng = np.random.default_rng(17)
    if how == "shift":
        n0 = int(rng.integers(c["Cout"]))
        sh = d["shift"].copy()
        sh[n0] = 70000.0 if (c["relu"] or n0 % 2) else -70000.0
        d["shift"] = sh
    else:
        assert c["res_mode"] == 1 and c["out_mode"] == 0
        cand = np.argwhere(base - d["res"] >= 16)                      # the sum after scale and shift is >= 16 there: + 65504 is past 65520
        assert len(cand)
        at = tuple(cand[int(rng.integers(len(cand)))])
        res = d["res"].copy()
        res[at] = G.F16_MAX
        d["res"] = res
    with np.errstate(invalid="ignore", over="ignore"):
        want = E.reference(c, "I", d, check=False)
    over = np.abs(want) >= 65520.0
    assert over.any() and np.isfinite(want).all()
    assert np.array_equal(want[~over], base[~over]), "the change must not reach any other output"
    return d, want, over


@pytest.mark.parametrize("name,how", PRODUCERS, ids=[p[0] for p in PRODUCERS])
def test_producer_stores_a_non_finite_half_and_its_consumer_raises_the_flag(gpu_ctx, name, how):
    import torch
    from ampis_amd._lib import ConvDesc, check, ptr
    from bwd_glue_ref import split_halves
    c = next(q for q in G.GUARD_CASES if q["name"] == name)
    assert c["fmt"] & E.Y_SPLIT
    inputs, kernel = E.planned(c)
    d, want, over = producer_operands(c, how)
    t = E.upload(c, d, kernel)
    want_bits = R.split_rows_ref(want).view(np.int32)
    for form, ws in t["w_forms"]:
        buf, y, g = E.guarded(want.shape, zero_fill=c["out_mode"] == 2)
        gpu_ctx.conv_range_flag()
        E.launch(gpu_ctx, c, inputs, t, ws, y)
        gpu_ctx.conv_range_flag()          # what the producer does with the flag is its own business: the accumulators are in range
        assert bands_dirty(buf, g) == 0
        got = y.cpu().numpy()
        hi, lo = split_halves(got)
        # beyond the range: a non-finite half, never a finite saturated pair
        sat = over & np.isfinite(hi) & np.isfinite(lo)
        assert not sat.any(), f"{name}, {form}: {int(sat.sum())} of {int(over.sum())} outputs beyond the range were stored as finite halves (first hi {hi[sat][0]}, lo' {lo[sat][0]})"
        # everything else bit for bit: compare the halves themselves where the output is in range
        whi, wlo = split_halves(want_bits.view(np.float32))
        same = (hi.view(np.int16) == whi.view(np.int16)) & (lo.view(np.int16) == wlo.view(np.int16))
        assert same[~over].all(), f"{name}, {form}: {int((~same[~over]).sum())} in-range outputs differ from the reference"
        # the consumer: a 1x1 convolution reading y as split rows
        B, Ho, Wo, Cy = want.shape
        rng = np.random.default_rng(3)
        w2 = torch.from_numpy(R.class_i(rng, (64, 1, 1, Cy))).to("cuda:0")
        y2 = torch.empty(B, Ho, Wo, 64, device="cuda:0")
        desc = ConvDesc(B, Ho, Wo, Cy, 64, 1, 1, 1, 0, 0, 0, 0)
        check(E._lib().amp_debug_conv_run(gpu_ctx.handle, C.byref(desc), 1, ptr(y), ptr(w2), None, None, None, None, None, ptr(y2), 0, E.X_SPLIT, 0), "amp_debug_conv_run")
        torch.cuda.synchronize()
        assert gpu_ctx.conv_range_flag(), f"{name}, {form}: the consumer of the producer's rows left the flag clear"
        assert not gpu_ctx.conv_range_flag()


# ---- 2d. the fused epilogues ------------------------------------------------------------------------------------------------------------------
def _pow2_past_range(peak):
    """k with peak * 2^k in [2^17, 2^18): beyond 65520 by a factor of two at the least"""
    k = 17 - int(np.floor(np.log2(float(peak))))
    assert 2.0 ** 17 <= float(peak) * 2.0 ** k < 2.0 ** 18
    return k


def test_fused_rpn_head_raises_the_flag(gpu_ctx):
    """amp_rpn_head_fused: the 3x3 convolution's hidden tensor is split in the epilogue and multiplied again, and never written.  A poisoned
    x raises the flag; so does a hidden activation past 65520 whose accumulators are finite (weights and bias times a power of two)."""
    import torch
    from ampis_amd import ops, _lib
    g = torch.Generator().manual_seed(21)
    B, H, W = 2, 112, 120
    x = torch.randn(B, H, W, 256, generator=g).clamp_(min=0).to("cuda:0")
    wc = (torch.randn(256, 3, 3, 256, generator=g) * 0.02).to("cuda:0")
    bc = (torch.randn(256, generator=g) * 0.1).to("cuda:0")
    wp = torch.zeros(16, 1, 1, 256); wp[:15] = torch.randn(15, 1, 1, 256, generator=g) * 0.05
    bp = torch.zeros(16); bp[:15] = torch.randn(15, generator=g) * 0.1
    wp_d, bp_d = wp.to("cuda:0"), bp.to("cuda:0")
    xs = ops.split_rows(gpu_ctx, x)
    pred = torch.empty(B * H * W, 16, device="cuda:0")

    def run(w, b):
        gpu_ctx.conv_range_flag()
        _lib.check(_lib.lib().amp_rpn_head_fused(gpu_ctx.handle, _lib.ptr(xs), B, H, W, _lib.ptr(w), _lib.ptr(b), _lib.ptr(wp_d), _lib.ptr(bp_d), _lib.ptr(pred)),
                   "amp_rpn_head_fused")
        torch.cuda.synchronize()
        raised = gpu_ctx.conv_range_flag()
        assert not gpu_ctx.conv_range_flag()
        return raised

    assert not run(wc, bc) and bool(torch.isfinite(pred).all())
    poke = Poke(xs, True)
    for at in ((0, 0, 0, 0), (B - 1, H - 1, W - 1, 255), (1, 57, 61, 100)):      # read by row 0, by the last row of the ragged last tile, in between
        for v in G.SPLIT_POISONS:
            poke.put(at, v)
            raised = run(wc, bc)
            poke.restore(at)
            assert raised, f"x{at} = {say(v)}: the flag stayed clear"
    assert poke.untouched()
    # the hidden activation: finite accumulators, FrozenBN + ReLU past the range
    hidden = ops.conv2d_nhwc(gpu_ctx, x, wc, None, bc, pad=1, relu=True)
    k = _pow2_past_range(hidden.max().item())
    wk, bk = wc * 2.0 ** k, bc * 2.0 ** k
    assert float(wk.abs().max()) < 60000.0                                  # the weights themselves stay inside the range
    assert not gpu_ctx.conv_range_flag()
    assert run(wk, bk), "a hidden activation beyond the fp16 range reached the predictor product with the flag clear"
    assert not run(wc, bc)


def test_fused_mask_tail_raises_the_flag_or_is_right(gpu_ctx):
    """amp_mask_deconv_predict: a poisoned x raises the flag.  Its hidden activation is NOT split again -- the predictor row is an fp32 dot
    product in the epilogue -- so past 65520 the call may leave the flag clear, and then the probabilities must be right."""
    import torch
    from ampis_amd import _lib, ops
    g = torch.Generator().manual_seed(12)
    N, K = 37, 3
    x = (torch.randn(N, 14, 14, 256, generator=g).clamp_(min=0) * 2).to("cuda:0")
    wd = torch.randn(256, 256, 2, 2, generator=g) * 0.05
    bd = torch.randn(256, generator=g) * 0.1
    wp = torch.randn(K, 256, generator=g) * 0.05
    bp = torch.randn(K, generator=g) * 0.1
    cls = torch.randint(0, K, (N,), generator=g).int()
    xs = ops.split_rows(gpu_ctx, x)
    prob = torch.empty(N, 28, 28, device="cuda:0")
    wp_d, bp_d, cls_d = wp.to("cuda:0"), bp.to("cuda:0"), cls.to("cuda:0")

    def run(wd_, bd_):
        w_lib = wd_.permute(2, 3, 1, 0).reshape(1024, 1, 1, 256).contiguous().to("cuda:0")
        b_lib = bd_.repeat(4).contiguous().to("cuda:0")
        gpu_ctx.conv_range_flag()
        _lib.check(_lib.lib().amp_mask_deconv_predict(gpu_ctx.handle, _lib.ptr(xs), N, _lib.ptr(w_lib), _lib.ptr(b_lib), _lib.ptr(wp_d), _lib.ptr(bp_d), _lib.ptr(cls_d), K,
                                                      _lib.ptr(prob)), "amp_mask_deconv_predict")
        torch.cuda.synchronize()
        raised = gpu_ctx.conv_range_flag()
        assert not gpu_ctx.conv_range_flag()
        return raised

    assert not run(wd, bd)
    poke = Poke(xs, True)
    for at in ((0, 0, 0, 0), (N - 1, 13, 13, 255), (19, 6, 9, 77)):
        for v in G.SPLIT_POISONS:
            poke.put(at, v)
            raised = run(wd, bd)
            poke.restore(at)
            assert raised, f"x{at} = {say(v)}: the flag stayed clear"
    assert poke.untouched()
    hid = torch.nn.functional.conv_transpose2d(x.cpu().double().permute(0, 3, 1, 2), wd.double(), bd.double(), stride=2).relu()
    k = _pow2_past_range(hid.max().item())
    wk, bk = wd * 2.0 ** k, bd * 2.0 ** k
    assert float(wk.abs().max()) < 60000.0
    if not run(wk, bk):
        # no tolerance: where the fp64 logit is beyond +-256 the fp32 sigmoid is exactly 0 or 1 whatever the rounding of the sums (e^-104 is
        # below the smallest fp32 subnormal, and a relative error of the logit below one half cannot bring it there); a hidden value turned
        # into inf would give inf - inf = NaN under a predictor row of mixed signs
        ref = torch.einsum("nchw,nc->nhw", hid * 2.0 ** k, wp.double()[cls.long()]) + bp.double()[cls.long()].view(-1, 1, 1)
        got = prob.cpu()
        assert bool(torch.isfinite(got).all()), "flag clear and non-finite probabilities"
        sure = ref.abs() > 256
        assert sure.double().mean().item() > 0.9
        assert torch.equal(got[sure], (ref[sure] > 0).float()), "flag clear and saturated probabilities on the wrong side"


# ---- 2e. weight gradients ---------------------------------------------------------------------------------------------------------------------
WGRAD_SHAPES = ("3x3_m99", "3x3_m3465", "1x1s2_m2310", "2x2s2_m1150", "1x1_noring_m117")      # single slab, several slabs per geometry, the no-ring shape
WGRAD_EDGE_SHAPES = ("3x3_m99", "1x1s2_m63", "2x2s2_m63", "1x1_noring_m117")                 # M < 128: a product of 65504 x 2 per pixel keeps every sum below 2^24
SPLIT_VARIANTS = [v for v in WG.VARIANTS if v["mode"] == "f16x3"]


def wgrad_positions(shape):
    """[(why, dy pixel (b, oy, ox), x pixel (b, iy, ix) that it multiplies)]: the first pixel, the last one, and one in the middle of the pixel
    range (several slabs: a slab other than the first)"""
    name, B, H, W, Cin, Cout, k, s, p = shape
    Ho, Wo = R.out_hw(H, W, k, k, s, p)
    M = B * Ho * Wo
    c = dict(H=H, W=W, KH=k, KW=k, stride=s, pad=p, B=B)
    out = []
    for why, m, which in (("first pixel", 0, 0), ("last pixel", M - 1, -1), ("middle pixel", M // 2 + 3, 0)):
        b, oy, ox = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
        taps = [(oy * s + ky - p, ox * s + kx - p) for ky in range(k) for kx in range(k) if 0 <= oy * s + ky - p < H and 0 <= ox * s + kx - p < W]
        iy, ix = taps[which]
        out.append((f"{why} (m = {m})", (b, oy, ox), (b, iy, ix)))
    slabs = WG.SLABS[name]
    if slabs and slabs[0] > 1:
        assert (M // 2 + 3) // -(-M // slabs[0]) >= 1 and (M // 2 + 3) // -(-M // slabs[1]) >= 1       # not in the first slab of either kernel
    return out


@pytest.mark.parametrize("name", WGRAD_SHAPES)
def test_wgrad_raises_the_flag(gpu_ctx, name):
    """wgrad_f16x3_kernel (every instantiation) and wgrad_split_kernel: a poisoned x element, a poisoned dy element, and a dy element whose value
    times 2^dy_shift reaches 65520"""
    import torch
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    shape = next(q for q in WG.SHAPES if q[0] == name)
    _, B, H, W, Cin, Cout, k, s, p = shape
    d = WG.operands(name, "I")
    desc = ConvDesc(B, H, W, Cin, Cout, k, k, s, p, 0, 0, 0)
    scratch = torch.empty(lib().amp_conv_wgrad_scratch_floats(C.byref(desc)), device="cuda:0")
    Kp = k * k * Cin
    gbuf, grad = WG._guarded((Cout, k, k, Cin), 128 * Kp)
    bbuf, bias = WG._guarded((Cout,), 256)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    scale = dev(d["scale"])
    missed, launches = [], 0
    for v in SPLIT_VARIANTS:
        x = R.shifted(d["x"], v["x_shift"]) if v["x_shift"] else d["x"]
        dy = R.shifted(d["dy"], v["dy_shift"]) if v["dy_shift"] else d["dy"]
        x_dev = dev(R.split_rows_ref(x) if v["x_split"] & 1 else x)
        dy_dev = dev(R.split_rows_ref(dy, v["dy_shift"]) if v["x_split"] & 2 else dy)
        px, pdy = Poke(x_dev, v["x_split"] & 1), Poke(dy_dev, v["x_split"] & 2)

        def run():
            grad.zero_()
            gpu_ctx.conv_range_flag()
            check(lib().amp_conv2d_wgrad_fmt(gpu_ctx.handle, C.byref(desc), ptr(x_dev), ptr(dy_dev), ptr(scale) if v["scale"] else None, ptr(scratch), ptr(grad), v["acc"],
                                             v["dy_shift"], v["x_shift"], v["x_split"], ptr(bias) if v["bias"] else None, int(v["bias"] == 2)), "amp_conv2d_wgrad_fmt")
            torch.cuda.synchronize()
            raised = gpu_ctx.conv_range_flag()
            assert not gpu_ctx.conv_range_flag()
            return raised

        assert not run(), f"{name} {v['name']}: the flag is up on clean operands"
        for why, dy_px, x_px in wgrad_positions(shape):
            pokes = [(px, x_px + (ch,), "x", val) for ch in (0, Cin - 1) for val in px.values()]
            pokes += [(pdy, dy_px + (ch,), "dy", val) for ch in (0, Cout - 1) for val in pdy.values()]
            if v["dy_shift"] and not v["x_split"] & 2:          # an fp32 dy the kernel lifts by 2^dy_shift: 65520 * 2^-dy_shift is in range before, beyond after
                pokes += [(pdy, dy_px + (ch,), "dy", sgn * 65520.0 * 2.0 ** -v["dy_shift"]) for ch in (0, Cout - 1) for sgn in (1, -1)]
            for poke, at, op, val in pokes:
                poke.put(at, val)
                raised = run()
                launches += 1
                poke.restore(at)
                if not raised:
                    missed.append(f"{v['name']}: {op}{at} = {say(val)} [{why}]")
        assert px.untouched() and pdy.untouched()
    assert bands_dirty_1d(gbuf, 128 * Kp) == 0 and bands_dirty_1d(bbuf, 256) == 0
    assert not missed, f"{name}: {len(missed)} of {launches} poisoned launches left the flag clear: " + "; ".join(missed[:8])


def bands_dirty_1d(buf, guard):
    n = buf.numel() - 2 * guard
    return int((buf[:guard] != WG.SENTINEL).sum() + (buf[guard + n:] != WG.SENTINEL).sum())


@pytest.mark.parametrize("name", WGRAD_EDGE_SHAPES)
def test_wgrad_with_the_largest_fp16_operand_is_exact(gpu_ctx, name):
    """+-65504 in the operand the variant does not scale (x; dy where x is lifted by 2^x_shift): exact, and the flag stays clear"""
    shape = next(q for q in WG.SHAPES if q[0] == name)
    d0 = WG.operands(name, "I")
    (_, dy_first, x_first), (_, dy_last, x_last) = wgrad_positions(shape)[:2]
    gpu_ctx.conv_range_flag()
    for v in SPLIT_VARIANTS:
        d = dict(d0)
        op, first, last, C_ = ("dy", dy_first, dy_last, shape[5]) if v["x_shift"] else ("x", x_first, x_last, shape[4])
        a = d0[op].copy()
        a[first + (0,)], a[last + (C_ - 1,)] = G.F16_MAX, -G.F16_MAX
        d[op] = a
        WG.run_variant(gpu_ctx, shape, "I", v, d)          # dW (and the bias sums) bit for bit against the float64 reference, sentinel bands
        assert not gpu_ctx.conv_range_flag(), f"{name} {v['name']}: the flag must stay clear at +-65504"


@pytest.mark.parametrize("cpg", [8, 64])
def test_grouped_wgrad_has_no_range(gpu_ctx, cpg):
    """the grouped weight gradient runs on the fp32 MFMA: an x element of 7e4 is a value like any other -- exact, flag clear"""
    import torch
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    B, H, W, Cw = WG.GROUPED_SHAPE
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    gpu_ctx.conv_range_flag()
    for stride, _, _ in WG.GROUPED_GEOMS:
        d = dict(WG.grouped_operands(cpg, stride))
        x = d["x"].copy()
        x[0, 0, 0, 0], x[B - 1, H - 1 - (H - 1) % stride, W - 1 - (W - 1) % stride, Cw - 1] = 7e4, -7e4      # pixels every stride reads
        d["x"] = x
        desc = ConvDesc(B, H, W, Cw, Cw, 3, 3, stride, 1, 0, 0, 0)
        scratch = torch.empty(lib().amp_grouped_wgrad_scratch_floats(C.byref(desc)), device="cuda:0")
        scale, x_dev = dev(d["scale"]), dev(x)
        for dy_shift in (0, 16):
            want, inside = WG.grouped_reference(cpg, stride, dy_shift, d)
            assert np.abs(want).max() >= 7e4 * 2.0 ** -dy_shift          # the element reaches the gradient (whose sums carry 2^-dy_shift)
            for fmt in (0, 2):                     # x stays fp32: 7e4 has no split form
                dy_dev = dev(R.split_rows_ref(d["dy"]) if fmt & 2 else d["dy"])
                guard = 64 * 9 * 64
                gbuf, grad = WG._guarded((Cw, 3, 3, 64), guard)
                check(lib().amp_conv2d_grouped_wgrad_fmt(gpu_ctx.handle, C.byref(desc), Cw // cpg, ptr(x_dev), ptr(dy_dev), ptr(scale), ptr(scratch), ptr(grad), fmt, dy_shift),
                      "amp_conv2d_grouped_wgrad_fmt")
                torch.cuda.synchronize()
                WG._check(gbuf, guard, want, 64, f"grouped wgrad with 7e4, cpg {cpg} stride {stride} fmt {fmt} dy_shift {dy_shift}")
    assert not gpu_ctx.conv_range_flag(), "the fp32 grouped weight gradient raised the range flag"
