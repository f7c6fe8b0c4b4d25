"""The weight-gradient kernels (csrc/wgrad.hip: wgrad_mfma_kernel, every instantiation of wgrad_f16x3_kernel that launch_wgrad_f16x3 can pick,
wgrad_split_kernel; csrc/grouped_bwd.hip: grouped_wgrad9_kernel, grouped_wgrad_kernel) against the float64 reference of
tests/gemm_exact_ref.py, BIT FOR BIT, on operands for which every summation order is exact (class I integers, class L with a live low half,
and both times 2^-16 under the entry's shift).  grad and bias_grad live inside larger allocations filled with a sentinel whose bands must
come back untouched.  The shapes, operands and references need no GPU: tests/test_gemm_exact_ref.py checks them on the CPU."""
import ctypes as C
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_exact_ref as R      # noqa: E402

SENTINEL = 0x7FA5A5A5

# name, B, H, W, Cin, Cout, k, stride, pad.  Per geometry (3x3 s1 p1; 1x1 s2; 2x2 s2: the deconv's shape) three pixel counts: M < 256 (one slab),
# M no multiple of the 32-pixel step (one slab still: M / 256 < 2), and M >= 512 chosen so that pick_nsplit (128 x 128 tiles, rounds of 512
# workgroups) and pick_nsplit_ring (128 x 256 tiles, rounds of 256) give DIFFERENT slab counts -- SLABS below, recomputed by
# test_gemm_exact_ref.py from the formulas.  For the 2x2 geometry K' = 4 Cin is a multiple of 512, the ring has exactly half the tiles in rounds of
# half the size, and the two counts agree for every M (searched up to 30000): its large case is multi-slab with equal counts.
SHAPES = [
    ("3x3_m99", 1, 9, 11, 128, 512, 3, 1, 1),
    ("3x3_m323", 1, 17, 19, 128, 512, 3, 1, 1),
    ("3x3_m3465", 3, 33, 35, 128, 512, 3, 1, 1),
    ("1x1s2_m63", 1, 13, 17, 384, 2048, 1, 2, 0),
    ("1x1s2_m342", 1, 35, 37, 384, 2048, 1, 2, 0),
    ("1x1s2_m2310", 2, 65, 70, 384, 2048, 1, 2, 0),
    ("2x2s2_m63", 1, 14, 18, 128, 256, 2, 2, 0),
    ("2x2s2_m323", 1, 34, 38, 128, 256, 2, 2, 0),
    ("2x2s2_m1150", 2, 46, 50, 128, 256, 2, 2, 0),
    # no ring shape (K' = 128 < 256, Cout % 128 != 0): a split x AND a pre-scaled split dy stay on wgrad_f16x3_kernel<1, true, false, true>
    ("1x1_noring_m117", 1, 9, 13, 128, 160, 1, 1, 0),
]
SLABS = {"3x3_m99": (1, 1), "3x3_m323": (1, 1), "3x3_m3465": (13, 11), "1x1s2_m63": (1, 1), "1x1s2_m342": (1, 1), "1x1s2_m2310": (9, 8),
         "2x2s2_m63": (1, 1), "2x2s2_m323": (1, 1), "2x2s2_m1150": (4, 4), "1x1_noring_m117": None}
CLASSES = ("I", "Ldy", "Lx")

# The calls made on every shape.  kernel: what amp_conv2d_wgrad_fmt launches (wgrad.hip:1065-1080); the template arguments are <SC, XS, BIAS(, PRE)>:
# SC 1 = dy scaled, 2 = x scaled; XS = x in split rows; PRE = dy in split rows, already times 2^dy_shift.  bias: 1 = written, 2 = accumulated.
VARIANTS = [
    dict(name="mfma", mode="f32"),
    dict(name="mfma_scale_acc", mode="f32", scale=1, acc=1),
    dict(name="f16x3<0,0,0>"),
    dict(name="f16x3<1,0,0>", dy_shift=16, scale=1, acc=1),
    dict(name="f16x3<2,0,0>", x_shift=16),
    dict(name="f16x3<0,0,1>", bias=1, scale=1),
    dict(name="f16x3<1,0,1>", dy_shift=16, bias=2),
    dict(name="f16x3<2,0,1>", x_shift=16, bias=1, acc=1),
    dict(name="f16x3<0,1,0>", x_split=1, acc=1),
    dict(name="f16x3<1,1,0>", x_split=1, dy_shift=16),
    dict(name="f16x3<0,1,1>", x_split=1, bias=2, scale=1, acc=1),
    dict(name="f16x3<1,1,1>", x_split=1, dy_shift=16, bias=1),
    dict(name="f16x3<1,0,0,pre>", x_split=2, dy_shift=16, scale=1),
    dict(name="split_or_f16x3<1,1,0,pre>", x_split=3, dy_shift=16, scale=1, acc=1),      # wgrad_split_kernel where ring_shape holds
    dict(name="split_or_pre_shift0", x_split=3, dy_shift=0),
]
for _v in VARIANTS:
    for _k, _d in (("mode", "f16x3"), ("dy_shift", 0), ("x_shift", 0), ("x_split", 0), ("bias", 0), ("scale", 0), ("acc", 0)):
        _v.setdefault(_k, _d)


def ring_shape(Cout, Cin, Kp):
    return Cout % 128 == 0 and Cin % 128 == 0 and Kp >= 256


def variants_for(cls):
    return [v for v in VARIANTS if cls == "I" or v["mode"] == "f16x3"]      # the low half exists in the split arithmetic only


@functools.lru_cache(maxsize=2)
def operands(name, cls):
    _, B, H, W, Cin, Cout, k, s, p = next(q for q in SHAPES if q[0] == name)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{cls}".encode()))
    Ho, Wo = R.out_hw(H, W, k, k, s, p)
    x = {"I": R.class_i, "Ldy": R.class_l_int, "Lx": R.class_l_low}[cls](rng, (B, H, W, Cin))
    dy = {"I": R.class_i, "Ldy": R.class_l_low, "Lx": R.class_l_int}[cls](rng, (B, Ho, Wo, Cout))
    return dict(x=x, dy=dy, scale=R.scales(rng, Cout), grad0=R.small_ints(rng, (Cout, k, k, Cin)), bias0=R.small_ints(rng, Cout))


def variant_reference(shape, cls, v, d, defect=None, check=True):
    """x and dy as the entry computes with them, the previous contents of grad / bias_grad where the call accumulates (times 2^-shift like the
    sums they join: a live low half times 2^-16 next to an integer is no fp32 value), and the expected dW and bias sums"""
    _, B, H, W, Cin, Cout, k, s, p = shape
    sh = v["x_shift"] + v["dy_shift"]
    x = R.shifted(d["x"], v["x_shift"]) if v["x_shift"] else d["x"]
    dy = R.shifted(d["dy"], v["dy_shift"]) if v["dy_shift"] else d["dy"]
    grad0 = R.shifted(d["grad0"], sh) if v["acc"] else None
    bias0 = R.shifted(d["bias0"], v["dy_shift"]) if v["bias"] == 2 else None
    g, b = R.wgrad_ref(x, dy, k, k, d["scale"] if v["scale"] else None, grad0, bias0, stride=s, pad=p, dy_shift=v["dy_shift"], want_bias=bool(v["bias"]),
                       low={"I": None, "Ldy": "dy", "Lx": "x"}[cls], defect=defect, check=check)
    return dict(x=x, dy=dy, grad0=grad0, bias0=bias0, g=g, b=b)


def _guarded(shape, guard, fill=None):
    import torch
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int32, device="cuda:0")
    inner = buf[guard:guard + n].view(torch.float32).view(*shape)
    if fill is not None:
        inner.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
    return buf, inner


def _check(buf, guard, want, row_len, what):
    host = buf.cpu().numpy()
    n = host.size - 2 * guard
    lo, hi = np.flatnonzero(host[:guard] != SENTINEL), np.flatnonzero(host[guard + n:] != SENTINEL)
    assert lo.size == 0, f"{what}: {lo.size} words written BEFORE the tensor, the nearest {guard - int(lo[-1])} words ahead of it"
    assert hi.size == 0, f"{what}: {hi.size} words written BEHIND the tensor, the first {int(hi[0])} words past its end"
    msg = R.first_difference(host[guard:guard + n], np.ascontiguousarray(want).view(np.int32).reshape(-1), row_len, 128, 128)
    assert not msg, f"{what}: {msg}"


def run_variant(ctx, shape, cls, v, d):
    import torch
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    name, B, H, W, Cin, Cout, k, s, p = shape
    r = variant_reference(shape, cls, v, d)
    x, dy, want_g, want_b = r["x"], r["dy"], r["g"], r["b"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    x_dev = dev(R.split_rows_ref(x) if v["x_split"] & 1 else x)
    dy_dev = dev(R.split_rows_ref(dy, v["dy_shift"]) if v["x_split"] & 2 else dy)
    desc = ConvDesc(B, H, W, Cin, Cout, k, k, s, p, 0, 0, 0)
    Kp = k * k * Cin
    scratch = torch.empty(lib().amp_conv_wgrad_scratch_floats(C.byref(desc)), device="cuda:0")
    gbuf, grad = _guarded((Cout, k, k, Cin), 128 * Kp, r["grad0"])
    bbuf = bias = None
    if v["bias"]:
        bbuf, bias = _guarded((Cout,), 256, r["bias0"])
    scale = dev(d["scale"]) if v["scale"] else None
    ctx.conv_mode = v["mode"]
    try:
        check(lib().amp_conv2d_wgrad_fmt(ctx.handle, C.byref(desc), ptr(x_dev), ptr(dy_dev), ptr(scale), ptr(scratch),
                                         ptr(grad), v["acc"], v["dy_shift"], v["x_shift"], v["x_split"], ptr(bias) if v["bias"] else None,
                                         int(v["bias"] == 2)), "amp_conv2d_wgrad_fmt")
        torch.cuda.synchronize()
    finally:
        ctx.conv_mode = "f16x3"
    what = f"{name} [{cls}] {v['name']}"
    _check(gbuf, 128 * Kp, want_g, Kp, what + " dW")
    if v["bias"]:
        _check(bbuf, 256, want_b, Cout, what + " bias")
    assert np.abs(want_g).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_wgrad_is_exact(gpu_ctx, shape, cls):
    """every variant on one shape and operand class; the first call of a geometry on the context makes its row table, the others read the cached one"""
    d = operands(shape[0], cls)
    gpu_ctx.conv_range_flag()
    hits0 = gpu_ctx.rowtab_stats()
    calls = variants_for(cls)
    for v in calls:
        run_variant(gpu_ctx, shape, cls, v, d)
    hits1 = gpu_ctx.rowtab_stats()
    # at most the first call of a geometry on the context makes its table; every other one must read the cached table
    assert hits1["hits"] - hits0["hits"] >= len(calls) - 1, (hits0, hits1, len(calls))
    assert not gpu_ctx.conv_range_flag(), "the range flag must stay clear"


@pytest.mark.gpu
def test_geometries_that_differ_only_in_pad_do_not_share_a_row_table(gpu_ctx):
    """3x3 stride 1 on the same tensor with pad 1 and pad 0, alternating: each must get its own table (the key holds the pad)"""
    rng = np.random.default_rng(4)
    B, H, W, Cin, Cout = 1, 11, 13, 128, 128
    x = R.class_i(rng, (B, H, W, Cin))
    for pad in (1, 0, 1, 0):
        Ho, Wo = R.out_hw(H, W, 3, 3, 1, pad)
        dy = R.class_i(np.random.default_rng(pad), (B, Ho, Wo, Cout))
        shape = (f"pad{pad}", B, H, W, Cin, Cout, 3, 1, pad)
        d = dict(x=x, dy=dy, scale=None, grad0=None, bias0=None)
        for v in (VARIANTS[0], VARIANTS[2]):
            run_variant(gpu_ctx, shape, "I", v, d)
    assert not gpu_ctx.conv_range_flag()


# ---- grouped weight gradients (ResNeXt conv2) ----------------------------------------------------------------------------------------------------
# geometry: (stride, which kernel amp_conv2d_grouped_wgrad_fmt launches for a fp32 x / for a split x)
GROUPED_GEOMS = [(1, "grouped_wgrad9_kernel", "grouped_wgrad_kernel"), (2, "grouped_wgrad_kernel", "grouped_wgrad_kernel")]
GROUPED_SHAPE = (2, 9, 11, 128)      # B, H, W, C: two 64-channel tiles, ragged rows


@functools.lru_cache(maxsize=8)
def grouped_operands(cpg, stride):
    B, H, W, Cw = GROUPED_SHAPE
    rng = np.random.default_rng(100 * cpg + stride)
    Ho, Wo = R.out_hw(H, W, 3, 3, stride, 1)
    return dict(x=R.class_i(rng, (B, H, W, Cw)), dy=R.class_i(rng, (B, Ho, Wo, Cw)), scale=R.scales(rng, Cw))


def grouped_reference(cpg, stride, dy_shift, d, defect=None, check=True):
    """fmt bit 1 or not, dy HOLDS dy * 2^dy_shift (the reduce pass multiplies the sums by 2^-dy_shift): the stored tensor is d['dy']"""
    dy_true = R.shifted(d["dy"], dy_shift) if dy_shift else d["dy"]
    return R.grouped_wgrad_ref(d["x"], dy_true, 3, 3, cpg, d["scale"], stride=stride, pad=1, dy_shift=dy_shift, defect=defect, check=check)


@pytest.mark.gpu
@pytest.mark.parametrize("cpg", [8, 16, 32, 64])
def test_grouped_wgrad_is_exact(gpu_ctx, cpg):
    import torch
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    B, H, W, Cw = GROUPED_SHAPE
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    for stride, _, _ in GROUPED_GEOMS:
        d = grouped_operands(cpg, stride)
        desc = ConvDesc(B, H, W, Cw, Cw, 3, 3, stride, 1, 0, 0, 0)
        scratch = torch.empty(lib().amp_grouped_wgrad_scratch_floats(C.byref(desc)), device="cuda:0")
        scale = dev(d["scale"])
        for dy_shift in (0, 16):
            want, inside = grouped_reference(cpg, stride, dy_shift, d)
            assert np.all(want[~inside].view(np.int32) == 0) and np.abs(want).max() > 0
            for fmt in range(4):
                x_dev = dev(R.split_rows_ref(d["x"]) if fmt & 1 else d["x"])
                dy_dev = dev(R.split_rows_ref(d["dy"]) if fmt & 2 else d["dy"])
                guard = 64 * 9 * 64
                gbuf, grad = _guarded((Cw, 3, 3, 64), guard)
                check(lib().amp_conv2d_grouped_wgrad_fmt(gpu_ctx.handle, C.byref(desc), Cw // cpg, ptr(x_dev), ptr(dy_dev), ptr(scale), ptr(scratch),
                                                         ptr(grad), fmt, dy_shift), "amp_conv2d_grouped_wgrad_fmt")
                torch.cuda.synchronize()
                _check(gbuf, guard, want, 64, f"grouped wgrad cpg {cpg} stride {stride} fmt {fmt} dy_shift {dy_shift}")      # exact zeros outside each group included
