"""Every launch family of conv_run (csrc/conv_plan.h conv_plan) against the float64 reference of tests/gemm_exact_ref.py, BIT FOR BIT: the
operands are of the classes on which both convolution arithmetics are exact (class I integers; class L with a live low half, AMP_CONV_F16X3 only),
so there is no tolerance.  Every case names the kernel and the epilogue it is meant to run and the switch state that selects them;
amp_debug_conv_plan is asked first, so a later rule change cannot make a case vacuous.  Every output lives inside a larger allocation
filled with a sentinel; the bands before and after it must come back untouched (an overrun at a ragged tile edge).

The case table, the operands and the references need no GPU: tests/test_gemm_exact_ref.py imports them, checks the exactness conditions
and shows that a seeded defect in the reference changes the expected output of every case (the data would show that defect)."""
import ctypes as C
import functools
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_exact_ref as R      # noqa: E402

X_SPLIT, Y_SPLIT, RES_SPLIT, MASK_SPLIT = 1, 2, 4, 8
XY = X_SPLIT | Y_SPLIT

# the switches of conv_plan in the order of tools/conv_plan_table.SWITCHES, their defaults, and the amp_debug_set_* entry of each
SW_DEFAULT = dict(f16x3_bn256=1, short_k=1, tall64=1, split_ring=1, korder=0, patch256=0, nloop=0, mask_tail_loop=1, patch_conv=1, stagger=1,
                  generic_epi=0, ablate=0)
SW_SETTER = dict(f16x3_bn256="amp_debug_set_f16x3_bn256", short_k="amp_debug_set_short_k", tall64="amp_debug_set_tall64",
                 split_ring="amp_debug_set_split_ring", korder="amp_debug_set_korder", patch256="amp_debug_set_patch256", nloop="amp_debug_set_nloop",
                 mask_tail_loop="amp_debug_set_mask_tail_loop", patch_conv="amp_debug_set_patch_conv",
                 generic_epi="amp_debug_set_conv_generic_epilogue", ablate="amp_debug_set_conv_ablate")

# values of amp::ConvKernel no case runs, and why
UNREACHED = {
    "MASK_TAIL": "the mask head's deconv with ReLU, predictor row and SIGMOID in its epilogue (PredictFuse): not an exact function of the operands, and "
                 "reached only through amp_mask_deconv_predict (tests/test_mask_tail_gpu.py holds it to the unfused chain)",
}
# launches of covered kernels that no case runs: the fused epilogues (ConvPlan::epi 3, 4, 5)
UNREACHED_LAUNCHES = {
    "SPLIT_128x256 / PATCH256 with RpnFuse": "the RPN predictors as a second GEMM in the epilogue: no stand-alone entry below 24576 pixels, and the hidden tensor is never written",
    "SPLIT_128x256 with PredictFuse": "as MASK_TAIL: a sigmoid in the epilogue",
}


def case(name, kernel, epi, B, H, W, Cin, Cout, k=1, stride=1, pad=0, mode="f16x3", classes=None, **kw):
    KH, KW = (k, k) if isinstance(k, int) else k
    c = dict(name=name, kernel=kernel, epi=epi, B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, mode=mode,
             relu=0, res_mode=0, out_mode=0, groups=1, fmt=0, in_shift=0, force_f32=0, mask=0, scale=1, shift=1, sw={}, keep=1.0)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    if classes is None:      # the low half exists in the split arithmetic only
        classes = ("I", "Lx", "Lw") if (mode == "f16x3" and not c["force_f32"] and kernel not in ("MFMA_64", "MFMA_128")) else ("I",)
    c["classes"] = classes
    return c


# Shapes: the smallest M at which the plan gives the family (Cout raised rather than M to meet the grid thresholds), then ragged: M, Ho and Wo
# are no multiples of a tile.  M = 89 * 91 = 8099 is 64 tiles of 128 (x 8 N tiles of 256 = 512, the 256-wide rule); 67 * 66 = 4422 is 35 tiles
# (x 15 or 16 N tiles of 128 >= 512); 93 * 94 = 8742 is 35 tiles of 256; 61 * 66 = 4026 is 32 tiles (x 32 N tiles of 128 = 1024, the short-K
# rule); 511 * 513 = 262143 is 1024 tiles of 256 (the tall rule).
CASES = [
    # ---- fp32 input, split in registers (conv_f16x3_kernel) ----
    case("f16x3_64_3x3", "F16X3_64", 1, 2, 7, 9, 64, 96, 3, 1, 1, relu=1, res_mode=1),
    case("f16x3_64_s2", "F16X3_64", 1, 1, 9, 11, 32, 64, 3, 2, 1),
    case("f16x3_64_p0", "F16X3_64", 1, 1, 6, 7, 32, 32, 3, 1, 0, relu=1, mask=1),
    case("f16x3_64_1xW", "F16X3_64", 1, 1, 1, 37, 32, 64, 3, 1, 1),
    case("f16x3_64_Hx2", "F16X3_64", 1, 1, 19, 2, 32, 64, 3, 1, 1),
    case("f16x3_64_5x3", "F16X3_64", 1, 1, 9, 8, 32, 64, (5, 3), 1, 1, classes=("I",)),
    case("f16x3_64_res2", "F16X3_64", 2, 1, 6, 10, 32, 64, 1, 1, 0, res_mode=2, relu=1),
    case("f16x3_64_deconv", "F16X3_64", 2, 2, 5, 7, 32, 128, 1, 1, 0, out_mode=1, relu=1),
    case("f16x3_64_scatter2", "F16X3_64", 2, 2, 5, 7, 64, 64, 1, 1, 0, out_mode=2, mask=1, res_mode=1),
    case("f16x3_64_generic", "F16X3_64", 0, 1, 7, 9, 32, 50, 3, 1, 1, relu=1, res_mode=1, mask=1),
    case("f16x3_64_generic_sw", "F16X3_64", 0, 1, 8, 10, 32, 64, 3, 1, 1, relu=1, res_mode=2, sw=dict(generic_epi=1)),
    case("f16x3_64_grouped", "F16X3_64", 1, 1, 7, 9, 128, 128, 3, 1, 1, groups=8, relu=1),
    case("f16x3_64_fc", "F16X3_64", 1, 1, 1, 70, 12544, 64, 1, 1, 0, keep=0.25, classes=("I", "Lx")),
    case("f16x3_128", "F16X3_128", 1, 1, 67, 66, 32, 1920, 1, 1, 0, relu=1, res_mode=1, classes=("I", "Lx")),
    case("f16x3_128_generic", "F16X3_128", 0, 1, 67, 66, 32, 1922, 1, 1, 0, relu=1, classes=("I",)),
    case("f16x3_128_3x3", "F16X3_128", 1, 1, 67, 66, 32, 1920, 3, 1, 1, mask=1, classes=("I", "Lw")),
    case("f16x3_128_s2_res2", "F16X3_128", 2, 1, 135, 131, 32, 1920, 1, 2, 0, res_mode=2, relu=1, classes=("I", "Lx")),
    case("f16x3_256", "F16X3_256", 1, 1, 89, 91, 32, 2048, 1, 1, 0, relu=1, res_mode=1, classes=("I", "Lw")),
    case("f16x3_256_3x3", "F16X3_256", 1, 1, 89, 91, 32, 2048, 3, 1, 1, classes=("I", "Lw")),
    case("f16x3_256_s2_res2", "F16X3_256", 2, 1, 179, 183, 32, 2048, 1, 2, 0, res_mode=2, mask=1, classes=("I", "Lx")),
    case("f16x3_stem", "F16X3_STEM", 1, 2, 21, 27, 4, 64, (7, 8), 2, 3, relu=1),
    case("f16x3_stem_s1_p0", "F16X3_STEM", 1, 1, 13, 19, 4, 64, (7, 8), 1, 0, res_mode=1, mask=1),
    case("f16x3_stem_res2_3x8", "F16X3_STEM", 0, 2, 14, 21, 4, 32, (3, 8), 1, 1, res_mode=2, relu=1),
    case("f16x3_stem_generic", "F16X3_STEM", 0, 1, 21, 27, 4, 50, (7, 8), 2, 3, relu=1, res_mode=1),
    # ---- split input, LDS-DMA, two buffers (conv_glds_kernel<F16>) ----
    case("f16x3s_64", "F16X3S_64", 1, 2, 7, 9, 64, 96, 3, 1, 1, fmt=XY | RES_SPLIT, relu=1, res_mode=1),
    case("f16x3s_64_s2", "F16X3S_64", 1, 1, 9, 11, 32, 64, 3, 2, 1, fmt=X_SPLIT),
    case("f16x3s_64_res2", "F16X3S_64", 2, 1, 6, 10, 32, 64, 1, 1, 0, fmt=XY | RES_SPLIT, res_mode=2, relu=1),
    case("f16x3s_64_noring", "F16X3S_64", 1, 1, 13, 11, 64, 128, 3, 1, 1, fmt=XY, relu=1, sw=dict(split_ring=0)),
    case("f16x3s_64_p0_mask", "F16X3S_64", 1, 1, 6, 7, 32, 32, 3, 1, 0, fmt=XY | MASK_SPLIT, mask=1, relu=1),
    case("f16x3s_64_mask32", "F16X3S_64", 1, 1, 7, 9, 32, 64, 3, 1, 1, fmt=X_SPLIT, mask=1),
    case("f16x3s_64_deconv", "F16X3S_64", 2, 2, 5, 7, 32, 128, 1, 1, 0, fmt=X_SPLIT, out_mode=1, relu=1),
    case("f16x3s_64_scatter2", "F16X3S_64", 2, 2, 5, 7, 64, 64, 1, 1, 0, fmt=X_SPLIT, out_mode=2, mask=1, res_mode=1),
    case("f16x3s_64_1xW", "F16X3S_64", 1, 1, 1, 37, 32, 64, 3, 1, 1, fmt=XY),
    case("f16x3s_64_Hx2", "F16X3S_64", 1, 1, 19, 2, 32, 64, 3, 1, 1, fmt=XY),
    case("f16x3s_g32", "F16X3S_G32", 1, 1, 9, 11, 128, 128, 3, 2, 1, groups=8, fmt=XY, relu=1),
    case("f16x3s_g32_cpg8", "F16X3S_G32", 1, 1, 7, 9, 64, 64, 3, 1, 1, groups=8, fmt=XY, relu=1, sw=dict(patch_conv=0)),
    case("f16x3s_g32_mask", "F16X3S_G32", 1, 1, 9, 11, 64, 64, 3, 2, 1, groups=4, fmt=XY | MASK_SPLIT | RES_SPLIT, mask=1, res_mode=1),
    case("f16x3s_128", "F16X3S_128", 1, 1, 67, 66, 32, 1952, 1, 1, 0, fmt=XY | RES_SPLIT, relu=1, res_mode=1, classes=("I", "Lx")),
    case("f16x3s_128_3x3", "F16X3S_128", 1, 1, 67, 66, 32, 1952, 3, 1, 1, fmt=XY | MASK_SPLIT, mask=1, classes=("I", "Lw")),
    case("f16x3s_128_s2_res2", "F16X3S_128", 2, 1, 135, 131, 32, 1952, 1, 2, 0, fmt=XY | RES_SPLIT, res_mode=2, relu=1, classes=("I", "Lx")),
    case("f16x3s_256", "F16X3S_256", 1, 1, 89, 91, 32, 2048, 1, 1, 0, fmt=XY | RES_SPLIT, relu=1, res_mode=1, sw=dict(split_ring=0), classes=("I", "Lw")),
    case("f16x3s_256_3x3", "F16X3S_256", 1, 1, 89, 91, 32, 2048, 3, 1, 1, fmt=XY | MASK_SPLIT, mask=1, sw=dict(split_ring=0), classes=("I", "Lx")),
    case("f16x3s_256_s2_res2", "F16X3S_256", 2, 1, 179, 183, 32, 2048, 1, 2, 0, fmt=X_SPLIT | RES_SPLIT, res_mode=2, relu=1, sw=dict(split_ring=0), classes=("I", "Lw")),
    # ---- split input, the ring kernels (conv_split_kernel) ----
    case("split_128x256", "SPLIT_128x256", 1, 1, 89, 91, 64, 2048, 1, 1, 0, fmt=XY, relu=1, classes=("I", "Lx")),
    case("split_128x256_y32_res32", "SPLIT_128x256", 1, 1, 89, 91, 32, 2048, 1, 1, 0, fmt=X_SPLIT, relu=1, res_mode=1, classes=("I", "Lw")),
    case("split_128x256_res", "SPLIT_128x256", 1, 1, 89, 91, 64, 2048, 1, 1, 0, fmt=XY | RES_SPLIT, relu=1, res_mode=1, sw=dict(short_k=0), classes=("I", "Lx")),
    case("split_128x256_mask", "SPLIT_128x256", 1, 1, 89, 91, 32, 2048, 1, 1, 0, fmt=XY | MASK_SPLIT, mask=1, classes=("I", "Lw")),
    case("split_128x256_shift", "SPLIT_128x256", 1, 1, 89, 91, 64, 2048, 1, 1, 0, fmt=XY | MASK_SPLIT, mask=1, in_shift=16, classes=("I",)),
    # (a live low half times 2^-16 next to an integer shift is no fp32 value: class L runs without the shift vector)
    case("split_128x256_shift_L", "SPLIT_128x256", 1, 1, 89, 91, 32, 2048, 1, 1, 0, fmt=XY, relu=1, in_shift=16, shift=0, classes=("Lx", "Lw")),
    case("split_128x256_3x3", "SPLIT_128x256", 1, 1, 89, 91, 32, 2048, 3, 1, 1, fmt=XY, relu=1, classes=("I", "Lx")),
    case("split_128x256_s2", "SPLIT_128x256", 1, 1, 177, 181, 32, 2048, 1, 2, 0, fmt=XY, classes=("I", "Lx")),
    case("split_128x256_deconv", "SPLIT_128x256", 2, 2, 5, 7, 64, 256, 1, 1, 0, fmt=XY, out_mode=1, relu=1),
    case("split_128x256_res2", "SPLIT_128x256", 2, 1, 90, 90, 32, 2048, 1, 1, 0, fmt=XY | RES_SPLIT, res_mode=2, relu=1, classes=("I", "Lw")),
    case("split_short", "SPLIT_SHORT_128x128", 1, 1, 61, 66, 64, 4096, 1, 1, 0, fmt=XY | RES_SPLIT, relu=1, res_mode=1, classes=("I", "Lx")),
    case("split_short_3x3", "SPLIT_SHORT_128x128", 1, 1, 61, 66, 32, 4096, 3, 1, 1, fmt=XY | RES_SPLIT, res_mode=1, classes=("I", "Lw")),
    case("split_short_s2", "SPLIT_SHORT_128x128", 1, 1, 121, 131, 64, 4096, 1, 2, 0, fmt=XY | RES_SPLIT, relu=1, res_mode=1, classes=("I", "Lx")),
    case("split_256x128", "SPLIT_256x128", 1, 1, 93, 94, 32, 1920, 1, 1, 0, fmt=XY | RES_SPLIT, relu=1, res_mode=1, sw=dict(short_k=0), classes=("I", "Lw")),
    case("split_256x128_3x3", "SPLIT_256x128", 1, 1, 93, 94, 32, 1920, 3, 1, 1, fmt=X_SPLIT, mask=1, classes=("I", "Lw")),
    case("split_256x128_s2_res2", "SPLIT_256x128", 2, 1, 187, 187, 32, 1920, 1, 2, 0, fmt=XY | RES_SPLIT, res_mode=2, relu=1, classes=("I", "Lx")),
    case("split_tall64", "SPLIT_TALL64", 1, 1, 511, 513, 32, 64, 3, 1, 1, fmt=XY, relu=1, classes=("I", "Lx")),
    case("split_tall64_s2", "SPLIT_TALL64", 1, 1, 1021, 1025, 32, 64, 1, 2, 0, fmt=X_SPLIT, res_mode=1, mask=1, classes=("I", "Lw")),
    case("nloop", "NLOOP", 1, 1, 89, 91, 64, 2048, 1, 1, 0, fmt=XY, relu=1, sw=dict(nloop=1), classes=("I", "Lx")),
    case("nloop_scatter", "NLOOP_SCATTER", 2, 1, 89, 91, 64, 2048, 1, 1, 0, fmt=XY, out_mode=1, relu=1, sw=dict(nloop=1), classes=("I", "Lw")),
    case("nloop_s2", "NLOOP", 1, 1, 177, 181, 64, 2048, 1, 2, 0, fmt=XY, sw=dict(nloop=1), classes=("I", "Lw")),
    case("nloop_scatter_s2", "NLOOP_SCATTER", 2, 1, 177, 181, 64, 2048, 1, 2, 0, fmt=XY, out_mode=1, sw=dict(nloop=1), classes=("I", "Lx")),
    # ---- the patch kernels: 8 x 16 pixel tiles, ragged H and W ----
    case("c64_patch", "C64_PATCH", 1, 2, 11, 21, 64, 64, 3, 1, 1, fmt=XY, relu=1, sw=dict(patch_conv=2)),
    case("c64_patch_mask", "C64_PATCH", 1, 1, 9, 17, 64, 64, 3, 1, 1, fmt=XY | MASK_SPLIT, mask=1, sw=dict(patch_conv=2)),
    case("c64_patch_cpg64", "C64_PATCH", 1, 1, 11, 21, 128, 128, 3, 1, 1, groups=2, fmt=XY, relu=1, sw=dict(patch_conv=2)),
    case("c64_patch_diag_cpg32", "C64_PATCH_DIAG", 1, 1, 11, 21, 128, 128, 3, 1, 1, groups=4, fmt=XY, relu=1, sw=dict(patch_conv=2)),
    case("c64_patch_diag_cpg16", "C64_PATCH_DIAG", 1, 1, 9, 17, 64, 64, 3, 1, 1, groups=4, fmt=XY, relu=1, sw=dict(patch_conv=2)),
    case("c64_patch_diag_cpg8", "C64_PATCH_DIAG", 1, 2, 7, 15, 64, 64, 3, 1, 1, groups=8, fmt=XY | MASK_SPLIT, mask=1, sw=dict(patch_conv=2)),
    case("patch256", "PATCH256", 1, 1, 11, 21, 64, 256, 3, 1, 1, fmt=XY, relu=1, sw=dict(patch256=2)),
    case("patch256_res_mask", "PATCH256", 1, 2, 9, 17, 96, 256, 3, 1, 1, fmt=XY | RES_SPLIT | MASK_SPLIT, res_mode=1, mask=1, sw=dict(patch256=2)),
    # ---- AMP_CONV_F32 (conv_glds_kernel, conv_mfma_kernel) ----
    case("glds_64_3x3", "GLDS_64", 1, 2, 7, 9, 64, 96, 3, 1, 1, mode="f32", relu=1, res_mode=1),
    case("glds_64_s2", "GLDS_64", 1, 1, 9, 11, 32, 64, 3, 2, 1, mode="f32", mask=1),
    case("glds_64_1xW", "GLDS_64", 1, 1, 1, 37, 32, 64, 3, 1, 1, mode="f32"),
    case("glds_64_Hx2", "GLDS_64", 1, 1, 19, 2, 32, 64, 3, 1, 1, mode="f32"),
    case("glds_64_res2", "GLDS_64", 2, 1, 6, 10, 32, 64, 1, 1, 0, mode="f32", res_mode=2, relu=1),
    case("glds_64_deconv", "GLDS_64", 2, 2, 5, 7, 32, 128, 1, 1, 0, mode="f32", out_mode=1, relu=1),
    case("glds_64_scatter2", "GLDS_64", 2, 2, 5, 7, 64, 64, 1, 1, 0, mode="f32", out_mode=2, mask=1, res_mode=1),
    case("glds_64_generic", "GLDS_64", 0, 1, 7, 9, 32, 50, 3, 1, 1, mode="f32", relu=1, res_mode=1, mask=1),
    case("glds_64_grouped", "GLDS_64", 1, 1, 7, 9, 128, 128, 3, 1, 1, mode="f32", groups=8, relu=1),
    case("glds_64_forced", "GLDS_64", 1, 1, 7, 9, 64, 96, 3, 1, 1, force_f32=1, relu=1),
    case("glds_128", "GLDS_128", 1, 1, 67, 66, 32, 1920, 1, 1, 0, mode="f32", relu=1, res_mode=1),
    case("glds_128_3x3", "GLDS_128", 1, 1, 67, 66, 32, 1920, 3, 1, 1, mode="f32", mask=1),
    case("glds_128_s2_res2", "GLDS_128", 2, 1, 135, 131, 32, 1920, 1, 2, 0, mode="f32", res_mode=2, relu=1),
    case("glds_128_deconv", "GLDS_128", 2, 1, 67, 66, 32, 1920, 1, 1, 0, mode="f32", out_mode=1, relu=1),
    case("glds_stem", "GLDS_STEM", 1, 2, 21, 27, 4, 64, (7, 8), 2, 3, mode="f32", relu=1),
    case("glds_stem_s1_p0", "GLDS_STEM", 1, 1, 13, 19, 4, 64, (7, 8), 1, 0, mode="f32", res_mode=1, mask=1),
    case("glds_stem_res2_3x8", "GLDS_STEM", 2, 2, 14, 21, 4, 32, (3, 8), 1, 1, mode="f32", res_mode=2, relu=1),
    case("glds_stem_generic", "GLDS_STEM", 0, 1, 21, 27, 4, 50, (7, 8), 2, 3, mode="f32", relu=1, res_mode=1),
    case("mfma_64", "MFMA_64", 1, 2, 7, 9, 12, 48, 3, 1, 1, mode="f32", relu=1, res_mode=1),
    case("mfma_64_f16x3_ctx", "MFMA_64", 1, 1, 9, 11, 12, 64, 3, 2, 1, mask=1),
    case("mfma_64_generic", "MFMA_64", 0, 1, 7, 9, 12, 50, 3, 1, 0, mode="f32", relu=1),
    case("mfma_64_deconv", "MFMA_64", 2, 2, 5, 7, 12, 64, 1, 1, 0, mode="f32", out_mode=1, relu=1),
    case("mfma_64_scatter2", "MFMA_64", 2, 2, 5, 7, 12, 48, 1, 1, 0, mode="f32", out_mode=2, mask=1, res_mode=1),
    case("mfma_64_1xW", "MFMA_64", 1, 1, 1, 37, 12, 48, 3, 1, 1, mode="f32"),
    case("mfma_64_Hx2", "MFMA_64", 1, 1, 19, 2, 12, 48, 3, 1, 1, mode="f32", mask=1),
    case("mfma_128", "MFMA_128", 1, 2, 7, 9, 12, 72, 3, 1, 1, mode="f32", relu=1, res_mode=1),
    case("mfma_128_res2", "MFMA_128", 2, 1, 6, 10, 12, 200, 1, 1, 0, mode="f32", res_mode=2),
    case("mfma_128_deconv", "MFMA_128", 2, 2, 5, 7, 12, 160, 1, 1, 0, mode="f32", out_mode=1, relu=1),
    case("mfma_128_scatter2_s2", "MFMA_128", 2, 1, 9, 13, 12, 72, 1, 2, 0, mode="f32", out_mode=2, mask=1),
    case("mfma_128_1xW", "MFMA_128", 1, 1, 1, 37, 12, 72, 3, 1, 1, mode="f32"),
    case("mfma_128_Hx2", "MFMA_128", 1, 1, 19, 2, 12, 72, 3, 1, 1, mode="f32", relu=1),
]
assert len({c["name"] for c in CASES}) == len(CASES)
CASE_IDS = [f"{c['name']}-{cls}" for c in CASES for cls in c["classes"]]
CASE_PARAMS = [(c, cls) for c in CASES for cls in c["classes"]]


def plan_inputs(c):
    """the 22 integers of amp_debug_conv_plan (tools/conv_plan_table.INPUTS) and the 12 switches of the case"""
    mode = 1 if c["mode"] == "f16x3" else 0
    inputs = [mode, c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KW"], c["stride"], c["pad"], c["relu"], c["res_mode"], c["out_mode"],
              c["groups"], c["fmt"], c["in_shift"], c["force_f32"], 1 if c["res_mode"] else 0, c["mask"], c["scale"], 0, 0]
    sw = dict(SW_DEFAULT)
    sw.update(c["sw"])
    import conv_plan_table as T
    return inputs, [sw[k] for k in T.SWITCHES]


def y_shape(c):
    Ho, Wo = R.out_hw(c["H"], c["W"], c["KH"], c["KW"], c["stride"], c["pad"])
    if c["out_mode"] == 1:
        return (c["B"], 2 * Ho, 2 * Wo, c["Cout"] // 4)
    if c["out_mode"] == 2:
        return (c["B"], 2 * Ho, 2 * Wo, c["Cout"])
    return (c["B"], Ho, Wo, c["Cout"])


@functools.lru_cache(maxsize=2)
def _operands(name, cls):
    c = next(q for q in CASES if q["name"] == name)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{cls}".encode()))
    cpg = c["Cin"] // c["groups"]
    xs, ws = (c["B"], c["H"], c["W"], c["Cin"]), (c["Cout"], c["KH"], c["KW"], cpg)
    x = {"I": R.class_i, "Lx": R.class_l_low, "Lw": R.class_l_int}[cls](rng, xs)
    w = {"I": R.class_i, "Lx": R.class_l_int, "Lw": R.class_l_low}[cls](rng, ws)
    if c["keep"] < 1.0:
        w = R.thin(rng, w, c["keep"])
    if c["in_shift"]:
        x = R.shifted(x, c["in_shift"])
    Ho, Wo = R.out_hw(c["H"], c["W"], c["KH"], c["KW"], c["stride"], c["pad"])
    d = dict(x=x, w=w, scale=R.scales(rng, c["Cout"]) if c["scale"] else None, shift=R.small_ints(rng, c["Cout"]) if c["shift"] else None, res=None, mask=None)
    if c["res_mode"] == 1:
        d["res"] = R.small_ints(rng, (c["B"], Ho, Wo, c["Cout"]))
    elif c["res_mode"] == 2:
        d["res"] = R.small_ints(rng, (c["B"], Ho // 2, Wo // 2, c["Cout"]))
    if c["mask"]:
        d["mask"] = R.small_ints(rng, y_shape(c), -2, 2)
    return d


def operands(c, cls):
    return _operands(c["name"], cls)


def reference(c, cls, d, defect=None, check=True):
    """the expected VALUES of y (float32, the shape of y_shape); with Y_SPLIT the device holds their split rows"""
    return R.conv_ref(d["x"], d["w"], d["scale"], d["shift"], d["res"], d["mask"], stride=c["stride"], pad=c["pad"], groups=c["groups"], relu=bool(c["relu"]),
                      res_mode=c["res_mode"], out_mode=c["out_mode"], in_shift=c["in_shift"], y_split=bool(c["fmt"] & Y_SPLIT),
                      low={"I": None, "Lx": "x", "Lw": "w"}[cls], defect=defect, check=check)


def applicable_defects(c, cls):
    """the seeded defects of gemm_exact_ref.CONV_DEFECTS that exist for the case (no border tap without padding, ...)"""
    Ho, Wo = R.out_hw(c["H"], c["W"], c["KH"], c["KW"], c["stride"], c["pad"])
    inside = lambda n_out, k, n_in: any(0 <= o * c["stride"] + k - 1 - c["pad"] < n_in for o in range(n_out))
    out = ["last_row"]
    if inside(Ho, c["KH"], c["H"]) and inside(Wo, c["KW"], c["W"]):      # (a 3x3 on a map of 1 x W: the last tap multiplies padding only)
        out.append("last_kstep")
    if c["pad"] > 0:
        out.append("border_tap")
    if c["KH"] == c["KW"] and c["KH"] > 1:
        out.append("swap_kykx")
    if cls != "I":
        out.append("cross_term")
    if c["res_mode"]:
        out.append("res_last_ntile")
    return out


# ---- the device side ------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FA5A5A5      # a NaN pattern no kernel writes


def _lib():
    from ampis_amd import _lib as M
    L = M.lib()
    vp, i = C.c_void_p, C.c_int
    L.amp_debug_conv_run.argtypes = [vp, C.POINTER(M.ConvDesc), i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i]
    L.amp_debug_conv_run.restype = i
    return L


def guarded(shape, zero_fill=False):
    """(whole buffer as int32, the view of `shape` inside it as float32, guard length): bands of 256 rows (whole tiles of every kernel) of the
    sentinel on both sides of the output"""
    import torch
    n = int(np.prod(shape))
    g = 256 * shape[-1]
    buf = torch.full((g + n + g,), SENTINEL, dtype=torch.int32, device="cuda:0")
    inner = buf[g:g + n]
    if zero_fill:
        inner.zero_()
    return buf, inner.view(torch.float32).view(*shape), g


def check_guarded(buf, g, want_bits, row_len, what, tile_m=128):
    """the bands first, then every word of the output"""
    host = buf.cpu().numpy()
    n = host.size - 2 * g
    lo, hi = np.flatnonzero(host[:g] != SENTINEL), np.flatnonzero(host[g + n:] != SENTINEL)
    assert lo.size == 0, f"{what}: {lo.size} words written BEFORE the output, the nearest {g - int(lo[-1])} words ahead of it"
    assert hi.size == 0, f"{what}: {hi.size} words written BEHIND the output, the first {int(hi[0])} words past its end"
    msg = R.first_difference(host[g:g + n], np.ascontiguousarray(want_bits).view(np.int32).reshape(-1), row_len, tile_m)
    assert not msg, f"{what}: {msg}"


def set_switches(L, sw):
    for k, v in sw.items():
        getattr(L, SW_SETTER[k])(int(v))


def planned(c):
    """(the 22 plan inputs, the kernel name the rules give): the case must get the kernel and the epilogue it is meant for"""
    import conv_plan_table as T
    inputs, switches = plan_inputs(c)
    chosen = T.plan(inputs, switches)
    assert (chosen[0], chosen[1]) == (c["kernel"], c["epi"]), f"{c['name']}: the plan gives {chosen}, the case is meant for {c['kernel']} with epilogue {c['epi']}"
    return inputs, chosen[0]


def upload(c, d, kernel):
    """the operands on the device in the formats of the case, and the weight forms it is launched with: split by conv_run per call (the public
    entries), and -- the split arithmetic only -- split beforehand as amp_model_finalize keeps them (here by the CPU reference of the format, so
    that no device split kernel stands between the operands and the convolution)"""
    import torch
    fmt = c["fmt"]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    t = dict(x=dev(R.split_rows_ref(d["x"], c["in_shift"]) if fmt & X_SPLIT else d["x"]),
             w=dev(R.group_window_weights(d["w"], c["Cin"] // c["groups"]) if c["groups"] > 1 else d["w"]),
             res=dev(R.split_rows_ref(d["res"]) if (fmt & RES_SPLIT) else d["res"]),
             mask=dev(R.split_rows_ref(d["mask"]) if (fmt & MASK_SPLIT) else d["mask"]), scale=dev(d["scale"]), shift=dev(d["shift"]))
    w_np = np.ascontiguousarray(t["w"].cpu().numpy())
    t["w_forms"] = [("split per call", None)]
    if kernel.startswith(("F16X3", "SPLIT", "NLOOP", "C64", "PATCH")):
        t["w_forms"].append(("weights split beforehand", dev(R.split_rows_ref(w_np.reshape(c["Cout"], -1)))))
    return t


def launch(ctx, c, inputs, t, w_split, y):
    """one amp_debug_conv_run of the case under its switches and mode; amp_debug_conv_plan is asked first (the process's current state, what
    conv_run is about to read), so the case cannot drift to another kernel"""
    import torch
    import conv_plan_table as T
    from ampis_amd._lib import ConvDesc, check, ptr
    L = _lib()
    desc = ConvDesc(c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KW"], c["stride"], c["pad"], c["relu"], c["res_mode"], c["out_mode"])
    ctx.conv_mode = c["mode"]
    try:
        set_switches(L, c["sw"])
        now = T.PlanOut()      # a null switch vector: the process's current state
        assert T._lib().amp_debug_conv_plan((C.c_int * 22)(*inputs), None, C.byref(now)) == 0
        assert T.kernel_names()[now.kernel] == c["kernel"] and now.epi == c["epi"], "the process's switch state gives another launch than the case's switch vector"
        check(L.amp_debug_conv_run(ctx.handle, C.byref(desc), c["groups"], ptr(t["x"]), ptr(t["w"]), ptr(w_split), ptr(t["scale"]), ptr(t["shift"]), ptr(t["res"]),
                                   ptr(t["mask"]), ptr(y), c["in_shift"], c["fmt"], c["force_f32"]), "amp_debug_conv_run")
        torch.cuda.synchronize()
    finally:
        set_switches(L, {k: SW_DEFAULT[k] for k in c["sw"]})
        ctx.conv_mode = "f16x3"


def case_tile_m(c):
    return 256 if c["kernel"] in ("SPLIT_256x128", "SPLIT_TALL64") else 128


def run_case(ctx, c, cls, d=None):
    """d: other operands than the case's own (tests/test_range_guard_gpu.py: the in-range edge)"""
    inputs, kernel = planned(c)
    d = operands(c, cls) if d is None else d
    want = reference(c, cls, d)
    t = upload(c, d, kernel)
    want_bits = R.split_rows_ref(want) if c["fmt"] & Y_SPLIT else want
    ctx.conv_range_flag()
    for form, w_split in t["w_forms"]:
        buf, y, g = guarded(want.shape, zero_fill=c["out_mode"] == 2)
        launch(ctx, c, inputs, t, w_split, y)
        check_guarded(buf, g, want_bits, want.shape[-1], f"{c['name']} [{cls}] {c['kernel']}, {form}", case_tile_m(c))
    assert not ctx.conv_range_flag(), "the range flag must stay clear"
    assert np.abs(want).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("c,cls", CASE_PARAMS, ids=CASE_IDS)
def test_conv_is_exact(gpu_ctx, c, cls):
    run_case(gpu_ctx, c, cls)


@pytest.mark.gpu
def test_public_entries_give_the_same_bits(gpu_ctx):
    """amp_conv2d_nhwc_ex / amp_conv2d_nhwc_fmt / amp_conv2d_grouped_nhwc(_fmt) are conv_run with fewer arguments, the grouped ones behind
    amp_group_expand_weights: one case each through the public C ABI against the same reference, every output between sentinel bands"""
    import torch
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    by_name = {c["name"]: c for c in CASES}
    L = lib()
    for name, cls in (("f16x3_64_3x3", "Lx"), ("f16x3s_64", "Lw"), ("f16x3_64_grouped", "I"), ("f16x3s_g32", "Lx"), ("f16x3_64_p0", "I")):
        c = by_name[name]
        d = operands(c, cls)
        want = reference(c, cls, d)
        fmt = c["fmt"]
        x = dev(R.split_rows_ref(d["x"]) if fmt & X_SPLIT else d["x"])
        res = dev(R.split_rows_ref(d["res"]) if fmt & RES_SPLIT else d["res"])
        w, scale, shift, mask = dev(d["w"]), dev(d["scale"]), dev(d["shift"]), dev(d["mask"])
        desc = ConvDesc(c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KW"], c["stride"], c["pad"], c["relu"], c["res_mode"], c["out_mode"])
        buf, y, g = guarded(want.shape)
        args = (ptr(scale), ptr(shift), ptr(res))
        if c["groups"] > 1:
            cpg = c["Cin"] // c["groups"]
            wbuf, w_win, wg = guarded((c["Cout"], c["KH"], c["KW"], 64))
            check(L.amp_group_expand_weights(gpu_ctx.handle, ptr(w), c["Cout"], c["KH"], c["KW"], cpg, ptr(w_win)), "amp_group_expand_weights")
            torch.cuda.synchronize()
            check_guarded(wbuf, wg, R.group_window_weights(d["w"], cpg), 64, f"{name}: amp_group_expand_weights")
            if fmt:
                check(L.amp_conv2d_grouped_nhwc_fmt(gpu_ctx.handle, C.byref(desc), c["groups"], ptr(x), ptr(w_win), *args, ptr(y), fmt), "amp_conv2d_grouped_nhwc_fmt")
            else:
                check(L.amp_conv2d_grouped_nhwc(gpu_ctx.handle, C.byref(desc), c["groups"], ptr(x), ptr(w_win), *args, ptr(y)), "amp_conv2d_grouped_nhwc")
        elif fmt:
            check(L.amp_conv2d_nhwc_fmt(gpu_ctx.handle, C.byref(desc), ptr(x), ptr(w), *args, ptr(y), fmt), "amp_conv2d_nhwc_fmt")
        else:
            check(L.amp_conv2d_nhwc_ex(gpu_ctx.handle, C.byref(desc), ptr(x), ptr(w), *args, ptr(mask), ptr(y)), "amp_conv2d_nhwc_ex")
        torch.cuda.synchronize()
        check_guarded(buf, g, R.split_rows_ref(want) if fmt & Y_SPLIT else want, want.shape[-1], f"{name} [{cls}] public entry")
    assert not gpu_ctx.conv_range_flag()


# ---- amp_bottleneck64_tail: conv2 3x3 + FrozenBN + ReLU + conv3 1x1 + FrozenBN + shortcut + ReLU in one launch -------------------------------
TAIL_CASES = [
    # name, B, H, W, C3, patch_conv switch, classes: 32 x 17 = 544 tiles of 8 x 16 pixels (the rule takes the kernel from 512 on), ragged H and W
    ("tail_c64", 1, 250, 270, 64, 1, ("I",)),
    ("tail_c256", 1, 250, 270, 256, 1, ("Lw",)),
    ("tail_small_c128", 2, 9, 17, 128, 2, ("I", "Lx", "Lw")),
]
TAIL_PARAMS = [(t, cls) for t in TAIL_CASES for cls in t[6]]


@functools.lru_cache(maxsize=2)
def tail_operands(name, cls):
    _, B, H, W, C3, _, _ = next(t for t in TAIL_CASES if t[0] == name)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{cls}".encode()))
    x = {"I": R.class_i, "Lx": R.class_l_low, "Lw": R.class_l_int}[cls](rng, (B, H, W, 64))
    w2 = {"I": R.class_i, "Lx": R.class_l_int, "Lw": R.class_l_low}[cls](rng, (64, 3, 3, 64))
    # conv2's output is conv3's operand: ReLU of integers / multiples of 2^-11 -- kept small by a sparse w2 so that it is an exact split value
    w2 = R.thin(rng, w2, 0.25)
    w3 = R.class_l_int(rng, (C3, 1, 1, 64))
    return dict(x=x, w2=w2, w3=w3, sc2=R.scales(rng, 64), sh2=R.small_ints(rng, 64), sc3=R.scales(rng, C3), sh3=R.small_ints(rng, C3),
                res=R.small_ints(rng, (B, H, W, C3)))


def tail_reference(d, cls, defect=None, check=True):
    low = {"I": None, "Lx": "x", "Lw": "w"}[cls]
    t2 = R.conv_ref(d["x"], d["w2"], d["sc2"], d["sh2"], stride=1, pad=1, relu=True, y_split=True, low=low, defect=defect if defect != "res_last_ntile" else None,
                    check=check)
    # t2 reaches conv3 as split halves: exact (asserted above); conv3's other operand is of {-1, 0, 1}, so a live low half of t2 stays exact
    return R.conv_ref(t2, d["w3"], d["sc3"], d["sh3"], d["res"], relu=True, res_mode=1, y_split=True, low="x" if cls != "I" else None,
                      defect="res_last_ntile" if defect == "res_last_ntile" else None, check=check)


@pytest.mark.gpu
@pytest.mark.parametrize("t,cls", TAIL_PARAMS, ids=[f"{t[0]}-{cls}" for t, cls in TAIL_PARAMS])
def test_bottleneck64_tail_is_exact(gpu_ctx, t, cls):
    import torch
    from ampis_amd._lib import check, ptr
    name, B, H, W, C3, patch_conv, _ = t
    L = _lib()
    d = tail_operands(name, cls)
    want = tail_reference(d, cls)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    xs, rs = dev(R.split_rows_ref(d["x"])), dev(R.split_rows_ref(d["res"]))
    w2s, w3s = dev(R.split_rows_ref(d["w2"].reshape(64, 576))), dev(R.split_rows_ref(d["w3"].reshape(C3, 64)))
    sc2, sh2, sc3, sh3 = (dev(d[k]) for k in ("sc2", "sh2", "sc3", "sh3"))
    buf, y, g = guarded(want.shape, zero_fill=False)
    gpu_ctx.conv_range_flag()
    try:
        L.amp_debug_set_patch_conv(patch_conv)
        check(L.amp_bottleneck64_tail(gpu_ctx.handle, B, H, W, ptr(xs), ptr(w2s), ptr(sc2), ptr(sh2), ptr(w3s), ptr(sc3), ptr(sh3), C3, ptr(rs), ptr(y)),
              "amp_bottleneck64_tail")
        torch.cuda.synchronize()
    finally:
        L.amp_debug_set_patch_conv(1)
    check_guarded(buf, g, R.split_rows_ref(want), C3, f"{name} [{cls}] amp_bottleneck64_tail")
    assert not gpu_ctx.conv_range_flag()


# ---- data gradients as a training step forms them ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
def test_strided_1x1_data_gradient_is_exact(gpu_ctx, split):
    """dx of a stride-2 1x1 convolution + FrozenBN: amp_dgrad_weights(_split) makes wt[c][0][0][n] = w[n][0][0][c] * scale[n], the forward kernel on dy
    with out_mode 2 scatters dy . wt to the even positions of a zeroed map, the ReLU mask and a residual gradient applied in its epilogue."""
    import torch
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    rng = np.random.default_rng(77 + split)
    B, Ho, Wo, Cin, Cout = 2, 5, 7, 64, 96
    w, sc = R.class_i(rng, (Cout, 1, 1, Cin)), R.scales(rng, Cout)
    dy = R.class_i(rng, (B, Ho, Wo, Cout))
    res = R.small_ints(rng, (B, Ho, Wo, Cin))
    act = R.small_ints(rng, (B, 2 * Ho, 2 * Wo, Cin), -2, 2)
    wt_ref = R.dgrad_weights_ref(w, sc)
    want = R.conv_ref(dy, wt_ref, None, None, res, act, res_mode=1, out_mode=2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    w_d, sc_d = dev(w), dev(sc)
    wbuf, wt, wg = guarded(wt_ref.shape)
    entry = lib().amp_dgrad_weights_split if split else lib().amp_dgrad_weights
    check(entry(gpu_ctx.handle, ptr(w_d), ptr(sc_d), Cout, 1, 1, Cin, ptr(wt)), "amp_dgrad_weights(_split)")
    torch.cuda.synchronize()
    check_guarded(wbuf, wg, R.split_rows_ref(wt_ref.reshape(Cin, Cout)).reshape(wt_ref.shape) if split else wt_ref, Cout, "amp_dgrad_weights(_split)")
    buf, y, g = guarded(want.shape, zero_fill=True)
    desc = ConvDesc(B, Ho, Wo, Cout, Cin, 1, 1, 1, 0, 0, 1, 2)
    L = _lib()
    gpu_ctx.conv_range_flag()
    dy_d, res_d, act_d = dev(dy), dev(res), dev(act)
    # the convolution consumes what the device made: the fp32 tensor (split per call), or the split one as the weights split beforehand
    w_plain = dev(wt_ref) if split else wt
    check(L.amp_debug_conv_run(gpu_ctx.handle, C.byref(desc), 1, ptr(dy_d), ptr(w_plain), ptr(wt) if split else None, None, None, ptr(res_d), ptr(act_d), ptr(y),
                               0, 0, 0), "amp_debug_conv_run")
    torch.cuda.synchronize()
    check_guarded(buf, g, want, Cin, "strided 1x1 data gradient")
    assert not gpu_ctx.conv_range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("cpg", [8, 64])
def test_grouped_stride2_data_gradient_is_exact(gpu_ctx, cpg):
    """dx of a stride-2 grouped 3x3: amp_subsample2_bwd spreads dy over the even positions of a zeroed map, then the grouped forward convolution
    (stride 1) with amp_group_dgrad_weights' windows -- transposed inside each 64-channel tile, taps flipped, times scale[co]."""
    import torch
    from ampis_amd import ops
    from ampis_amd._lib import ConvDesc, check, lib, ptr
    rng = np.random.default_rng(5 + cpg)
    B, H, W, Cw = 1, 9, 11, 128
    groups = Cw // cpg
    w, sc = R.class_i(rng, (Cw, 3, 3, cpg)), R.scales(rng, Cw)
    Ho, Wo = R.out_hw(H, W, 3, 3, 2, 1)
    dy = R.class_i(rng, (B, Ho, Wo, Cw))
    # the reference: dx[b, iy, ix, c] = sum over (n, ky, kx) with iy = 2 oy + ky - 1 of dy[b, oy, ox, n] * scale[n] * w[n, ky, kx, c - group offset]
    up = np.zeros((B, H, W, Cw), np.float32)
    up[:, ::2, ::2] = dy
    wt = np.zeros((Cw, 3, 3, cpg), np.float32)          # grouped weights of the data gradient: [c][2 - ky][2 - kx][n - group offset]
    for gi in range(groups):
        blk = (w[gi * cpg:(gi + 1) * cpg] * sc[gi * cpg:(gi + 1) * cpg, None, None, None])[:, ::-1, ::-1, :]
        wt[gi * cpg:(gi + 1) * cpg] = blk.transpose(3, 1, 2, 0)
    want = R.conv_ref(up, wt, stride=1, pad=1, groups=groups)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    w_win_ref = R.group_window_weights(w, cpg)
    # transposed inside each 64-channel tile, taps flipped, times scale[co] -- every slot of the window, so a zero outside the group keeps scale's sign
    wt_win_ref = np.empty_like(w_win_ref)
    for t0 in range(0, Cw, 64):
        blk = w_win_ref[t0:t0 + 64] * sc[t0:t0 + 64, None, None, None]          # [n][ky][kx][j]: input channel t0 + j
        wt_win_ref[t0:t0 + 64] = blk[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)       # [c = t0 + j][2 - ky][2 - kx][n - t0]
    assert np.array_equal(wt_win_ref, R.group_window_weights(wt, cpg))           # the same numbers as the grouped form above (signs of zero aside)
    w_win, sc_d = dev(w_win_ref), dev(sc)
    wbuf, wt_win, wg = guarded(w_win_ref.shape)
    check(lib().amp_group_dgrad_weights(gpu_ctx.handle, ptr(w_win), ptr(sc_d), Cw, 3, 3, ptr(wt_win)), "amp_group_dgrad_weights")
    torch.cuda.synchronize()
    check_guarded(wbuf, wg, wt_win_ref, 64, "amp_group_dgrad_weights")
    dx0 = torch.zeros((B, H, W, Cw), device="cuda:0")
    ops.subsample2_bwd(gpu_ctx, dev(dy), dx0)
    buf, y, g = guarded((B, H, W, Cw))
    desc = ConvDesc(B, H, W, Cw, Cw, 3, 3, 1, 1, 0, 0, 0)
    check(lib().amp_conv2d_grouped_nhwc(gpu_ctx.handle, C.byref(desc), groups, ptr(dx0), ptr(wt_win), None, None, None, ptr(y)), "amp_conv2d_grouped_nhwc")
    torch.cuda.synchronize()
    check_guarded(buf, g, want, Cw, "grouped stride-2 data gradient")


def test_every_conv_kernel_is_covered_or_listed():
    import conv_plan_table as T
    names = set(T.kernel_names())
    covered = {c["kernel"] for c in CASES}
    assert covered <= names and set(UNREACHED) <= names and not (covered & set(UNREACHED))
    assert not (names - covered - set(UNREACHED)), f"no exact case runs {sorted(names - covered - set(UNREACHED))}"


def append_plan_rows():
    """python tests/test_conv_exact_gpu.py: append a row to tests/golden/conv_plan_table.json for every case that has none yet, its chosen half
    recorded from the CURRENT rules (said so in the table's "what" field), through tools/conv_plan_table.py's load / plan / save"""
    import conv_plan_table as T
    t = T.load()
    have = {(tuple(r[0]), tuple(r[1])) for r in t["rows"]}
    new = []
    for c in CASES:
        inputs, switches = plan_inputs(c)
        if (tuple(inputs), tuple(switches)) not in have:
            have.add((tuple(inputs), tuple(switches)))
            new.append([inputs, switches, T.plan(inputs, switches)])
    t["rows"] += new
    note = "; the rows of tests/test_conv_exact_gpu.py's cases were appended later, their chosen half recorded from the rules current at that commit"
    if note not in t["what"]:
        t["what"] += note
    T.save(t)
    print(f"{len(new)} rows appended")


if __name__ == "__main__":
    append_plan_rows()
