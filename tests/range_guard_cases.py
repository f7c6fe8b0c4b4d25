"""Shared by tests/test_range_guard_cases.py (no GPU) and tests/test_range_guard_gpu.py: where the split arithmetic (AMP_CONV_F16X3) is
pulled over the edge of the fp16 range, case by case.

The cases are those of tests/test_conv_exact_gpu.py whose planned kernel multiplies split operands; a POISON is one element of x or of w
replaced by a value the split cannot hold (|v| >= 65520 rounds to an infinite hi half), at the positions where a range check can go
missing: the first output row, the last valid row of the ragged last tile, a row in the second half of a tile, the first and the last
channel, the first, the last and an interior output column, the first and the last k index.  A position is kept only if a valid output
reads it (computed here from stride, pad, kernel and map size, and checked against the float64 reference by the CPU test), so that
"the flag is set" can never hold vacuously.  The IN-RANGE EDGE is the opposite: elements of +-65504, the largest fp16 value, on which the
flag must stay clear and the result exact."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_exact_ref as R                                                          # noqa: E402
from bwd_glue_ref import split_halves                                              # noqa: E402
from test_conv_exact_gpu import CASES, Y_SPLIT, case_tile_m as tile_rows, operands, reference, y_shape       # noqa: E402

SPLIT_PREFIXES = ("F16X3", "SPLIT", "NLOOP", "C64", "PATCH")      # the kernel names of the split arithmetic (run_case's own test for "weights split beforehand")
GUARD_CASES = [c for c in CASES if c["mode"] == "f16x3" and c["kernel"].startswith(SPLIT_PREFIXES)]
GUARD_IDS = [c["name"] for c in GUARD_CASES]
# fp32 kernels reached from an AMP_CONV_F16X3 context: no range, so no flag
F32_FROM_F16X3_CTX = [c for c in CASES if c["name"] in ("mfma_64_f16x3_ctx", "glds_64_forced")]

# split-arithmetic kernels no flag-raising case launches through amp_debug_conv_run, and where they are pulled instead
UNREACHED = {
    "MASK_TAIL": "reached only through amp_mask_deconv_predict: tests/test_range_guard_gpu.py poisons it there (test_fused_mask_tail_raises_the_flag_or_is_right)",
}

F16_MAX = 65504.0
FP32_POISONS = (65520.0, -65520.0, 7e4, float("inf"), float("nan"))      # 65520 is the first fp32 value that rounds to an infinite half


def split_pair(v):
    """(hi, lo') as a producer's epilogue writes them for the fp32 value v: hi = (f16)v, lo' = (f16)((v - (float)hi) * 2048)"""
    hi, lo = split_halves(R.split_rows_ref(np.full(32, v, np.float32)))
    return hi[0], lo[0]


# what a split-row operand can hold of a value beyond the range: the producer's pair of every fp32 poison, and the hand-made (inf, 0)
SPLIT_POISONS = tuple(split_pair(v) for v in FP32_POISONS) + ((np.float16(np.inf), np.float16(0.0)),)


def geometry(c):
    Ho, Wo = R.out_hw(c["H"], c["W"], c["KH"], c["KW"], c["stride"], c["pad"])
    return Ho, Wo, c["B"] * Ho * Wo


def row_taps(c, m):
    """the taps (ky, kx, iy, ix) of output row m = (b, oy, ox) that fall inside the map, in the K order"""
    Ho, Wo, _ = geometry(c)
    oy, ox = (m // Wo) % Ho, m % Wo
    out = []
    for ky in range(c["KH"]):
        for kx in range(c["KW"]):
            iy, ix = oy * c["stride"] + ky - c["pad"], ox * c["stride"] + kx - c["pad"]
            if 0 <= iy < c["H"] and 0 <= ix < c["W"]:
                out.append((ky, kx, iy, ix))
    return out


def readers_of_pixel(c, iy, ix):
    """the (oy, ox) whose window holds input pixel (iy, ix): the other direction of row_taps, written on its own"""
    Ho, Wo, _ = geometry(c)
    out = []
    for ky in range(c["KH"]):
        ny = iy + c["pad"] - ky
        if ny % c["stride"] or not 0 <= ny // c["stride"] < Ho:
            continue
        for kx in range(c["KW"]):
            nx = ix + c["pad"] - kx
            if nx % c["stride"] == 0 and 0 <= nx // c["stride"] < Wo:
                out.append((ny // c["stride"], nx // c["stride"]))
    return out


def readers_of_tap(c, ky, kx):
    """the (oy, ox) for which weight tap (ky, kx) multiplies a pixel inside the map (elsewhere it multiplies padding)"""
    Ho, Wo, _ = geometry(c)
    ys = [oy for oy in range(Ho) if 0 <= oy * c["stride"] + ky - c["pad"] < c["H"]]
    xs = [ox for ox in range(Wo) if 0 <= ox * c["stride"] + kx - c["pad"] < c["W"]]
    return [(oy, ox) for oy in ys for ox in xs]


def _rng(c, what):
    return np.random.default_rng(zlib.crc32(f"range guard/{c['name']}/{what}".encode()))


def x_positions(c):
    """[(why, (b, iy, ix, ch))]: pixels read by output row 0, by the last valid row M - 1 and by a seeded row in the second half of a tile,
    each at the first and the last channel (grouped: of the first and of the last group)"""
    Ho, Wo, M = geometry(c)
    rng = _rng(c, "x")
    rows = [("row 0", 0, 0), ("last row", M - 1, -1)]
    T = tile_rows(c)
    second_half = [m for m in range(M) if (m % T) >= T // 2 and m not in (0, M - 1)]
    if second_half:
        rows.append(("second half of a tile", int(rng.choice(second_half)), None))
    cpg = c["Cin"] // c["groups"]
    chans = sorted({0, cpg - 1, c["Cin"] - cpg, c["Cin"] - 1})
    out = []
    for why, m, which in rows:
        taps = row_taps(c, m)
        if not taps:
            continue
        ky, kx, iy, ix = taps[int(rng.integers(len(taps)))] if which is None else taps[which]
        for ch in chans:
            out.append((f"x, {why} (m = {m}, tap {ky},{kx}), channel {ch}", (m // (Ho * Wo), iy, ix, ch)))
    return out


def w_positions(c):
    """[(why, (n, ky, kx, cc))] in the grouped layout [Cout][KH][KW][Cin / groups]: columns 0, Cout - 1 and a seeded interior one, at the first and
    the last k index whose tap some valid output reads"""
    rng = _rng(c, "w")
    cpg = c["Cin"] // c["groups"]
    taps = [(ky, kx) for ky in range(c["KH"]) for kx in range(c["KW"]) if readers_of_tap(c, ky, kx)]
    ks = [taps[0] + (0,), taps[-1] + (cpg - 1,)]
    cols = [0, c["Cout"] - 1, int(rng.integers(1, c["Cout"] - 1))]
    return [(f"w, column {n}, k = ({ky},{kx},{cc})", (n, ky, kx, cc)) for n in cols for ky, kx, cc in ks]


def w_window_index(c, idx):
    """the index of grouped weight element idx in the array the device holds: [Cout][KH][KW][cpg], or the 64-channel window of a grouped case"""
    n, ky, kx, cc = idx
    if c["groups"] == 1:
        return idx
    cpg = c["Cin"] // c["groups"]
    return (n, ky, kx, (n // cpg) * cpg - (n & ~63) + cc)


def to_y_layout(t, out_mode):
    """[B, Ho, Wo, Cout] -> the layout of y (the rearrangements of gemm_exact_ref.conv_ref)"""
    B, Ho, Wo, Cout = t.shape
    if out_mode == 1:
        return t.reshape(B, Ho, Wo, 2, 2, Cout // 4).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, Cout // 4)
    if out_mode == 2:
        z = np.zeros((B, 2 * Ho, 2 * Wo, Cout), t.dtype)
        z[:, ::2, ::2] = t
        return z
    return t


def footprint(c, op, idx, mask=None, padding_multiplies=False):
    """bool array of the shape of y: the outputs that read the poisoned element (and that the output mask lets through).  padding_multiplies:
    a weight tap also counts where it meets the zero padding -- the reference, like the kernels, multiplies the zeros (NaN * 0 = NaN)"""
    Ho, Wo, _ = geometry(c)
    fp = np.zeros((c["B"], Ho, Wo, c["Cout"]), bool)
    if op == "x":
        b, iy, ix, ch = idx
        opg, cpg = c["Cout"] // c["groups"], c["Cin"] // c["groups"]
        g = ch // cpg
        for oy, ox in readers_of_pixel(c, iy, ix):
            fp[b, oy, ox, g * opg:(g + 1) * opg] = True
    else:
        n, ky, kx, _ = idx
        for oy, ox in ([(slice(None), slice(None))] if padding_multiplies else readers_of_tap(c, ky, kx)):
            fp[:, oy, ox, n] = True
    fp = to_y_layout(fp, c["out_mode"])
    if mask is not None:
        fp &= np.asarray(mask) > 0
    return fp


def poisons(c):
    """[(why, "x" | "w", index)]: every position of the case; the values are FP32_POISONS or SPLIT_POISONS, by the format of the operand"""
    return [(why, "x", i) for why, i in x_positions(c)] + [(why, "w", i) for why, i in w_positions(c)]


# ---- the in-range edge --------------------------------------------------------------------------------------------------------------
# one case per kernel name: the first in the order of CASES
EDGE_CASES = list({c["kernel"]: c for c in reversed(GUARD_CASES)}.values())[::-1]


def edge_operands(c):
    """the class I operands of the case with one element of x at +65504 and another at -65504.  Where y is written as split rows a product
    of 65504 with a weight of 2, or with a scale of 2, would itself leave the range (that is the producer side, tested on its own): there
    the weights that multiply the two elements are thinned to a single +-1 in a column whose scale is +-0.5."""
    d = dict(operands(c, "I"))
    rng = _rng(c, "edge")
    x, w = d["x"].copy(), d["w"].copy()
    xs = x_positions(c)
    (_, p_hi), (_, p_lo) = xs[0], xs[-1]                 # row 0 at the first channel, the last (or an interior) row at the last channel
    assert p_hi != p_lo
    x[p_hi], x[p_lo] = F16_MAX, -F16_MAX
    if c["fmt"] & Y_SPLIT:
        assert d["scale"] is not None
        cpg, opg = c["Cin"] // c["groups"], c["Cout"] // c["groups"]
        for b, iy, ix, ch in (p_hi, p_lo):
            g, cc = ch // cpg, ch % cpg
            cols = [n for n in range(g * opg, (g + 1) * opg) if abs(d["scale"][n]) == 0.5]
            assert cols, "no column of scale +-0.5 in the group"
            n0 = int(rng.choice(cols))
            w[g * opg:(g + 1) * opg, :, :, cc] = 0
            w[n0, :, :, cc] = rng.choice(np.array([-1.0, 1.0], np.float32), size=w.shape[1:3])
    d["x"], d["w"] = x, w
    return d, (p_hi, p_lo)


def edge_reference(c, d, check=True):
    return reference(c, "I", d, check=check)


__all__ = ["GUARD_CASES", "GUARD_IDS", "F32_FROM_F16X3_CTX", "UNREACHED", "FP32_POISONS", "SPLIT_POISONS", "EDGE_CASES", "poisons", "footprint",
           "edge_operands", "edge_reference", "w_window_index", "y_shape"]
