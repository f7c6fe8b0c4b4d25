"""The case table of tests/range_guard_cases.py, checked without a GPU: every poison sits where a valid output reads it (so a device
assertion "the flag is set" cannot hold vacuously), on small cases the float64 reference turns non-finite exactly on the computed
footprint, the in-range edge (+-65504) passes the reference's own exactness conditions for one case of every split kernel, and every
split-arithmetic kernel name is either launched by a flag-raising case or listed with a reason."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_exact_ref as R               # noqa: E402
import range_guard_cases as G            # noqa: E402
from test_conv_exact_gpu import CASES, operands, reference      # noqa: E402

# small cases for the footprint check: plain, strided, padded borders of a 1 x W map, both scatter forms with an output mask, grouped, the stem
FOOTPRINT_CASES = ("f16x3_64_3x3", "f16x3_64_s2", "f16x3_64_p0", "f16x3_64_1xW", "f16x3s_64_deconv", "f16x3s_64_scatter2", "f16x3s_g32",
                   "f16x3s_g32_mask", "c64_patch_diag_cpg8", "f16x3_stem", "f16x3_64_generic")


def test_the_poison_values_leave_the_range():
    with np.errstate(over="ignore"):
        assert not any(np.isfinite(np.float32(v).astype(np.float16)) for v in G.FP32_POISONS)
    assert np.isfinite(np.float32(G.F16_MAX).astype(np.float16)) and np.float32(np.nextafter(np.float32(65520.0), np.float32(0))).astype(np.float16) == G.F16_MAX
    # the producer's pairs: hi infinite or NaN, lo' = (v - hi) * 2048 -- never a finite, saturated pair
    for (hi, lo), v in zip(G.SPLIT_POISONS, G.FP32_POISONS):
        assert not np.isfinite(hi) and not np.isfinite(lo), (v, hi, lo)
    hi, lo = G.split_pair(65520.0)
    assert hi == np.inf and lo == -np.inf
    assert G.SPLIT_POISONS[-1][0] == np.inf and G.SPLIT_POISONS[-1][1] == 0


def test_the_guard_cases_are_the_split_cases():
    assert len(G.GUARD_CASES) > 50
    assert all(c["mode"] == "f16x3" and not c["force_f32"] for c in G.GUARD_CASES)
    assert {c["kernel"] for c in G.F32_FROM_F16X3_CTX} == {"MFMA_64", "GLDS_64"} and all(c["mode"] == "f16x3" for c in G.F32_FROM_F16X3_CTX)


@pytest.mark.parametrize("c", G.GUARD_CASES, ids=G.GUARD_IDS)
def test_every_poison_is_read(c):
    Ho, Wo, M = G.geometry(c)
    cpg = c["Cin"] // c["groups"]
    ps = G.poisons(c)
    xs, ws = [p for p in ps if p[1] == "x"], [p for p in ps if p[1] == "w"]
    assert len(xs) >= 2 * 2 and len(ws) == 6 and len({p[2] for p in ps if p[1] == "x"}) == len(xs)
    rows_hit = set()
    for why, op, idx in ps:
        if op == "x":
            b, iy, ix, ch = idx
            assert 0 <= b < c["B"] and 0 <= iy < c["H"] and 0 <= ix < c["W"] and 0 <= ch < c["Cin"]
            readers = G.readers_of_pixel(c, iy, ix)
            assert readers, f"{c['name']}: no output reads the pixel of [{why}]"
            rows_hit |= {(b * Ho + oy) * Wo + ox for oy, ox in readers}
        else:
            n, ky, kx, cc = idx
            assert 0 <= n < c["Cout"] and 0 <= ky < c["KH"] and 0 <= kx < c["KW"] and 0 <= cc < cpg
            assert G.readers_of_tap(c, ky, kx), f"{c['name']}: tap of [{why}] multiplies padding only"
            wi = G.w_window_index(c, idx)
            assert 0 <= wi[3] < (64 if c["groups"] > 1 else cpg)
            if c["groups"] > 1:      # the window slot holds exactly this element
                probe = np.zeros((c["Cout"], c["KH"], c["KW"], cpg), np.float32)
                probe[idx] = 1
                assert R.group_window_weights(probe, cpg)[wi] == 1
    assert 0 in rows_hit and M - 1 in rows_hit
    T = G.tile_rows(c)
    if M > T // 2 + 1:
        assert any((m % T) >= T // 2 for m in rows_hit - {0, M - 1}), "no poison in the second half of a tile"
    assert {idx[3] for _, op, idx in ps if op == "x"} >= {0, c["Cin"] - 1}
    assert {idx[0] for _, op, idx in ps if op == "w"} >= {0, c["Cout"] - 1}


@pytest.mark.parametrize("name", FOOTPRINT_CASES)
def test_reference_is_non_finite_exactly_on_the_footprint(name):
    c = next(q for q in G.GUARD_CASES if q["name"] == name)
    d = operands(c, "I")
    for why, op, idx in G.poisons(c):
        p = dict(d)
        p[op] = d[op].copy()
        p[op][idx] = np.nan
        with np.errstate(invalid="ignore"):
            got = ~np.isfinite(reference(c, "I", p, check=False))
        want = G.footprint(c, op, idx, d["mask"], padding_multiplies=True)
        assert want.shape == got.shape
        assert np.array_equal(got, want), f"{name} [{why}]: the reference is non-finite at {int(got.sum())} outputs, the footprint has {int(want.sum())}"
        # the reading rule is the stricter one: outputs whose window holds the element inside the map
        read = G.footprint(c, op, idx)
        assert read.any() and not (read & ~G.footprint(c, op, idx, padding_multiplies=True)).any()


def test_edge_cases_cover_every_split_kernel():
    assert {c["kernel"] for c in G.EDGE_CASES} == {c["kernel"] for c in G.GUARD_CASES} and len(G.EDGE_CASES) == len({c["kernel"] for c in G.GUARD_CASES})


@pytest.mark.parametrize("c", G.EDGE_CASES, ids=[c["name"] for c in G.EDGE_CASES])
def test_in_range_edge_is_exact_in_the_reference(c):
    d, (p_hi, p_lo) = G.edge_operands(c)
    assert d["x"][p_hi] == G.F16_MAX and d["x"][p_lo] == -G.F16_MAX
    assert np.array_equal(d["x"].astype(np.float16).astype(np.float32), d["x"])      # every x is its own hi half, finite: inside the range
    want = G.edge_reference(c, d, check=True)          # raises where a sum, a rounding step or a split output is not exact
    assert np.isfinite(want).all()
    # not vacuous: without the two elements the expected output differs, and products of 65504 reach it (times a scale of 0.5 at the least;
    # the class I sums alone stay below 2 * 2 * 2 * K < 2^13)
    assert np.abs(want).max() >= 2.0 ** 14
    base = dict(d, x=operands(c, "I")["x"])
    assert not np.array_equal(want, reference(c, "I", base, check=False))


def test_every_split_kernel_is_pulled_or_listed():
    import conv_plan_table as T
    split_names = {n for n in T.kernel_names() if not n.startswith(("GLDS", "MFMA_"))}
    covered = {c["kernel"] for c in G.GUARD_CASES}
    assert covered <= split_names and set(G.UNREACHED) <= split_names and not covered & set(G.UNREACHED)
    assert not split_names - covered - set(G.UNREACHED), f"no flag-raising case launches {sorted(split_names - covered - set(G.UNREACHED))}"
    assert all(n.startswith(G.SPLIT_PREFIXES) for n in covered)
    # and the fp32 kernels are exactly what is left
    assert {c["kernel"] for c in CASES if c["kernel"] not in split_names} == {n for n in T.kernel_names() if n not in split_names}
