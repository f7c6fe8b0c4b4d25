"""CPU checks of the exact-operand oracle (tests/gemm_exact_ref.py) and of the case tables of tests/test_conv_exact_gpu.py and
tests/test_wgrad_exact_gpu.py, without a GPU:

- the references agree with torch's float64 conv2d / its autograd on every GEOMETRY the GPU cases use (kernel size, stride, pad, groups, epilogue
  options), on tensors shrunk to at most 12 x 12 pixels and a few channels -- not at the case shapes themselves;
- every case's operands meet the exactness conditions (the references assert them: every intermediate an fp32 value, a split output a
  split-row value, sum |x||w| < 2^24) and the plan gives the kernel and epilogue the case names;
- SENSITIVITY: for every GPU case and its data, a reference with one seeded defect -- a border tap treated as inside, the last 32-channel
  K-step dropped, the last pixel row dropped, ky and kx swapped, one cross term dropped (class L), the residual of the last N tile dropped --
  differs from the true one in at least one output: the data would show that defect in a kernel."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_exact_ref as R      # noqa: E402
import test_conv_exact_gpu as TC      # noqa: E402
import test_wgrad_exact_gpu as TW      # noqa: E402


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


def _conv_geometries():
    seen = {}
    for c in TC.CASES:
        key = (c["KH"], c["KW"], c["stride"], c["pad"], c["groups"], c["res_mode"], c["out_mode"], bool(c["relu"]), bool(c["mask"]), min(c["H"], 12), min(c["W"], 12))
        seen.setdefault(key, c)
    return list(seen.values())


@pytest.mark.parametrize("c", _conv_geometries(), ids=lambda c: c["name"])
def test_conv_ref_agrees_with_torch(c):
    """every distinct geometry / epilogue of the case table on a small tensor of general (not exact-class) float64 operands"""
    rng = np.random.default_rng(1)
    B, H, W = min(c["B"], 2), min(c["H"], 12), min(c["W"], 12)
    if c["res_mode"] == 2:      # even output size
        ho, wo = R.out_hw(H, W, c["KH"], c["KW"], c["stride"], c["pad"])
        H, W = H - (ho % 2) * c["stride"], W - (wo % 2) * c["stride"]
    groups = c["groups"]
    Cin, Cout = (c["Cin"], c["Cout"]) if groups > 1 else (min(c["Cin"], 8), min(c["Cout"], 12) // 4 * 4 if c["out_mode"] == 1 else min(c["Cout"], 10))
    x = rng.standard_normal((B, H, W, Cin))
    w = rng.standard_normal((Cout, c["KH"], c["KW"], Cin // groups))
    Ho, Wo = R.out_hw(H, W, c["KH"], c["KW"], c["stride"], c["pad"])
    sc, sh = rng.standard_normal(Cout), rng.standard_normal(Cout)
    res = None if not c["res_mode"] else rng.standard_normal((B, Ho, Wo, Cout) if c["res_mode"] == 1 else (B, Ho // 2, Wo // 2, Cout))
    yshape = {0: (B, Ho, Wo, Cout), 1: (B, 2 * Ho, 2 * Wo, Cout // 4), 2: (B, 2 * Ho, 2 * Wo, Cout)}[c["out_mode"]]
    mask = rng.standard_normal(yshape) if c["mask"] else None
    s = R.conv_sum(x, w, c["stride"], c["pad"], groups)
    t = F.conv2d(_nchw(x), _nchw(w), stride=c["stride"], padding=c["pad"], groups=groups)
    assert np.abs(s - t.permute(0, 2, 3, 1).numpy()).max() < 1e-12
    # the epilogue, in torch: affine, residual (res_mode 2: nearest x2), ReLU, the deconv / stride-2 scatter, the mask
    t = t * torch.from_numpy(sc).view(1, -1, 1, 1) + torch.from_numpy(sh).view(1, -1, 1, 1)
    if c["res_mode"]:
        r = _nchw(res)
        t = t + (F.interpolate(r, scale_factor=2, mode="nearest") if c["res_mode"] == 2 else r)
    if c["relu"]:
        t = F.relu(t)
    if c["out_mode"] == 1:      # channels ordered (ky, kx, co) = pixel_shuffle's (co, ky, kx) after a permutation
        C2 = Cout // 4
        t = F.pixel_shuffle(t.view(B, 2, 2, C2, Ho, Wo).permute(0, 3, 1, 2, 4, 5).reshape(B, Cout, Ho, Wo), 2)
    elif c["out_mode"] == 2:
        z = torch.zeros(B, Cout, 2 * Ho, 2 * Wo, dtype=torch.float64)
        z[:, :, ::2, ::2] = t
        t = z
    t = t.permute(0, 2, 3, 1).numpy()
    if mask is not None:
        t = np.where(mask > 0, t, 0.0)
    got = R.conv_ref(x, w, sc, sh, res, mask, stride=c["stride"], pad=c["pad"], groups=groups, relu=bool(c["relu"]), res_mode=c["res_mode"],
                     out_mode=c["out_mode"], check=False)
    assert got.shape == yshape and np.abs(got - t).max() <= 2e-6 * max(1.0, np.abs(t).max())      # conv_ref returns float32


def test_deconv_order_is_conv_transpose2d():
    """out_mode 1 with w ordered (ky, kx, co) is torch's ConvTranspose2d 2x2 stride 2"""
    rng = np.random.default_rng(2)
    B, H, W, Cin, C2 = 2, 3, 5, 6, 4
    x = rng.standard_normal((B, H, W, Cin))
    wt = rng.standard_normal((Cin, C2, 2, 2))                    # torch layout [Cin][C2][ky][kx]
    w = wt.transpose(2, 3, 1, 0).reshape(4 * C2, 1, 1, Cin)      # [(ky, kx, co)][1][1][Cin]
    want = F.conv_transpose2d(_nchw(x), torch.from_numpy(wt), stride=2).permute(0, 2, 3, 1).numpy()
    got = R.conv_ref(x, w, out_mode=1, check=False)
    assert np.abs(got - want).max() < 1e-5


@pytest.mark.parametrize("shape", TW.SHAPES, ids=[s[0] for s in TW.SHAPES])
def test_wgrad_ref_agrees_with_torch_autograd(shape):
    _, B, H, W, Cin, Cout, k, s, p = shape
    rng = np.random.default_rng(3)
    Cin, Cout = 8, 12
    x = rng.standard_normal((B, H, W, Cin))
    Ho, Wo = R.out_hw(H, W, k, k, s, p)
    dy = rng.standard_normal((B, Ho, Wo, Cout))
    wt = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(_nchw(x), wt, stride=s, padding=p).backward(_nchw(dy))
    got = R.wgrad_sum(x, dy, k, k, s, p)
    assert np.abs(got - wt.grad.permute(0, 2, 3, 1).numpy()).max() < 1e-10


def test_grouped_wgrad_ref_agrees_with_torch_autograd():
    rng = np.random.default_rng(5)
    B, H, W, Cw = 2, 7, 9, 128
    for cpg in (8, 64):
        for stride in (1, 2):
            x = rng.integers(-2, 3, (B, H, W, Cw)).astype(np.float32)
            Ho, Wo = R.out_hw(H, W, 3, 3, stride, 1)
            dy = rng.integers(-2, 3, (B, Ho, Wo, Cw)).astype(np.float32)
            wt = torch.zeros(Cw, cpg, 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(_nchw(x), wt, stride=stride, padding=1, groups=Cw // cpg).backward(_nchw(dy))
            win, inside = R.grouped_wgrad_ref(x, dy, 3, 3, cpg, stride=stride, pad=1)
            want = R.group_window_weights(wt.grad.permute(0, 2, 3, 1).numpy(), cpg)
            assert np.array_equal(win, want) and inside.sum() == Cw * 9 * cpg and not win[~inside].any()


def test_dgrad_weights_ref_gives_the_data_gradient():
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((1, 5, 7, 4))).double().permute(0, 3, 1, 2).requires_grad_(True)
    w = rng.standard_normal((6, 3, 3, 4)).astype(np.float32)
    dy = rng.standard_normal((1, 5, 7, 6))
    F.conv2d(x, _nchw(w), padding=1).backward(_nchw(dy))
    got = R.conv_sum(dy, R.dgrad_weights_ref(w), 1, 1)
    assert np.abs(got - x.grad.permute(0, 2, 3, 1).numpy()).max() < 1e-10


def test_class_l_splits_exactly_away_from_a_binade_edge():
    rng = np.random.default_rng(0)
    v = R.class_l_low(rng, (4096,))
    bits = R.split_rows_ref(v.reshape(-1, 32))
    assert np.array_equal(R.unsplit_rows_ref(bits).reshape(-1), v)
    assert np.float16(np.float32(4.0 - 3.0 / 2048.0)) != np.float16(4.0)      # why h = 4 is not in the set: the low half would not be l


@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c["name"])
def test_conv_case_selects_its_kernel_is_exact_and_shows_every_defect(c):
    import conv_plan_table as T
    inputs, switches = TC.plan_inputs(c)
    chosen = T.plan(inputs, switches)
    assert (chosen[0], chosen[1]) == (c["kernel"], c["epi"]), chosen
    M = c["B"] * np.prod(R.out_hw(c["H"], c["W"], c["KH"], c["KW"], c["stride"], c["pad"]))
    assert c["kernel"] in ("C64_PATCH", "C64_PATCH_DIAG", "PATCH256") or M % 128 != 0, "a ragged last tile"
    for cls in c["classes"]:
        d = TC.operands(c, cls)
        true = TC.reference(c, cls, d)            # asserts the representability conditions
        assert true.shape == TC.y_shape(c)
        for defect in TC.applicable_defects(c, cls):      # every defect on the data of every class
            bad = TC.reference(c, cls, d, defect=defect, check=False)
            assert not np.array_equal(bad.view(np.int32), true.view(np.int32)), f"{c['name']} [{cls}]: the data would not show '{defect}'"


@pytest.mark.parametrize("t", TC.TAIL_CASES, ids=lambda t: t[0])
def test_tail_case_is_exact_and_shows_every_defect(t):
    for cls in t[6]:
        d = TC.tail_operands(t[0], cls)
        true = TC.tail_reference(d, cls)
        for defect in ["border_tap", "last_kstep", "last_row", "swap_kykx", "res_last_ntile"] + (["cross_term"] if cls != "I" else []):
            bad = TC.tail_reference(d, cls, defect=defect, check=False)
            assert not np.array_equal(bad.view(np.int32), true.view(np.int32)), (t[0], cls, defect)


def test_wgrad_shapes_have_the_slab_counts_they_are_meant_for():
    for name, B, H, W, Cin, Cout, k, s, p in TW.SHAPES:
        Ho, Wo = R.out_hw(H, W, k, k, s, p)
        M, Kp = B * Ho * Wo, k * k * Cin
        assert name.endswith(f"_m{M}")
        if TW.SLABS[name] is None:
            assert not TW.ring_shape(Cout, Cin, Kp)
            continue
        assert TW.ring_shape(Cout, Cin, Kp) and R.wgrad_slab_counts(M, Cout, Kp) == TW.SLABS[name]
    by_geom = {}
    for name, (a, b) in ((n, v) for n, v in TW.SLABS.items() if v):
        by_geom.setdefault(name.split("_m")[0], []).append((int(name.split("_m")[1]), a, b))
    for geom, rows in by_geom.items():
        assert any(M < 256 and a == 1 for M, a, b in rows) and any(M % 32 for M, a, b in rows) and any(M >= 512 and a > 1 and b > 1 for M, a, b in rows)
    assert all(a != b for g in ("3x3", "1x1s2") for M, a, b in by_geom[g] if M >= 512)
    # 2x2 stride 2: K' = 4 Cin is a multiple of 512, half the tiles in rounds of half the size -- the counts agree whatever M
    assert all(R.wgrad_slab_counts(M, 256, 512)[0] == R.wgrad_slab_counts(M, 256, 512)[1] for M in range(513, 6000, 7))


@pytest.mark.parametrize("shape", TW.SHAPES, ids=[s[0] for s in TW.SHAPES])
def test_wgrad_case_is_exact_and_shows_every_defect(shape):
    _, B, H, W, Cin, Cout, k, s, p = shape
    for cls in TW.CLASSES:
        d = TW.operands(shape[0], cls)
        for v in TW.variants_for(cls):
            TW.variant_reference(shape, cls, v, d)      # asserts the representability conditions of every call
        v = next(q for q in TW.VARIANTS if q["name"] == "f16x3<1,0,1>")
        true = TW.variant_reference(shape, cls, v, d)["g"]
        defects = ["last_kstep", "last_row"] + (["border_tap"] if p else []) + (["swap_kykx"] if k > 1 else []) + (["cross_term"] if cls != "I" else [])
        for defect in defects:      # every defect on the data of every class
            bad = TW.variant_reference(shape, cls, v, d, defect=defect, check=False)["g"]
            assert not np.array_equal(bad.view(np.int32), true.view(np.int32)), (shape[0], cls, defect)


def test_grouped_wgrad_cases_are_exact_and_show_every_defect():
    for cpg in (8, 16, 32, 64):
        for stride, _, _ in TW.GROUPED_GEOMS:
            d = TW.grouped_operands(cpg, stride)
            for dy_shift in (0, 16):
                true, inside = TW.grouped_reference(cpg, stride, dy_shift, d)
                for defect in ("border_tap", "last_kstep", "last_row", "swap_kykx"):
                    bad, _ = TW.grouped_reference(cpg, stride, dy_shift, d, defect=defect, check=False)
                    assert not np.array_equal(bad.view(np.int32), true.view(np.int32)), (cpg, stride, dy_shift, defect)
