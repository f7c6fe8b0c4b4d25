"""RoIAlign backward on the device (train_bwd.hip: roi_bwd_meta_kernel + roi_align_bwd_tile_kernel, and the float-atomic roi_align_bwd_kernel)
against the NumPy references of tests/scatter_ref.py.

No tolerance here is measured.  The owner-computes (tile) path sums in a documented order: it must equal roi_align_bwd_ref bit for bit on
every case.  On NARROW cases (scatter_ref.narrow_premise asserts the class from the inputs) every order of every sum is exact, so the tile
kernel AND the atomic kernel must equal the float64 sum bit for bit.  On WIDE cases the atomic kernel, whose order is not fixed, must lie
within n * 2^-24 * sum |terms| of the float64 sum per cell: three roundings per term (w = wy * wx, g * inv, their product) and one per
addition; the preset cell is one of the terms, n = the terms + 2.  The worst error / bound ratio is printed, not tuned.

Every map lies between two bands of a sentinel that must come back untouched.

What the rules of a path forbid (listed, not skipped silently): the tile path exists for C = 256 and P <= 16 only, so the C = 4 / 64 / 320
cases, P = 17 and the tap-by-tap cases (C = 64) run the atomic kernel alone; P = 17 reaches it with the debug switch off.  The atomic kernel
adds -0 + -0 = -0 where the tile path stores +0, so presets with -0.0 go to the tile path only."""
import ctypes as C

import numpy as np
import pytest
import torch

import scatter_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENTINEL = 0x7FA5A5A5      # a NaN pattern no kernel writes
U = 2.0 ** -24

_CASES = {}
_WANT = {}                 # (case, init, which) -> reference result: computed once, shared by the paths and tests, never modified


def cases():
    if not _CASES:
        _CASES.update(S.roi_cases())
    return _CASES


CASE_NAMES = ("edge-p7", "empty-only", "maps-ragged-p7", "maps-ragged-p14", "maps-ragged-wide", "maps-multiples-p7", "maps-multiples-p14",
              "maps-multiples-wide", "tile-ownership", "whole-p5-one-bin", "whole-p5-bins-of-8", "bin-slots-p14-narrow", "bin-slots-p14-wide",
              "bin-slots-p15-narrow", "bin-slots-p15-wide", "bin-slots-p16-narrow", "bin-slots-p16-wide", "bin-slots-p17-narrow", "bin-slots-p17-wide",
              "p1", "p1-wide", "130-rois-one-tile-narrow", "130-rois-one-tile-wide", "image-without-rois", "batch-idx-none", "wide-p7", "wide-p14",
              "same-box-100", "c4", "c64", "c320", "taps-128-y", "taps-280px-y", "taps-128-x", "taps-280px-x")
ATOMIC_ONLY = ("bin-slots-p17-narrow", "bin-slots-p17-wide", "c4", "c64", "c320", "taps-128-y", "taps-280px-y", "taps-128-x", "taps-280px-x")


def _lib():
    from ampis_amd import _lib as M
    L = M.lib()
    vp, i = C.c_void_p, C.c_int
    L.amp_debug_roi_align_bwd.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, i, i, vp, i, i]
    L.amp_debug_roi_align_bwd.restype = i
    L.amp_debug_set_roi_bwd_atomics.argtypes = [i]
    L.amp_debug_set_roi_bwd_atomics.restype = None
    return L


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.astype(F32, copy=False).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, (what, f"{bad.size} of {g.size} words differ", bad[:6].tolist(), g.reshape(-1)[bad[:6]].tolist(), w.reshape(-1)[bad[:6]].tolist())


def exact_f32(x64):
    x32 = np.asarray(x64, np.float64).astype(F32)
    assert np.array_equal(x32.astype(np.float64), x64)
    return x32


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.float32, np.uint32):
        return torch.from_numpy(a.view(np.int32)).to(DEV).view(torch.float32)
    return torch.from_numpy(a).to(DEV)


def run(ctx, c, presets, atomics, init=0, B=None, entry="debug"):
    """One call on maps preset to `presets` (float32 or uint32 patterns), each between sentinel bands; the bands are checked, the maps returned
    as uint32.  entry 'ops': ampis_amd.ops.roi_align_bwd (the public entry, init = 0)."""
    from ampis_amd import ops
    from ampis_amd._lib import check
    L = _lib()
    bufs, views = [], []
    for p in presets:
        n = p.size
        g = max(4 * p.shape[2] * p.shape[3], 4096)                  # four map rows: more than a tile beyond either end
        buf = torch.full((g + n + g,), SENTINEL, dtype=torch.int32, device=DEV)
        buf[g:g + n] = torch.from_numpy(bits(p).view(np.int32).reshape(-1)).to(DEV)
        bufs.append((buf, g, n))
        views.append(buf[g:g + n].view(torch.float32).view(*p.shape))
    R = len(c["rois"])
    rois = dev(c["rois"]) if R else torch.zeros(0, 4, device=DEV)
    dout = dev(c["dout"]) if R else torch.zeros(0, c["P"], c["P"], c["C"], device=DEV)
    bidx = None if c["bidx"] is None else dev(c["bidx"])
    B = c["B"] if B is None else B
    L.amp_debug_set_roi_bwd_atomics(int(atomics))
    try:
        if entry == "ops":
            assert not init
            ops.roi_align_bwd(ctx, views, S.STRIDES, rois, bidx, c["P"], dout, B=B)
        else:
            i4 = C.c_int * 4
            ptrs = (C.c_void_p * 4)(*[v.data_ptr() for v in views])
            check(L.amp_debug_roi_align_bwd(ctx.handle, ptrs, i4(*[v.shape[1] for v in views]), i4(*[v.shape[2] for v in views]), i4(*S.STRIDES), c["C"],
                                            rois.data_ptr() if R else None, None if bidx is None else bidx.data_ptr(), R, c["P"],
                                            dout.data_ptr() if R else None, int(B), int(init)), "amp_debug_roi_align_bwd")
        torch.cuda.synchronize()
    finally:
        L.amp_debug_set_roi_bwd_atomics(0)
    out = []
    for (buf, g, n), p in zip(bufs, presets):
        h = buf.cpu().numpy().view(np.uint32)
        assert (h[:g] == SENTINEL).all() and (h[g + n:] == SENTINEL).all(), (c["name"], "a sentinel band was written")
        out.append(h[g:g + n].reshape(p.shape))
    return out


def within(got, ref64, bound, what):
    err = np.abs(got.view(F32).astype(np.float64) - ref64)
    ratio = float((err / np.maximum(bound, 1e-300)).max(initial=0.0))
    print(f"{what}: worst error / bound = {ratio:.3g}")
    assert (err <= bound).all(), (what, float(err.max()), ratio)


def atomic_bound(c, presets, taps_per_bin=1):
    """(float64 sums with the preset as one term, bound per cell) -- n = terms + 2, terms = the bins of non-zero weight (x the taps a bin can
    land on one cell in the tap-by-tap branch) + the preset"""
    sums = S.roi_align_bwd_sum64([m.shape for m in presets], c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])
    out = []
    for m, (s, sa, cnt) in zip(presets, sums):
        m64 = m.astype(np.float64)
        n = (taps_per_bin * cnt + 1 + 2)[..., None]
        out.append((m64 + s, n * U * (sa + np.abs(m64))))
    return out


def check_case(ctx, c, path, init=0, presets=None, B=None, entry="debug"):
    atomics = path == "atomic"
    presets = c["maps"] if presets is None else presets
    base = [np.zeros_like(m) for m in c["maps"]] if init else c["maps"]       # what the result is a function of
    got = run(ctx, c, presets, atomics, init=init, B=B, entry=entry)
    what = f"{c['name']} {path}{' init' if init else ''}"
    memo = presets is c["maps"] or bool(init)
    if c["cls"] == "narrow":
        key = (c["name"], bool(init), "f64")
        if not (memo and key in _WANT):
            _WANT[key] = [exact_f32(w) for w in S.narrow_premise(base, c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])]
        want = _WANT[key]
        for l in range(4):
            same_bits(got[l], want[l], f"{what} p{l + 2} against float64")
    if path == "tile":
        key = (c["name"], bool(init), "ref")
        if not (memo and key in _WANT):
            _WANT[key] = S.roi_align_bwd_ref(base, c["rois"], c["bidx"], c["P"], c["levels"], c["dout"], init=bool(init))
        want = _WANT[key]
        for l in range(4):
            same_bits(got[l], want[l], f"{what} p{l + 2} against roi_align_bwd_ref")
    elif c["cls"] == "wide":
        taps = 1
        if c.get("taps"):       # samples one cell apart: a cell is the lower tap of one sample and the upper tap of the one before, on each axis
            ys, xs = S.PR.roi_samples(c["rois"][0], 1, 4, *c["hw"][0])
            assert np.all(np.diff(ys[0]) == 1) and np.all(np.diff(xs[0]) == 1)
            taps = 4
        for l, (ref64, bound) in enumerate(atomic_bound(c, base, taps)):
            within(got[l], ref64, bound, f"{what} p{l + 2} against float64")
    return got


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case(gpu_ctx, name):
    """every case on every path its rules allow, accumulating into a preset map (small integers / randn)"""
    c = cases()[name]
    assert (c["C"] != 256 or c["P"] > 16 or c.get("taps", False)) == (name in ATOMIC_ONLY)
    if name not in ATOMIC_ONLY:
        got = check_case(gpu_ctx, c, "tile")
        if c.get("unchanged"):
            for l in range(4):
                same_bits(got[l], c["maps"][l], "the empty RoIs leave the map as preset")
        check_case(gpu_ctx, c, "atomic")
    else:
        # P = 17 reaches the atomic kernel by the dispatch rule, the switch off; the others too (C != 256)
        check_case(gpu_ctx, c, "atomic" if c["P"] <= 16 and c["C"] == 256 else "dispatch")


def test_empty_rois_leave_every_bit_pattern(gpu_ctx):
    """the wholly-outside, zero-area, inverted and NaN RoIs alone: maps of arbitrary bit patterns (-0.0, NaN payloads) come back as they were"""
    c = cases()["empty-only"]
    rng = np.random.default_rng(5)
    presets = [rng.integers(0, 2 ** 32, m.shape, dtype=np.uint32) for m in c["maps"]]
    presets[0].reshape(-1)[::7] = 0x80000000
    for path in ("tile", "atomic"):
        got = run(gpu_ctx, c, presets, path == "atomic")
        for l in range(4):
            same_bits(got[l], presets[l], f"empty-only {path} p{l + 2}")


def test_negative_zero_presets_on_the_tile_path(gpu_ctx):
    """a touched tile turns a stored -0.0 into +0.0 (fl(-0 + +0)), an untouched tile keeps it: roi_align_bwd_ref models both"""
    c = cases()["tile-ownership"]
    presets = [m.copy() for m in c["maps"]]
    for m in presets:
        m.reshape(-1)[::3] = F32(-0.0)
    want = S.roi_align_bwd_ref(presets, c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])
    nz = lambda a: int((bits(a) == 0x80000000).sum())
    assert 0 < nz(want[0]) < nz(presets[0])                # some -0.0 lie under touched tiles, some do not
    got = run(gpu_ctx, c, presets, 0)
    for l in range(4):
        same_bits(got[l], want[l], f"-0.0 presets p{l + 2}")


@pytest.mark.parametrize("name", ["edge-p7", "maps-ragged-p7", "image-without-rois", "wide-p14", "bin-slots-p16-wide", "130-rois-one-tile-narrow"])
def test_init_writes_every_cell(gpu_ctx, name):
    """init = 1, the mode the training step uses: maps of 0xffffffff, every cell written, +0 bits where nothing reaches; on the tile path and
    on the atomic path (a zero fill, then the atomics)"""
    c = cases()[name]
    presets = [np.full(m.shape, 0xffffffff, np.uint32) for m in c["maps"]]
    for path in ("tile", "atomic"):
        got = check_case(gpu_ctx, c, path, init=1, presets=presets)
        sums = S.roi_align_bwd_sum64([m.shape for m in presets], c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])
        for l in range(4):
            nothing = sums[l][2] == 0
            assert (got[l][nothing] == 0).all(), (name, path, l, "a cell no RoI reaches is not +0")


def test_init_without_rois(gpu_ctx):
    c = dict(cases()["maps-ragged-p7"])
    c.update(rois=c["rois"][:0], bidx=c["bidx"][:0], dout=c["dout"][:0], levels=c["levels"][:0])
    presets = [np.full(m.shape, 0xffffffff, np.uint32) for m in c["maps"]]
    for path in ("tile", "atomic"):
        got = run(gpu_ctx, c, presets, path == "atomic", init=1)
        assert all((g == 0).all() for g in got), path
    got = run(gpu_ctx, c, presets, 0, init=0)                    # and without init nothing is written
    assert all((g == 0xffffffff).all() for g in got)


def test_two_calls_as_the_model_issues_them(gpu_ctx):
    """P = 14 with init (the mask head's RoIs), then P = 7 accumulating into the result (the box head's)"""
    c14, c7 = cases()["wide-p14"], cases()["wide-p7"]
    presets = [np.full(m.shape, 0xffffffff, np.uint32) for m in c14["maps"]]
    first = run(gpu_ctx, c14, presets, 0, init=1)
    want1 = S.roi_align_bwd_ref(c14["maps"], c14["rois"], c14["bidx"], 14, c14["levels"], c14["dout"], init=True)
    second = run(gpu_ctx, c7, [f.view(F32) for f in first], 0)
    want2 = S.roi_align_bwd_ref(want1, c7["rois"], c7["bidx"], 7, c7["levels"], c7["dout"])
    for l in range(4):
        same_bits(first[l], want1[l], f"first call p{l + 2}")
        same_bits(second[l], want2[l], f"second call p{l + 2}")


@pytest.mark.parametrize("name", ["wide-p7", "image-without-rois", "batch-idx-none"])
def test_public_entry_and_derived_image_count(gpu_ctx, name):
    """ops.roi_align_bwd (amp_roi_align_bwd_batched) with B passed and with B = 0 (derived from batch_idx: 1 + its maximum)"""
    c = cases()[name]
    for B in (c["B"], 0):
        check_case(gpu_ctx, c, "tile", B=B, entry="ops")
