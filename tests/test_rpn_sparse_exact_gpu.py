"""The sparse backward pass of the RPN head on the device (rpn_sparse.hip: seven kernels and three GEMM calls) through the test entry
amp_debug_rpn_sparse_backward, against the references of tests/scatter_ref.py.

No tolerance.  NARROW operands (gemm_exact_ref's classes: class I integers for d_pred * 2^16, W_pred, W_conv and the scale, class L for the
features and t, so the low half of the split rows is live) make every sum of the pass exact in both convolution arithmetics and in any order
-- scatter_ref.rpn_sparse_ref asserts that from the inputs -- so rows, nrows, the four parameter gradients, the five d_feat maps and the
workspace rows (d_pred, activations, d_t, the gathered patches) must equal the dense float64 reference bit for bit.  On WIDE randn data the row
kernels and the head sums, whose order is fixed, must equal their fp32 restatements bit for bit; the two GEMM outputs are compared on narrow
data only (their arithmetic is held by test_conv_exact_gpu.py; here the gather, the wiring, the shift and the scatter are under test).

The test allocates the workspace itself at exactly the sizes common.h documents; every output and workspace buffer lies between sentinel
bands that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import scatter_ref as S
from bwd_glue_ref import split_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENTINEL = 0x7FA5A5A5
BAND = 4096
HID = 256
F32_MODE, F16X3_MODE = 0, 1

_CASES, _REF = {}, {}
CASE_NAMES = ("one-pixel-all-anchors", "borders-and-1x1-levels", "adjacent-pixels", "same-pixel-levels-images", "invalid-entries-and-overfull", "batch-1",
              "batch-1-three-images", "a5-batch-256", "a9-batch-512", "a9-k45-one-image", "no-scale", "recompute", "recompute-shift", "recompute-wsplit",
              "recompute-wsplit-shift", "recompute-no-scale", "wide-a3", "wide-a9")


def case(name):
    if not _CASES:
        _CASES.update(S.sparse_cases())
    return _CASES[name]


def ref(name):
    """the dense float64 reference of a case (its NARROW premises asserted from the inputs), computed once and left unchanged"""
    if name not in _REF:
        _REF[name] = S.sparse_ref_of(case(name))
    return _REF[name]


vp, ci = C.c_void_p, C.c_int


class Args(C.Structure):          # amp_debug_rpn_sparse_args
    _fields_ = [("B", ci), ("batch", ci), ("ld", ci), ("K", ci), ("C", ci), ("A", ci), ("fh", ci * 5), ("fw", ci * 5), ("sampled", vp), ("counts", vp),
                ("dpred", vp * 5), ("t", vp * 5), ("feat", vp * 5), ("t_split", ci), ("feat_split", ci), ("recompute_t", ci),
                ("w_conv_split", vp), ("conv_shift", vp), ("w_pred", vp), ("w_conv", vp), ("conv_scale", vp),
                ("gw_pred", vp), ("gb_pred", vp), ("gw_conv", vp), ("gb_conv", vp), ("dfeat", vp * 5), ("rows", vp), ("nrows", vp),
                ("dpred_rows", vp), ("act_rows", vp), ("dt_rows", vp), ("xg", vp), ("G", vp), ("wt", vp), ("G_floats", C.c_size_t),
                ("wg_scratch", vp), ("wg_scratch_floats", C.c_size_t)]


def _lib():
    from ampis_amd import _lib as M
    L = M.lib()
    L.amp_debug_rpn_sparse_backward.argtypes = [vp, C.POINTER(Args)]
    L.amp_debug_rpn_sparse_backward.restype = ci
    L.amp_conv_wgrad_scratch_floats.argtypes = [C.POINTER(M.ConvDesc)]
    L.amp_conv_wgrad_scratch_floats.restype = C.c_size_t
    L.amp_set_conv_mode.argtypes = [vp, ci]
    L.amp_get_conv_mode.argtypes = [vp]
    return L, M


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.astype(F32, copy=False).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, f"{bad.size} of {g.size} words differ", bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


def exact_f32(x64):
    x32 = np.asarray(x64, np.float64).astype(F32)
    assert np.array_equal(x32.astype(np.float64), x64)
    return x32


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.float32, np.uint32):
        return torch.from_numpy(a.view(np.int32)).to(DEV)
    return torch.from_numpy(a).to(DEV)


class Guarded:
    """n 32-bit words between two sentinel bands; the inside preset to `init` or to the sentinel as well"""
    def __init__(self, n, init=None):
        self.n = int(n)
        self.buf = torch.full((BAND + self.n + BAND,), SENTINEL, dtype=torch.int32, device=DEV)
        if init is not None:
            self.buf[BAND:BAND + self.n] = dev(np.ascontiguousarray(init).reshape(-1))
        self.ptr = self.buf.data_ptr() + 4 * BAND

    def host(self, what):
        h = self.buf.cpu().numpy().view(np.uint32)
        assert (h[:BAND] == SENTINEL).all() and (h[BAND + self.n:] == SENTINEL).all(), (what, "a sentinel band was written")
        return h[BAND:BAND + self.n]


def build_args(c, t_split, feat_split, L, M):
    """(Args, the guarded outputs and workspace by name, the tensors that must stay alive)"""
    B, batch, ld, K = c["B"], c["batch"], c["ld"], c["K"]
    R = B * batch
    keep = []

    def inp(a):
        t = dev(a)
        keep.append(t)
        return t.data_ptr()

    a = Args()
    a.B, a.batch, a.ld, a.K, a.C, a.A = B, batch, ld, K, HID, c["A"]
    a.fh = (ci * 5)(*[h for h, w in c["levels"]])
    a.fw = (ci * 5)(*[w for h, w in c["levels"]])
    a.sampled, a.counts = inp(c["sampled"]), inp(c["counts"])
    a.dpred = (vp * 5)(*[inp(d) for d in c["dpred"]])
    if not c["recompute"]:          # with recompute_t the stored t is not read: null pointers
        a.t = (vp * 5)(*[inp(split_rows_ref(t) if t_split else t) for t in c["t"]])
    a.feat = (vp * 5)(*[inp(split_rows_ref(f) if feat_split else f) for f in c["feat"]])
    a.t_split, a.feat_split, a.recompute_t = int(t_split), int(feat_split), int(c["recompute"])
    a.w_conv_split = inp(split_rows_ref(c["w_conv"].reshape(HID, 9 * HID))) if c["wsplit"] else None
    a.conv_shift = None if c["shift"] is None else inp(c["shift"])
    a.conv_scale = None if c["scale"] is None else inp(c["scale"])
    a.w_pred, a.w_conv = inp(c["w_pred"]), inp(c["w_conv"])
    desc = M.ConvDesc(1, 1, R, 9 * HID, HID, 1, 1, 1, 0, 0, 0, 0)
    g_floats = max(R * 9 * HID, (ld + 2) * 32 * 256)
    wg = int(L.amp_conv_wgrad_scratch_floats(C.byref(desc)))
    out = dict(gw_pred=Guarded(K * HID), gb_pred=Guarded(K), gw_conv=Guarded(HID * 9 * HID), gb_conv=Guarded(HID), rows=Guarded(R), nrows=Guarded(B),
               dpred_rows=Guarded(R * ld), act_rows=Guarded(R * HID), dt_rows=Guarded(R * HID), xg=Guarded(R * 9 * HID), G=Guarded(g_floats),
               wt=Guarded(9 * HID * HID), wg_scratch=Guarded(wg))
    for l in range(5):
        out["dfeat%d" % l] = Guarded(c["dfeat"][l].size, c["dfeat"][l])
    for k in ("gw_pred", "gb_pred", "gw_conv", "gb_conv", "rows", "nrows", "dpred_rows", "act_rows", "dt_rows", "xg", "G", "wt", "wg_scratch"):
        setattr(a, k, out[k].ptr)
    a.dfeat = (vp * 5)(*[out["dfeat%d" % l].ptr for l in range(5)])
    a.G_floats, a.wg_scratch_floats = g_floats, wg
    return a, out, keep


def run(ctx, c, mode, t_split, feat_split, mutate=None):
    """(return code, host copies of every guarded buffer) of one call in convolution arithmetic `mode`"""
    L, M = _lib()
    a, out, keep = build_args(c, t_split, feat_split, L, M)
    if mutate:
        mutate(a)
    before = L.amp_get_conv_mode(ctx.handle)
    assert L.amp_set_conv_mode(ctx.handle, mode) == 0 and L.amp_get_conv_mode(ctx.handle) == mode
    try:
        rc = L.amp_debug_rpn_sparse_backward(ctx.handle, C.byref(a))
        torch.cuda.synchronize()
    finally:
        L.amp_set_conv_mode(ctx.handle, before)
    return rc, {k: g.host(f"{c['name']} {k}") for k, g in out.items()}


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("mode", [F16X3_MODE, F32_MODE], ids=["f16x3", "f32"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case(gpu_ctx, name, mode, split):
    c, o = case(name), ref(name)
    rc, h = run(gpu_ctx, c, mode, split, split)
    assert rc == 0, rc
    B, batch, K, ld = c["B"], c["batch"], c["K"], c["ld"]
    what = f"{name} {'f16x3' if mode else 'f32'} split={split}"
    assert np.array_equal(h["rows"], o["rows"]) and np.array_equal(h["nrows"].view(np.int32), o["nrows"]), what
    t32 = [t.astype(F32) for t in o["t"]]
    dr, ar = S.rpn_gather_rows_ref(c["levels"], o["rows"], batch, c["dpred"], t32, K)
    same_bits(h["dpred_rows"], dr, what + " dpred_rows")
    same_bits(h["xg"], S.rpn_gather_x_ref(c["levels"], o["rows"], batch, c["feat"]), what + " xg")
    if c["cls"] == "narrow":
        same_bits(h["act_rows"], ar + F32(0), what + " act_rows")
        dt = np.zeros((B * batch, HID))
        for r, key in enumerate(o["rows"]):
            if key != S.NOROW:
                dt[r] = o["dt"][int(key >> 26)][r // batch, int(key & 0x3ffffff)]
        same_bits(h["dt_rows"], exact_f32(dt), what + " dt_rows")
        for k in ("gw_pred", "gb_pred", "gw_conv", "gb_conv"):
            same_bits(h[k], exact_f32(o[k]), what + " " + k)
        for l in range(5):
            same_bits(h["dfeat%d" % l], exact_f32(o["dfeat"][l]), what + f" dfeat {l}")
    else:
        same_bits(h["act_rows"], ar, what + " act_rows")
        dt = S.rpn_dt_rows_ref(dr, ar, c["w_pred"], K)
        same_bits(h["dt_rows"], dt, what + " dt_rows against rpn_dt_rows_ref")
        gw, gb, gc = S.rpn_head_sums_ref(dr, ar, dt, K)
        same_bits(h["gw_pred"], gw, what + " gw_pred against rpn_head_sums_ref")
        same_bits(h["gb_pred"], gb, what + " gb_pred against rpn_head_sums_ref")
        same_bits(h["gb_conv"], gc, what + " gb_conv against rpn_head_sums_ref")


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


REFUSALS = {"batch-513": _set(batch=513), "ld-24": _set(ld=24), "5A-above-K": _set(K=14),
            "G-one-short": lambda a: setattr(a, "G_floats", a.G_floats - 1),
            "wgrad-scratch-one-short": lambda a: setattr(a, "wg_scratch_floats", a.wg_scratch_floats - 1)}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusals_write_nothing(gpu_ctx, which):
    """the AMP_REQUIRE lines of rpn_sparse_backward: an error code, and no word of any output or workspace buffer written"""
    c = case("adjacent-pixels")
    rc, h = run(gpu_ctx, c, F16X3_MODE, 0, 0, mutate=REFUSALS[which])
    assert rc != 0, which
    for k, v in h.items():
        if k.startswith("dfeat"):
            same_bits(v, c["dfeat"][int(k[5:])], which + " " + k)
        else:
            assert (v == SENTINEL).all(), (which, k, "written by a refused call")
