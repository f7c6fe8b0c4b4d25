"""What the two GPU files of the training-forward tests share (tests/test_label_sample_exact_gpu.py, tests/test_loss_exact_gpu.py): buffers
between sentinel bands, the bit-for-bit comparison, amp_rpn_levels for a case and the C ABI with the test entry's signature."""
import ctypes as C

import numpy as np
import torch

import train_fwd_cases as Cs
import train_fwd_ref as R

DEV = "cuda:0"
F32 = np.float32
SENTINEL = 0x7FA5A5A5
BAND = 1024
AMP_OK = 0


def dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(4, a.dtype)          # a valid pointer for an empty list
    return torch.from_numpy(a.view(np.int32) if a.dtype in (np.float32, np.uint32) else a).to(DEV)


class Guarded:
    """n bytes between two sentinel bands, preset to the sentinel pattern (n a multiple of 4 after padding)"""
    def __init__(self, nbytes):
        self.words = (int(nbytes) + 3) // 4
        self.buf = torch.full((BAND + self.words + BAND,), SENTINEL, dtype=torch.int32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * BAND

    def host(self, what, dtype=np.uint32):
        h = self.buf.cpu().numpy().view(np.uint32)
        assert (h[:BAND] == SENTINEL).all() and (h[BAND + self.words:] == SENTINEL).all(), (what, "a sentinel band was written")
        return h[BAND:BAND + self.words].view(dtype)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    g, w = (R.bits(g) if g.dtype == np.float32 else g), (R.bits(w) if w.dtype == np.float32 else w)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, f"{bad.size} of {g.size} words differ", bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


def levels_of(levels, sizes, ratios, preds=None, ld=None):
    from ampis_amd import ops
    shapes = [(h, w) for h, w, _ in levels]
    custom = hasattr(sizes[0], "__len__") or tuple(ratios) != Cs.RATIOS
    lv = ops.make_rpn_levels(preds if preds is not None else [None] * 5, shapes, strides=[s for _, _, s in levels],
                             sizes=[list(s) if hasattr(s, "__len__") else [s] for s in sizes] if custom else sizes, ratios=list(ratios) if custom else None)
    if ld is not None:
        lv.ld = ld
    return lv


def _abi():
    from ampis_amd import _lib
    L = _lib.lib()
    L.amp_debug_last_rpn_sample_path.argtypes = [C.c_void_p]
    L.amp_debug_last_rpn_sample_path.restype = C.c_int
    return L
