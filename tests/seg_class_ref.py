"""The independent reference of amp_seg_class_map: a dense NumPy restatement of the definition (ampis/analyze.py:631-682) -- decode every mask
of a pair with rle.decode, OR g & q, g & ~q, ~g & q over the pairs, code = TP + 2 FN + 4 FP, one bool image per class, rle.encode of the
Fortran-ordered array.  It shares no code with the run-domain / bit-plane implementation (mask_analysis_host.hip, seg_class_map.hip); every comparison
against it is exact.  The planes are built pair by pair, so the reference needs three images whatever the number of pairs."""
import numpy as np

from ampis_amd import rle

LABELS = {"reduced": ["TP", "FN", "FP", "other"], "all": ["TP", "FN", "TP+FN", "FP", "TP+FP", "FN+FP", "TP+FN+FP"]}


def planes(gt, pred, pairs, size):
    h, w = size
    tp, fn, fp = (np.zeros((h, w), bool) for _ in range(3))
    for g, q in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        a, b = rle.decode(gt[g]).astype(bool), rle.decode(pred[q]).astype(bool)
        tp |= a & b
        fn |= a & ~b
        fp |= ~a & b
    return tp, fn, fp


def dense(gt, pred, pairs, mode, size):
    """(list of K uint32 run lists, int64 [8] pixel counts, the code image)"""
    tp, fn, fp = planes(gt, pred, pairs, size)
    code = tp.astype(np.uint8) + 2 * fn.astype(np.uint8) + 4 * fp.astype(np.uint8)
    if mode == "all":
        classes = [code == k for k in range(1, 8)]
    else:
        assert mode == "reduced"
        classes = [code == 1, code == 2, code == 4, np.isin(code, (3, 5, 6, 7))]
    counts = [rle.string_to_counts(rle.encode(np.asfortranarray(c))["counts"]) for c in classes]
    return counts, np.bincount(code.reshape(-1), minlength=8).astype(np.int64), code
