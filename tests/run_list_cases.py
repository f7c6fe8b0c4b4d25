"""One small case set that all four mask analyses on run lists are driven with (mask_edge_distance, region properties, group overlap,
segmentation class map): they share one walk over the run lists, one plan and one bit-plane painter (ampis_amd/csrc/run_list.h), and these are
the shapes at which those can go wrong.  Heights around the 64-row word (1, 63, 64, 65, 129), widths 1, 2, 5, at most 6 masks a side, given as
RAW run lengths so that zero-length runs reach the library as they are:

  ground truths  empty | full | one pixel in the last row of a word (or of the image) in the last column | a run that wraps a column end |
                 a run that spans more than one full column | a list that starts with a zero-length run of zeros and has interior
                 zero-length runs of both kinds
  predictions    one pixel in the first row of the next word (or of the last column) | two pixels, exactly one of them the ground truths'
                 single pixel | full | empty | every other pixel

A mask that does not fit a size (a wrap needs two columns) is left out there.  Every pair is matched.  dense() decodes in numpy, apart from
the library."""
import numpy as np

from ampis_amd import rle
from ampis_amd._lib import lib

from edge_distance_cases import call_c

SIZES = [(h, w) for h in (1, 63, 64, 65, 129) for w in (1, 2, 5)]


def _spans(h, w, spans):
    """run lengths of the column-major pixel positions [s, e) of `spans` (ascending, apart), zeros first; no zero-length run but the first"""
    counts, pos = [], 0
    for s, e in spans:
        counts += [s - pos, e - s]
        pos = e
    return counts + ([h * w - pos] if pos < h * w or not counts else [])


def masks(h, w):
    """(ground truths, predictions): lists of {'size': [h, w], 'counts': uint32 run lengths}"""
    A = h * w
    edge = (w - 1) * h + min(63, h - 1)                              # the last row of a word, last column
    nxt = 64 if h > 64 else (w - 1) * h                              # the first row of the next word / of the last column
    gt = [[A], [0, A], _spans(h, w, [(edge, edge + 1)])]
    if w >= 2:
        gt.append(_spans(h, w, [(h - 1, h + 1)]))                    # the last row of column 0 and the first of column 1
    if w >= 3:
        gt.append(_spans(h, w, [(h // 2, h // 2 + 2 * h + 1)]))      # more than two columns' worth, all of column 1 inside
    if A >= 4:
        gt.append([0, 1, 0, 1, 1, 0, A - 3])                         # pixels 0 and 1 as two runs, an empty run of ones behind pixel 2
    pred = [_spans(h, w, [(nxt, nxt + 1)]), _spans(h, w, [(max(edge - 1, 0), edge + 1)]), [0, A], [A], [1] * A]
    mk = lambda c: {"size": [h, w], "counts": np.asarray(c, dtype=np.uint32)}
    return [mk(c) for c in gt], [mk(c) for c in pred]


def dense(r):
    """bool [h, w] of raw run lengths, by numpy alone"""
    h, w = r["size"]
    c = np.asarray(r["counts"], dtype=np.int64)
    flat = np.repeat(np.arange(len(c)) & 1, c).astype(bool)
    assert flat.size == h * w
    return flat.reshape(w, h).T.copy()


def pairs_and_boxes(gt, pred):
    """every (g, q) and one index box [r1, r2, c1, c2] each: the image, its lower half, its right part reaching beyond the image"""
    h, w = gt[0]["size"]
    pairs = [(g, q) for g in range(len(gt)) for q in range(len(pred))]
    kinds = [[0, h, 0, w], [h // 2, h, 0, w], [0, max(h - 1, 1), w // 2, w + 3]]
    return np.array(pairs, np.int32), np.array([kinds[k % 3] for k in range(len(pairs))], np.int32)


def run_all(gt, pred, ctx=None):
    """The four calls on one case, ctx None = the host path: a dict of name -> list of arrays (the outputs as the C ABI wrote them)."""
    h, w = gt[0]["size"]
    pairs, boxes = pairs_and_boxes(gt, pred)
    gc, pc = [m["counts"] for m in gt], [m["counts"] for m in pred]
    cap = h * w * len(pairs)
    st, fp, fpo, fn, fno = call_c(ctx, gc, pc, pairs, boxes, h, w, cap, cap)
    assert st == 0, lib().amp_last_error()
    out = {"edge": [fpo, fno, fp[: int(fpo[-1])], fn[: int(fno[-1])]]}
    out["props"] = list(rle.region_props(gt + pred, ctx=ctx))
    inter, aa, ab = rle.overlap_groups([gt, pred], [pred, gt], ctx=ctx)          # two groups in one call
    out["overlap"] = inter + aa + ab
    for mode in ("reduced", "all"):
        counts, px = rle.seg_class_map(gt, pred, pairs, mode, ctx=ctx)
        out["seg-" + mode] = counts + [px]
    return out


def same(a, b):
    return a.keys() == b.keys() and all(len(a[k]) == len(b[k]) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                                                                       for x, y in zip(a[k], b[k])) for k in a)


# ---- what the shared walk refuses, once per entry point -----------------------------------------------------------------------------------------

FAULTS = {"empty": ([], "empty"), "short": ([2, 3], "cover 5 pixels, the image has 6"), "over": ([1, 6], "more than the image's 6 pixels")}


def _mk(c):
    return {"size": [2, 3], "counts": np.asarray(c, dtype=np.uint32)}


ENTRY_POINTS = {
    "edge": lambda bad, ctx: rle.edge_distance([_mk([6])], [_mk(bad)], [(0, 0)], [[0, 2, 0, 3]], ctx=ctx),
    "props": lambda bad, ctx: rle.region_props([_mk([0, 6]), _mk(bad)], ctx=ctx),
    "overlap": lambda bad, ctx: rle.overlap_groups([[_mk([0, 6])]], [[_mk(bad)]], ctx=ctx),
    "seg": lambda bad, ctx: rle.seg_class_map([_mk(bad)], [_mk([0, 6])], [(0, 0)], "reduced", ctx=ctx),
}
