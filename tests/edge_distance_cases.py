"""Shared by tests/test_edge_distance.py and tests/test_edge_distance_gpu.py: the reference's mask_edge_distance vectors
(tests/golden/edge_distance_vectors.json.gz, made by tests/golden/make_edge_distance_vectors.py), loaded once, and the direct C-ABI call."""
import base64
import ctypes as C
import functools
import gzip
import json
import os

import numpy as np

from ampis_amd import analyze, rle
from ampis_amd._lib import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_distance_vectors.json.gz")


@functools.lru_cache(maxsize=1)
def cases():
    """name -> dict(size, gt, pred (RLE dicts), gt_box, pred_box, matches [n, 2], boxes [n, 4] merged, fp / fn: per pair the reference's
    squared distances rint(v^2) as uint32; the reference's own float64 values under fp_ref / fn_ref)."""
    raw = json.load(gzip.open(GOLDEN, "rt"))
    out = {}
    for c in raw["cases"]:
        size = [int(v) for v in c["size"]]
        d = {"size": size, "matches": np.asarray(c["matches"], dtype=np.int64).reshape(-1, 2),
             "gt_box": np.asarray(c["gt_box"], dtype=np.int64).reshape(-1, 4), "pred_box": np.asarray(c["pred_box"], dtype=np.int64).reshape(-1, 4)}
        for k in ("gt", "pred"):
            d[k] = [{"size": size, "counts": base64.b64decode(s)} for s in c[k]]
        d["boxes"] = np.array([analyze.merge_boxes(d["gt_box"][g], d["pred_box"][p]) for g, p in d["matches"]], dtype=np.int64).reshape(-1, 4)
        for k in ("fp", "fn"):
            d[k + "_ref"] = [np.frombuffer(base64.b64decode(s), dtype="<f8") for s in c[k]]
            d[k] = [np.rint(v * v).astype(np.uint32) for v in d[k + "_ref"]]
            assert all(np.abs(v * v - np.rint(v * v)).max(initial=0.0) < 1e-6 for v in d[k + "_ref"])
        out[c["name"]] = d
    assert raw["max_abs_square_minus_rint"] < 1e-6 and len(out) == 18
    return out


def check_case(name, ctx=None):
    """amp_mask_edge_distance (ctx None: host path) against the fixture: list lengths and every squared distance, exactly."""
    c = cases()[name]
    fp, fn = rle.edge_distance(c["gt"], c["pred"], c["matches"], c["boxes"], ctx=ctx)
    assert len(fp) == len(fn) == len(c["matches"])
    for k, (got, want) in enumerate(zip(fp + fn, c["fp"] + c["fn"])):
        assert got.dtype == np.uint32 and len(got) == len(want), (name, k, len(got), len(want))
        assert np.array_equal(got, want), (name, k, np.flatnonzero(got != want)[:5])


def same_lists(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def call_c(ctx, gt_counts, pred_counts, pairs, boxes, h, w, fp_cap, fn_cap):
    """The raw C call on lists of uint32 run arrays -> (status, fp, fp_off, fn, fn_off); the output arrays start as 0xAB bytes (untouched())."""
    pool = lambda cs: (np.concatenate(cs).astype(np.uint32) if sum(map(len, cs)) else np.zeros(1, np.uint32),
                       np.cumsum([0] + [len(x) for x in cs[:-1]]).astype(np.uint64), np.array([len(x) for x in cs], np.int32))
    gp, go, gl = pool(gt_counts)
    pp, po, pl = pool(pred_counts)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    pg, pq = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    boxes = np.ascontiguousarray(boxes, dtype=np.int32)
    fp, fn = np.full(max(fp_cap, 1), 0xABABABAB, np.uint32), np.full(max(fn_cap, 1), 0xABABABAB, np.uint32)
    fpo, fno = np.full(len(pairs) + 1, 0xABABABABABABABAB, np.uint64), np.full(len(pairs) + 1, 0xABABABABABABABAB, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib().amp_mask_edge_distance(ctx.handle if ctx is not None else None, vp(gp), vp(go), vp(gl), len(gt_counts), vp(pp), vp(po), vp(pl),
                                      len(pred_counts), vp(pg), vp(pq), vp(boxes), len(pairs), h, w, vp(fp), fp_cap, vp(fpo), vp(fn), fn_cap, vp(fno))
    return st, fp, fpo, fn, fno


def untouched(*arrays):
    """every byte of the arrays is still call_c's fill"""
    return all((a.view(np.uint8) == 0xAB).all() for a in arrays)
