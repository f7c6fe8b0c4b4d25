"""Golden vectors of `ampis.analyze.mask_edge_distance` (ampis/analyze.py:416-499) made BY THE REFERENCE ITSELF, run in the build container (where
/root/reference exists) in the manner of make_reference_vectors.py: the reference is imported UNMODIFIED on the façade and called with
device='cpu'.  Inputs (counts strings, per-mask index boxes, matches) and the reference's float64 outputs (base64, little-endian) go to
tests/golden/edge_distance_vectors.json.gz; tests/test_edge_distance.py and tests/test_edge_distance_gpu.py hold the product to them.

The reference's values are torch.sqrt of exact integers and not always the correctly rounded root, so the contract is the integer:
every value v satisfies |v^2 - rint(v^2)| < 1e-6 (asserted here, the maximum is recorded), and rint(v^2) is the reference's squared distance.

    python tests/golden/make_edge_distance_vectors.py        # needs /root/reference and the built library

Groups, the smallest cases at which the native code can go wrong: A hand-built shapes on 40 x 70; B crop heights / widths around the 32 / 64 / 128
bit word borders; C searches that run the whole length of the crop; D 320 pairs in one call; E run positions beyond 2^20 on 1024 x 1536.
"""
import base64
import gzip
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = "/root/reference"
sys.path.insert(0, ROOT)
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402

import ampis_amd  # noqa: E402

ampis_amd.install_as_detectron2()
for name, attrs in (("skimage", {}), ("skimage.io", {}), ("skimage.measure", {}), ("skimage.draw", {"polygon2mask": lambda shape, poly: None}), ("cv2", {})):
    if name not in sys.modules:
        m = types.ModuleType(name); m.__dict__.update(attrs); m.__path__ = []
        sys.modules[name] = m
for alias, t in (("int", int), ("float", float), ("bool", bool)):
    if not hasattr(np, alias):
        setattr(np, alias, t)
sys.path.insert(0, REFERENCE)
from ampis import analyze  # noqa: E402
from ampis_amd import rle  # noqa: E402

LIMIT = 523152          # the largest fixture so far (rle_pickles.json.gz)


def b64(b):
    return base64.b64encode(b).decode("ascii")


def tight(m):
    """index box [r1, r2, c1, c2] of the set pixels; [0, 0, 0, 0] for an empty mask"""
    rows, cols = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
    return [0, 0, 0, 0] if len(rows) == 0 else [int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1]


def disc(h, w, cy, cx, ry, rx=None):
    yy, xx = np.ogrid[:h, :w]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / (rx or ry)) ** 2 <= 1.0)


def blobs(r, h, w, k, lo, hi):
    m = np.zeros((h, w), bool)
    for _ in range(k):
        m |= disc(h, w, r.integers(0, h), r.integers(0, w), r.integers(lo, hi), r.integers(lo, hi))
    return m


def group_a():
    h, w = 40, 70
    z = lambda: np.zeros((h, w), bool)
    full = [0, h, 0, w]
    out = []

    def case(name, gt, pred, matches, gt_box=None, pred_box=None):
        out.append((f"A/{name}", (h, w), gt, pred, gt_box or [tight(m) for m in gt], pred_box or [tight(m) for m in pred], matches))

    d = disc(h, w, 20, 30, 11)
    case("identical", [d], [d], [(0, 0)])
    case("pred_inside_gt", [d], [disc(h, w, 20, 31, 6)], [(0, 0)])
    a, b = z(), z()
    a[0, 0] = True; b[h - 1, w - 1] = True
    case("corner_pixels", [a], [b], [(0, 0)], [full], [full])
    case("annulus_vs_disc", [disc(h, w, 19, 35, 17) & ~disc(h, w, 19, 35, 9)], [disc(h, w, 19, 35, 13)], [(0, 0)])
    a, b = z(), z()
    a[5:15, 5:15] = True; a[5:15, 40:50] = True          # two components of the ground truth ...
    b[5:15, 8:38] = True; b[20:30, 40:50] = True         # ... the prediction's spill from the first ends next to the second
    case("two_components", [a], [b], [(0, 0)])
    a, b = z(), z()
    for i in range(12):
        a[3 * i: 3 * i + 3, 5 * i: 5 * i + 5] = True
        b[3 * i + 2: 3 * i + 5, 5 * i + 1: 5 * i + 7] = True
    case("staircase", [a], [b], [(0, 0)])
    a, b = ~z(), ~z()
    a[10:20, 10:30] = False; b[15:33, 25:60] = False
    case("all_borders_full_box", [a], [b], [(0, 0)], [full], [full])
    g, p = disc(h, w, 20, 30, 14), disc(h, w, 23, 36, 14)
    case("boxes_cut_masks", [g], [p], [(0, 0)], [[12, 25, 22, 40]], [[15, 29, 25, 44]])
    case("box_beyond_image", [g], [p], [(0, 0)], [[5, 100, 10, 200]], [[8, 41, 12, 70]])
    case("empty_crop", [g], [p], [(0, 0)], [[7, 7, 3, 3]], [[7, 7, 3, 3]])
    g2, p2 = disc(h, w, 18, 40, 12, 20), disc(h, w, 22, 26, 13, 18)
    case("indices_reused", [g, g2], [p, p2], [(0, 0), (0, 1), (1, 0), (1, 1)])
    case("no_matches", [g], [p], [])
    return out


def group_b():
    h = w = 140
    dims = (1, 31, 32, 33, 63, 64, 65, 127, 129)
    r = np.random.default_rng(4242)
    gt, pred, gb, pb = [], [], [], []
    for hh in dims:
        for ww in dims:
            g = blobs(r, h, w, 4, 6, 40)
            p = np.roll(g, (int(r.integers(-3, 4)), int(r.integers(-3, 4))), (0, 1)) ^ blobs(r, h, w, 2, 3, 12)
            g[3, 5] = p[3, 5] = True                     # the crop's origin belongs to both: no crop without a target
            gt.append(g); pred.append(p)
            gb.append([3, 3 + hh, 5, 5 + ww]); pb.append([3, 3 + hh, 5, 5 + ww])
    return [("B/word_borders", (h, w), gt, pred, gb, pb, [(i, i) for i in range(len(gt))])]


def group_c():
    out = []
    for name, (h, w) in (("tall", (300, 3)), ("wide", (3, 300))):
        a, b = np.zeros((h, w), bool), np.zeros((h, w), bool)
        if h > w:
            a[0, :] = True; b[h - 1, :] = True
        else:
            a[:, 0] = True; b[:, w - 1] = True
        out.append((f"C/{name}", (h, w), [a], [b], [[0, h, 0, w]], [[0, h, 0, w]], [(0, 0)]))
    n = 200
    a, b = np.zeros((n, n), bool), np.ones((n, n), bool)
    a[0, 0] = True
    out.append(("C/pixel_vs_square", (n, n), [a], [b], [tight(a)], [tight(b)], [(0, 0)]))
    return out


def group_d(pairs=320):
    h, w = 48, 64
    r = np.random.default_rng(777)
    gt, pred = [], []
    for _ in range(pairs):
        g = blobs(r, h, w, 2, 3, 14)
        p = np.roll(g, (int(r.integers(-2, 3)), int(r.integers(-2, 3))), (0, 1)) | blobs(r, h, w, 1, 2, 6)
        if r.random() < 0.5:
            p &= ~blobs(r, h, w, 1, 2, 6)
        if not (g & p).any():
            p |= g
        gt.append(g); pred.append(p)
    return [("D/many_pairs", (h, w), gt, pred, [tight(m) for m in gt], [tight(m) for m in pred], [(i, i) for i in range(pairs)])]


def group_e():
    h, w = 1024, 1536
    g, p = disc(h, w, 955, 1465, 60, 62), disc(h, w, 962, 1472, 58, 61)
    return [("E/large_offsets", (h, w), [g], [p], [tight(g)], [tight(p)], [(0, 0)])]


def main():
    import torch
    cases, worst = [], 0.0
    for name, (h, w), gt, pred, gb, pb, matches in group_a() + group_b() + group_c() + group_d() + group_e():
        gr = [rle.encode(np.asfortranarray(m.astype(np.uint8))) for m in gt]
        pr = [rle.encode(np.asfortranarray(m.astype(np.uint8))) for m in pred]
        mt = np.asarray(matches, dtype=int).reshape(-1, 2)
        fp, fn = analyze.mask_edge_distance(gr, pr, np.asarray(gb), np.asarray(pb), mt, device="cpu")
        assert len(fp) == len(fn) == len(mt)
        for t in fp + fn:
            assert t.dtype == torch.float64
            v = t.numpy()
            if len(v):
                err = float(np.abs(v * v - np.rint(v * v)).max())
                assert err < 1e-6, (name, err)
                worst = max(worst, err)
        cases.append({"name": name, "size": [h, w], "gt": [b64(x["counts"]) for x in gr], "pred": [b64(x["counts"]) for x in pr],
                      "gt_box": gb, "pred_box": pb, "matches": mt.tolist(),
                      "fp": [b64(t.numpy().astype("<f8").tobytes()) for t in fp], "fn": [b64(t.numpy().astype("<f8").tobytes()) for t in fn]})
        print(name, len(mt), "pairs,", sum(len(t) for t in fp), "fp,", sum(len(t) for t in fn), "fn")
    out = {"made_by": "tests/golden/make_edge_distance_vectors.py: ampis.analyze.mask_edge_distance of rccohn/AMPIS imported unmodified on the "
                      "ampis_amd facade, device='cpu'",
           "max_abs_square_minus_rint": worst, "cases": cases}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "edge_distance_vectors.json.gz")
    with gzip.open(dst, "wt", compresslevel=9) as f:
        json.dump(out, f)
    size = os.path.getsize(dst)
    print("wrote", dst, size, "bytes,", len(cases), "cases, max |v^2 - rint(v^2)| =", worst)
    assert size <= LIMIT, f"{size} bytes: larger than the largest fixture ({LIMIT})"


if __name__ == "__main__":
    main()
