"""The case set of amp_seg_class_map, shared by tests/test_seg_class_map.py (host path), tests/test_seg_class_map_gpu.py (device path) and, as
the hand-made shapes, by the sanitizer run.  A case is {gt, pred: lists of RLE dicts, pairs: [(g, q)], size: (h, w)}; the expected run lists
and pixel counts come from tests/seg_class_ref.py (dense NumPy), computed once per process and mode.  The smallest shapes at which the paint
or the encode can go wrong: see the comment of each case."""
import functools

import numpy as np

from ampis_amd import rle

import seg_class_ref as ref

MODES = ("reduced", "all")
H, W = 20, 30


def enc(m):
    return rle.encode(np.asfortranarray(np.asarray(m).astype(np.uint8)))


def case(gt, pred, pairs, size):
    gt, pred = [np.asarray(m, bool) for m in gt], [np.asarray(m, bool) for m in pred]
    assert all(m.shape == tuple(size) for m in gt + pred)
    return {"gt": [enc(m) for m in gt], "pred": [enc(m) for m in pred], "pairs": [tuple(p) for p in pairs], "size": tuple(size)}


def cols(h, w, which, rows=None):
    m = np.zeros((h, w), bool)
    r = slice(None) if rows is None else slice(*rows)
    for c in which:
        m[r, c] = True
    return m


def rect(h, w, r0, r1, c0, c1):
    m = np.zeros((h, w), bool)
    m[r0:r1, c0:c1] = True
    return m


def disc(h, w, cy, cx, ry, rx=None):
    yy, xx = np.ogrid[:h, :w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / (rx or ry)) ** 2 <= 1.0


def column_seam(h):
    """h rows, 5 columns: set pixels in the last row of a column and the first row of the next (one run across the seam), a blob over every
    64-row word boundary there is, and a prediction that differs in exactly the seam pixels"""
    g, q = np.zeros((h, 5), bool), np.zeros((h, 5), bool)
    g[h - 1, 1] = g[0, 2] = True                                    # one run of two pixels across columns 1 | 2
    q[h - 1, 1] = True                                              # TP in the last row, FN in the first row of the next column
    q[h - 1, 2] = q[0, 3] = True                                    # FP across columns 2 | 3
    g[h - 1, 4] = q[h - 1, 4] = True                                # the image's last pixel
    for b in range(64, h, 64):                                      # rows b - 2 .. b + 1 of column 0: across the word boundary
        g[b - 2:b + 2, 0] = True
        q[b - 1:b + 3, 0] = True
    return case([g], [q], [(0, 0)], (h, 5))


@functools.lru_cache(maxsize=None)
def hand_cases():
    z = lambda: np.zeros((H, W), bool)
    c = {}
    # 8 x 8, every one of the seven non-zero codes (and code 0).  A pair gives a pixel ONE of TP / FN / FP, so code 7 needs three pairs: the
    # smallest arrangement.  Columns 0 .. 6 hold codes 1, 2, 4, 3, 5, 6, 7 in rows 1 .. 6; column 7 is TP in rows 1 .. 3 and background below
    r = (1, 7)
    c["all_codes_8x8"] = case([cols(8, 8, (0, 1, 3, 4, 5, 6), r), cols(8, 8, (3, 6), r), cols(8, 8, (7,), (1, 4))],
                              [cols(8, 8, (0, 2, 3, 4, 6), r), cols(8, 8, (4, 5), r), cols(8, 8, (6,), r) | cols(8, 8, (7,), (1, 4))],
                              [(0, 0), (1, 1), (2, 2)], (8, 8))
    # a mask that owns pixel 0: the first count of the TP class is 0; and one that owns the last pixel: no run of zeros closes the list
    c["first_pixel"] = case([rect(H, W, 0, 3, 0, 2)], [rect(H, W, 0, 2, 0, 3)], [(0, 0)], (H, W))
    c["last_pixel"] = case([rect(H, W, H - 3, H, W - 2, W)], [rect(H, W, H - 2, H, W - 3, W)], [(0, 0)], (H, W))
    # full columns: runs cross column boundaries, the tight boxes are as tall as the image
    c["full_columns"] = case([cols(H, W, (3, 4, 5))], [cols(H, W, (4, 5, 6, 7))], [(0, 0)], (H, W))
    c["full_image"] = case([np.ones((H, W), bool)], [np.ones((H, W), bool), rect(H, W, 5, 9, 5, 9)], [(0, 0), (0, 1)], (H, W))
    # one column / one row
    c["w1"] = case([rect(37, 1, 0, 20, 0, 1)], [rect(37, 1, 10, 37, 0, 1)], [(0, 0)], (37, 1))
    c["h1"] = case([rect(1, 41, 0, 1, 0, 20)], [rect(1, 41, 0, 1, 10, 41)], [(0, 0)], (1, 41))
    c["one_pixel_image"] = case([np.ones((1, 1), bool)], [np.ones((1, 1), bool)], [(0, 0)], (1, 1))
    # the last word of a column has 63, 64, 1 and 1 valid rows
    for h in (63, 64, 65, 129):
        c[f"h{h}_seam"] = column_seam(h)
    # no pair at all, with masks on both sides
    c["no_pairs"] = case([disc(H, W, 8, 8, 5)], [disc(H, W, 9, 9, 5)], [], (H, W))
    # identical masks: TP only.  Disjoint masks: FN and FP, no TP
    c["identical"] = case([disc(H, W, 9, 14, 7, 9)], [disc(H, W, 9, 14, 7, 9)], [(0, 0)], (H, W))
    c["disjoint"] = case([rect(H, W, 2, 8, 2, 9)], [rect(H, W, 10, 18, 12, 25)], [(0, 0)], (H, W))
    # two ground truths matched to one prediction: where the prediction covers one of them it is TP of one pair and FP of the other
    c["two_gt_one_pred"] = case([rect(H, W, 3, 10, 3, 12), rect(H, W, 10, 17, 8, 20)], [rect(H, W, 5, 15, 5, 18)], [(0, 0), (1, 0)], (H, W))
    # the same pair twice
    c["pair_twice"] = case([disc(H, W, 8, 10, 6)], [disc(H, W, 10, 13, 6)], [(0, 0), (0, 0)], (H, W))
    # 64 pairs that paint the same words: shifted copies of a tall blob, all inside rows 0 .. 19 of columns 5 .. 20
    g64 = [disc(H, W, 10, 8 + i % 8, 8, 3) for i in range(8)]
    q64 = [disc(H, W, 9 + i % 3, 9 + i % 8, 8, 3) for i in range(8)]
    c["pairs_64_same_words"] = case(g64, q64, [(i % 8, i // 8) for i in range(64)], (H, W))
    # an empty mask (the single run h * w) inside a pair, on either side and on both
    c["empty_in_pair"] = case([z(), disc(H, W, 8, 8, 5), z()], [disc(H, W, 12, 20, 5), z(), z()], [(0, 0), (1, 1), (2, 2)], (H, W))
    # 257 x 13500: 67 500 plane words in 264 workgroups, so the scan of the classes x workgroups sums runs over 1056 entries (reduced) and
    # 1848 (all) -- past the 1024 entries that one round of the one-workgroup scan takes, neither a multiple of it.  Bands of rows against the
    # same bands one row lower (TP, FN and FP in every column, one band across the word edge 63 | 64, one in the single row of the ragged
    # fifth word), and a second pair whose boxes overlap the bands (the mixed codes)
    h2, w2 = 257, 13500
    g2, q2 = np.zeros((h2, w2), bool), np.zeros((h2, w2), bool)
    for a, b in ((0, 2), (62, 66), (100, 128), (200, 202), (255, 257)):
        g2[a:b, :] = True
        q2[a + 1:b + 1, :] = True
    c["two_round_scan"] = case([g2, rect(h2, w2, 90, 140, 3000, 9000)], [q2, rect(h2, w2, 110, 210, 5000, 12000)], [(0, 0), (1, 1)], (h2, w2))
    return c


HAND = ("all_codes_8x8", "first_pixel", "last_pixel", "full_columns", "full_image", "w1", "h1", "one_pixel_image", "h63_seam", "h64_seam",
        "h65_seam", "h129_seam", "no_pairs", "identical", "disjoint", "two_gt_one_pred", "pair_twice", "pairs_64_same_words", "empty_in_pair",
        "two_round_scan")
N_SEEDED = 200


@functools.lru_cache(maxsize=None)
def seeded_case(i):
    """images of at most 96 x 96, up to 12 blobs a side (discs, boxes, now and then an empty or a full mask), a random pair list with repeats"""
    r = np.random.default_rng(20261018 + i)
    h, w = (int(v) for v in r.integers(1, 97, size=2))
    if i % 10 == 0:
        h = int(r.choice([63, 64, 65, 96]))

    def blob():
        kind = int(r.integers(0, 10))
        if kind == 0:
            return np.zeros((h, w), bool)
        if kind == 1:
            return np.ones((h, w), bool)
        if kind < 5:
            r0, c0 = int(r.integers(0, h)), int(r.integers(0, w))
            return rect(h, w, r0, r0 + 1 + int(r.integers(0, h)), c0, c0 + 1 + int(r.integers(0, w)))
        return disc(h, w, r.integers(0, h), r.integers(0, w), r.integers(1, 40), r.integers(1, 40))

    gt, pred = [blob() for _ in range(int(r.integers(1, 13)))], [blob() for _ in range(int(r.integers(1, 13)))]
    n = int(r.integers(0, 21))
    pairs = [(int(r.integers(0, len(gt))), int(r.integers(0, len(pred)))) for _ in range(n)]
    if n > 2:
        pairs[-1] = pairs[0]                                        # a repeat for sure
    return case(gt, pred, pairs, (h, w))


def get(name):
    return seeded_case(int(name[5:])) if name.startswith("seed_") else hand_cases()[name]


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    c = get(name)
    return ref.dense(c["gt"], c["pred"], c["pairs"], mode, c["size"])


def check_case(name, mode, ctx=None):
    """amp_seg_class_map on the case (ctx None: the host path) against the dense reference: every count and every pixel count exactly.
    Returns the result."""
    c = get(name)
    counts, pixels = rle.seg_class_map(c["gt"], c["pred"], c["pairs"], mode, ctx=ctx, size=c["size"])
    want, want_px, _ = expected(name, mode)
    assert len(counts) == len(want) == (7 if mode == "all" else 4)
    for k, (a, b) in enumerate(zip(counts, want)):
        assert a.dtype == np.uint32 and a.tobytes() == b.astype(np.uint32).tobytes(), (name, mode, k, a[:12], b[:12])
    assert pixels.dtype == np.int64 and pixels.tolist() == want_px.tolist(), (name, mode, pixels, want_px)
    assert int(pixels.sum()) == c["size"][0] * c["size"][1]
    return counts, pixels
