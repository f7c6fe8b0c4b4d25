"""The case set of amp_mask_distance, shared by tests/test_mask_distance.py (host path) and tests/test_mask_distance_gpu.py (device path).  A case
is a pool {masks: bool [N, h, w], rles: the run lists handed to the call (the encoded masks unless the case brings looser ones)}; every case
is run at both border values and at ncurve 0, 1, 9 and 1025, with the map.  The reference is tests/mask_distance_ref.py, scipy on one decoded
mask; the seeded pools are those of tests/morphology_cases.py; the largest images are shapes whose distances are written down in closed form,
because nothing dense of 2^30 pixels is made."""
import functools

import numpy as np

from ampis_amd import rle

import mask_distance_ref as ref
import morphology_cases as mc

NONE = ref.NONE
BORDERS = (0, 1)
NCURVES = (0, 1, 9, 1025)
N_SEEDED = mc.N_SEEDED


def _case(masks, rles=None):
    masks = np.asarray(masks).astype(bool)
    assert masks.ndim == 3
    return {"masks": masks, "rles": rles}


def _disk(h, w, cy, cx, r2):
    yy, xx = np.indices((h, w))
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r2


def _hand():
    c = {}
    c["image_1x1"] = _case([[[False]], [[True]]])
    corners = np.zeros((4, 6, 7), bool)
    for i, (r, q) in enumerate(((0, 0), (0, 6), (5, 0), (5, 6))):
        corners[i, r, q] = True
    c["one_pixel_in_each_corner"] = _case(corners)
    c["full_image"] = _case(np.ones((1, 5, 6), bool))                # the sentinel with border_value 1
    c["single_row_image"] = _case(np.stack([np.ones(11, bool), np.arange(11) % 4 != 1, np.arange(11) > 3, np.arange(11) == 10])[:, None, :])
    c["single_column_image"] = _case(np.stack([np.ones(11, bool), np.arange(11) % 4 != 1, np.arange(11) > 3, np.arange(11) == 10])[:, :, None])
    sq = np.zeros((1, 5, 6), bool); sq[0, 2:4, 3:5] = True
    c["square_2x2"] = _case(sq)                                      # all d2 equal: the tie rule decides
    rect = np.zeros((2, 9, 9), bool); rect[0, 2:5, 2:7] = True; rect[1, 2:7, 3:6] = True
    c["rectangles_3x5_and_5x3"] = _case(rect)
    c["disk"] = _case(_disk(15, 17, 7, 8, 36)[None])
    c["ring"] = _case((_disk(17, 17, 8, 8, 60) & ~_disk(17, 17, 8, 8, 6))[None])          # the hole is the nearest background
    neck = np.zeros((1, 11, 19), bool); neck[0] = _disk(11, 19, 5, 4, 16) | _disk(11, 19, 5, 14, 16); neck[0, 5, 4:15] = True
    c["two_parts_with_a_neck"] = _case(neck)
    ell = np.zeros((1, 10, 9), bool); ell[0, 1:9, 1:4] = True; ell[0, 6:9, 1:8] = True
    c["L"] = _case(ell)
    board = np.add.outer(np.arange(7), np.arange(8)) % 2 == 0
    c["checkerboard"] = _case(np.stack([board, ~board]))
    cross = np.zeros((1, 9, 11), bool); cross[0, 3:6, :] = True; cross[0, :, 4:7] = True
    frame = np.ones((1, 9, 11), bool); frame[0, 2:7, 2:9] = False
    c["touching_all_four_sides"] = _case(np.concatenate([cross, frame]))
    tall = np.zeros((2, 134, 7), bool); tall[0, 2:132, 1:6] = True; tall[0, 64, 3] = False; tall[1, 2:132, 1:6] = True; tall[1, 127, 3] = False
    c["piece_130_rows_tall"] = _case(tall)                           # crosses the 64-row tiles of its pieces at rows 65 / 66 and 129 / 130
    slot = np.ones((2, 5, 40), bool); slot[0, 2, 35] = False; slot[1, 0, 38] = False
    c["background_in_a_far_column_only"] = _case(slot)               # border_value 1: every near column is full and has no column distance
    blob = np.zeros((3, 9, 8), bool); blob[0, 1:8, 1:7] = True; blob[1, :, 2:5] = True; blob[2, 4, :] = True; blob[2, 0:6, 3] = True
    c["zero_length_runs"] = _case(blob, rles=[mc.loosen(rle.encode(np.asfortranarray(m))) for m in blob])
    three = np.zeros((3, 8, 9), bool); three[0, 1:6, 1:6] = True; three[2, 3:8, 3:9] = True
    c["an_empty_mask_between_two_others"] = _case(three)
    over = np.zeros((3, 9, 10), bool); over[0, 1:7, 1:7] = True; over[1, 3:9, 4:10] = True; over[2, 1:7, 1:7] = True
    c["overlapping_masks"] = _case(over)
    return c


_HAND = _hand()
HAND = tuple(_HAND)
SEEDED = mc.SEEDED


@functools.lru_cache(maxsize=None)
def get(name):
    return _HAND[name] if name in _HAND else _case(mc.get(name)["masks"])


def size(name):
    return tuple(int(v) for v in get(name)["masks"].shape[1:])


@functools.lru_cache(maxsize=None)
def rles(name):
    c = get(name)
    return tuple(c["rles"]) if c["rles"] is not None else tuple(rle.encode(np.asfortranarray(m)) for m in c["masks"])


@functools.lru_cache(maxsize=None)
def expected(name, b):
    """per mask ref.outputs from scipy on the decoded mask; computed once and shared"""
    return tuple(ref.outputs(m, ref.scipy_d2(m, b), NCURVES) for m in get(name)["masks"])


def run(name, b, ncurve=0, want_map=True, ctx=None):
    return rle.mask_distance(list(rles(name)), b, ncurve, want_map, ctx=ctx, size=size(name))


def result_bytes(res):
    stats, boxes, curve, maps = res
    return (stats.tobytes(), boxes.tobytes(), curve.tobytes(), None if maps is None else tuple((m.shape, m.tobytes()) for m in maps))


def equal_to(res, want, ncurve, where):
    """a result of rle.mask_distance against the per-mask expectations, every word"""
    stats, boxes, curve, maps = res
    n = len(want)
    assert stats.dtype == np.int64 and boxes.dtype == np.int64 and curve.dtype == np.int64, where
    assert stats.shape == (n, 4) and boxes.shape == (n, 4) and curve.shape == (n, ncurve), where
    assert stats.tolist() == [x["stats"] for x in want], where
    assert boxes.tolist() == [x["box"] for x in want], where
    assert curve.tolist() == [x["curve"][ncurve] for x in want], where
    if maps is not None:
        assert len(maps) == n, where
        for got, x in zip(maps, want):
            assert got.dtype == np.uint32 and got.shape == x["map"].shape and got.tobytes() == x["map"].tobytes(), where


def check_case(name, b, ctx=None):
    """one case at one border value and every ncurve, with the map, against the reference; the statistics-only call as well; [result bytes]"""
    want, out = expected(name, b), []
    for ncurve in NCURVES:
        res = run(name, b, ncurve, True, ctx=ctx)
        equal_to(res, want, ncurve, (name, b, ncurve))
        out.append(result_bytes(res))
    res = run(name, b, 9, False, ctx=ctx)
    assert res[3] is None
    equal_to(res, want, 9, (name, b, "no map"))
    out.append(result_bytes(res))
    return out


# ---- the largest sides: distances in closed form --------------------------------------------------------------------------------------------------

def _strip_d2(n, pieces, border, along_rows):
    """a 1-pixel-wide image n long with the mask's pieces [a, e) along it.  Across the strip both neighbours lie outside the image: d2 = 1 with
    border_value 0, nothing with 1.  Along it the distance to the piece's ends, an end at the image's edge not counting with border_value 1."""
    d2 = np.zeros(n, np.int64)
    for a, e in pieces:
        y = np.arange(a, e, dtype=np.int64)
        if border == 0:
            d2[a:e] = 1
            continue
        g = np.full(e - a, NONE, np.int64)
        if a > 0:
            g = np.minimum(g, y - a + 1)
        if e < n:
            g = np.minimum(g, e - y)
        d2[a:e] = np.where(g == NONE, NONE, g * g)
    return d2[:, None] if along_rows else d2[None, :]


def _bar_d2(n, border, vertical):
    """a bar 3 pixels wide and n long in a 5 x n (or n x 5) image, one free line on either side: the side lines are at distance 1, the middle
    line at 2 -- except, with border_value 0, at its two ends, which are 1 from the outside of the image"""
    d2 = np.zeros((5, n), np.int64)
    d2[1] = d2[3] = 1
    d2[2] = 4
    if border == 0:
        d2[2, 0] = d2[2, n - 1] = 1
    return d2.T.copy() if vertical else d2


STRIPS = {
    "strip_32768x1": (True, [[(10, 60), (300, 301), (32760, 32768)], [(0, 40), (32700, 32768)], [(0, 32768)], []]),
    "strip_1x32768": (False, [[(10, 60), (300, 301), (32760, 32768)], [(0, 40), (32700, 32768)], []]),
}
LARGEST = ("strip_32768x1", "strip_1x32768", "bar_32768x5", "bar_5x32768")
LARGEST_NCURVES = (0, 9)


@functools.lru_cache(maxsize=None)
def largest(name, b):
    """(size, rles, per mask ref.outputs) of a case with one long side, from dense arrays of at most 5 x 32768"""
    if name in STRIPS:
        rows, masks = STRIPS[name]
        dense = [_strip_d2(32768, p, b, rows) for p in masks]
    else:
        dense = [_bar_d2(32768, b, name == "bar_32768x5")]
    ms = [d > 0 for d in dense]
    return ms[0].shape, [rle.encode(np.asfortranarray(m)) for m in ms], [ref.outputs(m, d, LARGEST_NCURVES) for m, d in zip(ms, dense)]


FRAME_K = 7                                                          # the side of the squares in the corners of the 2^30 image
FAR_RECTS = [(100, 200, 103, 205), (32765, 32763, 32768, 32768), (20000, 32767, 20004, 32768)]      # 3 x 5 inside, 3 x 5 in the last corner, 4 x 1 on the last column


def frame_inputs():
    """the 32768 x 32768 image: mask 0 is the one-pixel frame round it with a FRAME_K x FRAME_K square in every corner, mask 1 is empty, mask 2 a
    3 x 5 rectangle far from everything"""
    n, k = 32768, FRAME_K
    rects = [(0, 0, n, 1), (0, n - 1, n, n), (0, 1, 1, n - 1), (n - 1, 1, n, n - 1),
             (1, 1, k, k), (n - k, 1, n - 1, k), (1, n - k, k, n - 1), (n - k, n - k, n - 1, n - 1)]
    return [mc.rects_rle(n, n, rects), mc.rects_rle(n, n, []), mc.rects_rle(n, n, [FAR_RECTS[0]])]


def _rect_d2(hh, ww):
    """a rectangle with background all round it: the distance to the nearest side"""
    r, c = np.indices((hh, ww))
    return (np.minimum(np.minimum(r + 1, hh - r), np.minimum(c + 1, ww - c)) ** 2).astype(np.int64)


def frame_expected(b, ncurve):
    """(stats, boxes, curve) of frame_inputs().  A frame pixel outside the squares has a background pixel beside it: d2 = 1.  Pixel (r, c) of the
    square in the first corner is (r + 1, c + 1) from the outside of the image (border_value 0 only) and sees the background inside the image
    at (k, max(c, 1)) and at (max(r, 1), k); the other corners are its mirror images."""
    n, k = 32768, FRAME_K
    r, c = np.indices((k, k))
    d2 = np.minimum((k - r) ** 2 + (c == 0), (k - c) ** 2 + (r == 0)).astype(np.int64)
    if b == 0:
        d2 = np.minimum(d2, np.minimum(r + 1, c + 1) ** 2)
    vals = np.concatenate([np.tile(d2.reshape(-1), 4), np.ones(4 * n - 4 - 4 * (2 * k - 1), np.int64)])
    top = int(d2.max())
    rr, cc = np.nonzero(d2 == top)
    pos = int((cc * n + rr).min())                                   # the square of the first corner comes first in column-major order
    small = _rect_d2(3, 5)
    stats = [[top, pos, int(vals.sum()), len(vals)], [0, 0, 0, 0], [4, 201 * n + 101, int(small.sum()), 15]]
    boxes = [[0, 0, n, n], [0, 0, 0, 0], [100, 200, 103, 205]]
    curve = [[int((v > q * q).sum()) for q in range(ncurve)] for v in (vals, np.zeros(0, np.int64), small.reshape(-1))]
    return stats, boxes, curve


def far_inputs():
    return [mc.rects_rle(32768, 32768, [q]) for q in FAR_RECTS]


def far_expected(b):
    """per mask ref.outputs-like dicts of far_inputs(): small rectangles whose positions need 30 bits; with border_value 1 a side on the image's
    edge does not count"""
    n, out = 32768, []
    for r0, c0, r1, c1 in FAR_RECTS:
        r, c = np.indices((r1 - r0, c1 - c0))
        sides = [r + 1 if (b == 0 or r0 > 0) else None, r1 - r0 - r if (b == 0 or r1 < n) else None,
                 c + 1 if (b == 0 or c0 > 0) else None, c1 - c0 - c if (b == 0 or c1 < n) else None]
        d2 = (np.minimum.reduce([s for s in sides if s is not None]) ** 2).astype(np.int64)
        top = int(d2.max())
        rr, cc = np.nonzero(d2 == top)
        k = int(np.argmin((cc + c0) * n + rr + r0))
        out.append({"stats": [top, int(cc[k] + c0) * n + int(rr[k] + r0), int(d2.sum()), int(d2.size)], "box": [r0, c0, r1, c1],
                    "map": d2.astype(np.uint32), "curve": {9: [int((d2 > q * q).sum()) for q in range(9)]}})
    return out
