"""The case set of amp_mask_parts, shared by tests/test_mask_parts.py (host path) and tests/test_mask_parts_gpu.py (device path).  A case is
{masks: bool [N, h, w], connectivity, min_size, area_threshold (None: all holes), keep_largest}; every case is evaluated as a colour-1 call
(parts: keep_largest, min_size), a colour-0 call (holes: area_threshold) and the sequential cleaning of analyze.clean_masks.

The reference shares no code with the run-based implementation: scipy.ndimage.label only.  Parts are the labels of the mask under the full
3 x 3 structure (connectivity 2) or the cross (1); holes are the labels of the complement under the DUAL structure that touch no border of the
array; the rules are written with np.bincount on the labels; results are encoded with the host codec rle.encode."""
import functools

import numpy as np
from scipy import ndimage

from ampis_amd import rle

N_SEEDED = 200
STRUCTURE = {1: ndimage.generate_binary_structure(2, 1), 2: np.ones((3, 3), int)}
TALL = (63, 64, 65, 127, 128, 129, 130)


def _case(masks, connectivity=2, min_size=0, area_threshold=0, keep_largest=False):
    masks = np.asarray(masks)
    return {"masks": (masks if masks.ndim == 3 else masks[None]).astype(bool), "connectivity": connectivity, "min_size": min_size,
            "area_threshold": area_threshold, "keep_largest": keep_largest}


def _ring(n, t=1):
    m = np.zeros((n, n), bool)
    m[1:n - 1, 1:n - 1] = True
    m[1 + t:n - 1 - t, 1 + t:n - 1 - t] = False
    return m


def _ring_in_ring():
    """Two rings, the inner one inside the outer one's hole, a speck in the inner hole: 3 parts and 2 holes; cleaning removes the speck first
    and then judges the inner hole as a whole."""
    m = np.zeros((15, 15), bool)
    m[1:14, 1:14] = True
    m[2:13, 2:13] = False
    m[4:11, 4:11] = True
    m[5:10, 5:10] = False
    m[7, 7] = True
    return m


def _serpentine(h, w):
    m = np.zeros((h, w), bool)
    m[:, ::2] = True
    for k, c in enumerate(range(1, w, 2)):
        m[h - 1 if k % 2 == 0 else 0, c] = True
    return m


def _board(h, w):
    return np.add.outer(np.arange(h), np.arange(w)) % 2 == 0


def _hand():
    c = {}
    c["one_pixel"] = _case([[1]])
    c["one_pixel_image_empty"] = _case([[0]])
    c["empty"] = _case(np.zeros((9, 11)))
    c["full"] = _case(np.ones((9, 11)), 2, 5, None)
    c["full_64x3"] = _case(np.ones((64, 3)), 1, 0, None)              # one COCO run across the column ends
    c["ring"] = _case(_ring(7), 2, 0, None)
    c["ring_keep_hole"] = _case(_ring(7), 2, 0, 9)                    # the hole has 9 pixels: < is strict, it stays
    c["ring_fill_hole"] = _case(_ring(7), 2, 0, 10)
    c["ring_min_size_equal"] = _case(_ring(7), 2, 16, 0)              # the ring has 16 pixels: it stays
    c["ring_min_size_above"] = _case(_ring(7), 2, 17, 0)              # ... and goes
    c["ring_in_ring"] = _case(_ring_in_ring(), 2, 0, 0)
    c["ring_in_ring_clean"] = _case(_ring_in_ring(), 2, 2, None)      # solid afterwards
    c["ring_in_ring_keep_largest"] = _case(_ring_in_ring(), 1, 0, None, True)
    c["ring_in_ring_small_holes"] = _case(_ring_in_ring(), 2, 2, 25)  # the inner hole has 24 + 1 pixels once the speck is gone: strict <
    cc = np.zeros((7, 6)); cc[1:6, 0:4] = 1; cc[2:5, 0:3] = 0         # a C closed only by the image border: no hole
    c["c_closed_by_border"] = _case(cc, 2, 0, None)
    c["c_closed_by_border_4"] = _case(cc, 1, 0, None)
    corner = np.zeros((5, 5)); corner[0, 1] = corner[1, 0] = corner[1, 2] = corner[2, 1] = 1; corner[0, 0] = 0
    corner2 = np.zeros((6, 6)); corner2[1:5, 1:5] = 1; corner2[2, 2] = 0; corner2[1, 1] = 0          # hole (2, 2) meets the outside zero (1, 1) by a corner only
    c["hole_corner_8"] = _case(corner2, 2, 0, None)                   # a hole under 4-connected zeros
    c["hole_corner_4"] = _case(corner2, 1, 0, None)                   # the outside under 8-connected zeros
    c["diamond_at_corner_8"] = _case(corner, 2, 0, None)
    c["diamond_at_corner_4"] = _case(corner, 1, 0, None)
    c["board_2x2_8"], c["board_2x2_4"] = _case(_board(2, 2), 2, 0, None), _case(_board(2, 2), 1, 0, None)
    c["board_8x8_8"], c["board_8x8_4"] = _case(_board(8, 8), 2, 0, None), _case(_board(8, 8), 1, 0, None)
    c["board_8x8_4_min2"] = _case(_board(8, 8), 1, 2, 2)
    tie = np.zeros((6, 9)); tie[3:5, 5:7] = 1; tie[1:3, 1:3] = 1; tie[0, 8] = 1
    c["two_equal_parts"] = _case(tie, 2, 0, 0, True)                  # the one whose first pixel comes first in column-major order stays
    tie2 = np.zeros((6, 9)); tie2[4, 1:5] = 1; tie2[0:4, 3] = 0; tie2[0:4, 6] = 1      # first pixel (4, 1) = position 10 against (0, 6) = 36
    c["two_equal_parts_row_first"] = _case(tie2, 1, 0, 0, True)
    c["serpentine_65x33"] = _case(_serpentine(65, 33), 1, 0, None)    # one long chain of unions
    c["serpentine_65x33_complement"] = _case(~_serpentine(65, 33), 1, 3, None)
    c["serpentine_65x33_complement_8"] = _case(~_serpentine(65, 33), 2, 0, 70, True)
    c["board_130x40_8"] = _case(_board(130, 40), 2, 0, None)          # 2600 pieces of ones: across the tile and workgroup sizes and the 64-row words
    c["board_130x40_4"] = _case(_board(130, 40), 1, 2, 2)
    c["board_130x40_4_keep"] = _case(_board(130, 40), 1, 0, None, True)
    allb = np.zeros((9, 12)); allb[0, :] = allb[8, :] = 1; allb[:, 0] = allb[:, 11] = 1; allb[4, 4:7] = 1
    c["touches_all_borders"] = _case(allb, 2, 0, None)
    c["touches_all_borders_4_min"] = _case(allb, 1, 4, 80)
    gap = np.zeros((8, 9)); gap[1:7, 1:3] = 1; gap[1:7, 6:8] = 1      # two bars with whole empty columns between them
    c["empty_columns_between"] = _case(gap, 2, 0, None, True)
    mix = np.zeros((12, 15, 15), bool)
    mix[0] = _ring_in_ring(); mix[1, 7, 7] = True; mix[3] = True; mix[4, :7, :7] = _ring(7); mix[5] = _board(15, 15); mix[6] = ~_board(15, 15)
    mix[7, 2:9, 3:10] = _ring(7, 2); mix[7, 12, 12] = True; mix[8] = _serpentine(15, 15); mix[9] = ~_serpentine(15, 15)
    mix[10, 0, :] = mix[10, 14, :] = True; mix[10, :, 0] = mix[10, :, 14] = True; mix[11, 3:6, 3:6] = True; mix[11, 9:12, 9:12] = True
    c["twelve_masks"] = _case(mix, 2, 0, None)
    c["twelve_masks_4"] = _case(mix, 1, 2, 10, True)
    c["twelve_masks_thresholds"] = _case(mix, 2, 9, 26)
    # one mask of alternating rows, 257 x 1100, closed by its first and last column so that the rows of zeros are 128 holes, the upper 100 of
    # them cut in two by a bar: as holes 2 + 57 + 1097 x 257 + 1 = 281 989 items in 1102 workgroups -- the scan of the workgroup sums runs
    # over more than the 1024 entries one round takes and no multiple of it --, as parts 141 545 items in 553; 257 rows: the last 64-row
    # word of a column holds one row.  The threshold fills the holes of 499 pixels and leaves those of 598 and 1098
    rows = np.zeros((257, 1100), bool)
    rows[::2, :] = True
    rows[:, 0] = rows[:, 1099] = True
    rows[:200, 500] = True
    c["two_round_scan"] = _case(rows, 1, 0, 550)
    return c


HAND_CASES = _hand()
HAND = sorted(HAND_CASES)


@functools.lru_cache(maxsize=None)
def _seeded(i):
    rng = np.random.default_rng(41000 + i)
    h = int(rng.integers(1, 41)) if rng.random() < 0.7 else int(rng.choice(TALL))
    w, n = int(rng.integers(1, 41)), int(rng.integers(1, 13))
    if i % 2 == 0:
        masks = rng.random((n, h, w)) < float(rng.choice([0.3, 0.5, 0.7]))
    else:                                        # dilated sparse points: blobs that hold real holes
        pts = rng.random((n, h, w)) < 0.08
        masks = np.stack([ndimage.binary_dilation(p, structure=STRUCTURE[2], iterations=int(rng.integers(1, 3))) for p in pts])
        masks &= rng.random((n, h, w)) < 0.93
    thr = lambda: None if rng.random() < 0.2 else int(rng.choice([0, 1, 2, 3, 5, 9, 30]))
    min_size = thr()
    return _case(masks, int(rng.integers(1, 3)), 0 if min_size is None else min_size, thr(), bool(rng.random() < 0.4))


def get(name):
    return _seeded(int(name[5:])) if name.startswith("seed_") else HAND_CASES[name]


def names():
    return HAND + [f"seed_{i}" for i in range(N_SEEDED)]


def rles(name):
    return [rle.encode(np.asfortranarray(m)) for m in get(name)["masks"]]


def components(m, colour, connectivity):
    """(labels, areas [K], first column-major position [K]) of the components of one dense mask by definition; labels 1 .. K, 0 elsewhere"""
    if colour == 1:
        lab, n = ndimage.label(m, structure=STRUCTURE[connectivity])
    else:
        lab, n = ndimage.label(~m, structure=STRUCTURE[3 - connectivity])
        outside = np.unique(np.concatenate([lab[0, :], lab[-1, :], lab[:, 0], lab[:, -1]]))
        keep = np.setdiff1d(np.arange(1, n + 1), outside)
        remap = np.zeros(n + 1, np.int64)
        remap[keep] = np.arange(1, len(keep) + 1)
        lab, n = remap[lab], len(keep)
    flat = lab.T.ravel()                                             # column-major: position col * h + row
    areas = np.bincount(flat, minlength=n + 1)[1:]
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return lab, areas, first[1:]


def ref_call(m, colour, connectivity, threshold, keep_largest):
    """([components, their pixels, largest, pixels flipped], the dense result) of one mask by definition"""
    lab, areas, first = components(m, colour, connectivity)
    flip = np.zeros(len(areas), bool)
    if colour == 1 and keep_largest and len(areas):
        best = min(range(len(areas)), key=lambda k: (-int(areas[k]), int(first[k])))
        flip[:] = True
        flip[best] = False
    flip |= np.ones(len(areas), bool) if threshold is None else areas < threshold            # strict, as in skimage
    sel = np.concatenate([[False], flip])[lab]
    stats = [len(areas), int(areas.sum()), int(areas.max()) if len(areas) else 0, int(areas[flip].sum())]
    return stats, (m & ~sel) if colour == 1 else (m | sel)


def _encode(m):
    return rle.string_to_counts(rle.encode(np.asfortranarray(m))["counts"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per colour (1, 0): (stats int64 [N, 4], list of uint32 counts) of the two single calls, and the dense sequential cleaning with its
    statistics [N, 4] = {parts removed, pixels removed, holes filled, pixels filled}; computed once a case."""
    c = get(name)
    k = c["connectivity"]
    out = {}
    for colour, thr, keep in ((1, c["min_size"], c["keep_largest"]), (0, c["area_threshold"], False)):
        res = [ref_call(m, colour, k, thr, keep) for m in c["masks"]]
        out[colour] = (np.array([r[0] for r in res], np.int64).reshape(-1, 4), [_encode(r[1]) for r in res])
    clean, cstats = [], []
    for m in c["masks"]:
        s1, m1 = ref_call(m, 1, k, c["min_size"], c["keep_largest"])
        s0, m2 = ref_call(m1, 0, k, c["area_threshold"], False)
        _, a1, _ = components(m1, 1, k)
        _, a2, _ = components(m2, 0, k)
        clean.append(m2)
        cstats.append([s1[0] - len(a1), s1[3], s0[0] - len(a2), s0[3]])
    out["clean"] = (clean, np.array(cstats, np.int64).reshape(-1, 4))
    return out


def run(name, ctx=None):
    """rle.mask_parts on the case for both colours: {colour: (stats, counts list)}"""
    c = get(name)
    r = rles(name)
    return {1: rle.mask_parts(r, 1, c["connectivity"], c["min_size"], c["keep_largest"], ctx=ctx),
            0: rle.mask_parts(r, 0, c["connectivity"], c["area_threshold"], False, ctx=ctx)}


def check_case(name, ctx=None):
    """amp_mask_parts on the case (ctx None: the host path) against the reference: the statistics and every counts array byte for byte; a
    stats-only call gives the same statistics.  Returns the result."""
    res = run(name, ctx)
    want = expected(name)
    c = get(name)
    for colour in (1, 0):
        stats, counts = res[colour]
        assert stats.dtype == np.int64 and stats.tolist() == want[colour][0].tolist(), (name, colour)
        assert len(counts) == len(want[colour][1])
        for i, (got, w) in enumerate(zip(counts, want[colour][1])):
            assert got.dtype == np.uint32 and got.tobytes() == w.astype(np.uint32).tobytes(), (name, colour, i)
        thr, keep = (c["min_size"], c["keep_largest"]) if colour else (c["area_threshold"], False)
        only, none = rle.mask_parts(rles(name), colour, c["connectivity"], thr, keep, ctx=ctx, emit=False)
        assert none is None and only.tolist() == stats.tolist(), (name, colour)
    return res


def result_bytes(res):
    return [res[c][0].tobytes() for c in (1, 0)] + [a.tobytes() for c in (1, 0) for a in res[c][1]]
