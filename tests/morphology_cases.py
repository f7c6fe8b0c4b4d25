"""The case set of amp_mask_morphology, shared by tests/test_morphology.py (host path) and tests/test_morphology_gpu.py (device path).  A case is a
pool {masks: bool [N, h, w], rles: the run lists handed to the call (the encoded masks unless the case brings looser ones), radii: the radii it
is run at}; every case is crossed with the three shapes, its radii, both border values and all six ops.  The reference is
tests/morphology_ref.py, scipy on one decoded mask; the largest images are built from rectangles whose results are written down in closed
form -- a rectangle dilated by a square is a rectangle, eroded by a disk it is the rectangle shrunk by the radius --, because nothing dense of
2^30 pixels is made."""
import functools

import numpy as np

from ampis_amd import rle

import morphology_ref as ref

OPS, SHAPES = ref.OPS, ref.SHAPES
RADII = (0, 1, 2, 3, 7)
BORDERS = (0, 1)
N_SEEDED = 200


def _case(masks, rles=None, radii=RADII):
    masks = np.asarray(masks).astype(bool)
    assert masks.ndim == 3
    return {"masks": masks, "rles": rles, "radii": tuple(radii)}


def _one(h, w, *pixels):
    m = np.zeros((1, h, w), bool)
    for r, c in pixels:
        m[0, r, c] = True
    return m


def loosen(r):
    """the run list of an RLE dict with zero-length runs put in: a run of 3 or more becomes 2, 0, the rest"""
    out = []
    for c in rle.string_to_counts(r["counts"]).tolist():
        out += [2, 0, c - 2] if c >= 3 else [c]
    return {"size": list(r["size"]), "counts": np.asarray(out, np.uint32)}


def _hand():
    c = {}
    c["empty"] = _case(np.zeros((1, 5, 6), bool))
    c["full"] = _case(np.ones((1, 5, 6), bool))
    for h, w in ((1, 1), (1, 9), (9, 1)):
        grid = np.arange(h * w).reshape(h, w)
        c[f"image_{h}x{w}"] = _case(np.stack([np.zeros((h, w), bool), np.ones((h, w), bool), grid % 2 == 0, grid % 4 != 1, grid == h * w - 1]))
    c["corner_and_side_pixels"] = _case(np.concatenate([_one(6, 7, (0, 0)), _one(6, 7, (0, 6)), _one(6, 7, (5, 0)), _one(6, 7, (5, 6)),
                                                        _one(6, 7, (0, 3)), _one(6, 7, (5, 3)), _one(6, 7, (2, 0)), _one(6, 7, (2, 6))]))
    cross = np.zeros((1, 9, 11), bool); cross[0, 3:6, :] = True; cross[0, :, 4:7] = True
    frame = np.ones((1, 9, 11), bool); frame[0, 2:7, 2:9] = False
    c["touching_all_four_borders"] = _case(np.concatenate([cross, frame]))
    for lo, gaps in (("a", (1, 2, 3, 4, 5)), ("b", (6, 7, 14, 15, 16))):          # 2 hh and 2 hh + 1 for hh = 1, 2, 3, 7: the grown pieces just merge, just do not
        m = np.zeros((len(gaps), 40, 5), bool)
        for i, g in enumerate(gaps):
            m[i, 8:12, 2] = True; m[i, 12 + g: 15 + g, 2] = True
        c[f"two_pieces_in_a_column_{lo}"] = _case(m)
    for lo, lens in (("a", (1, 2, 3, 4, 5)), ("b", (6, 7, 14, 15, 16))):          # 2 hh rows vanish under erosion, 2 hh + 1 survive as one row
        m = np.zeros((len(lens), 24, 21), bool)
        for i, k in enumerate(lens):
            m[i, 3: 3 + k, 2:19] = True
        c[f"pieces_of_length_{lo}"] = _case(m)
    cols = np.zeros((2, 5, 4), bool); cols[0, :, 1] = True; cols[0, 3:, 0] = True; cols[0, :2, 2] = True; cols[1, :, 1:] = True
    c["runs_joined_across_column_ends"] = _case(cols)
    blob = np.zeros((3, 9, 8), bool); blob[0, 1:8, 1:7] = True; blob[1, :, 2:5] = True; blob[2, 4, :] = True; blob[2, 0:6, 3] = True
    c["zero_length_runs"] = _case(blob, rles=[loosen(rle.encode(np.asfortranarray(m))) for m in blob])
    c["radius_beyond_both_sides"] = _case(np.stack([np.add.outer(np.arange(5), np.arange(6)) % 3 == 0, np.ones((5, 6), bool), np.zeros((5, 6), bool)]),
                                          radii=(6, 8, 40))
    bridge = np.zeros((1, 9, 15), bool); bridge[0, 1:8, 1:6] = True; bridge[0, 1:8, 9:14] = True; bridge[0, 4, 6:9] = True
    c["bridge"] = _case(bridge)
    crack = np.zeros((1, 11, 15), bool); crack[0, 2:9, 2:13] = True; crack[0, 2:9, 7] = False
    c["crack"] = _case(crack)
    board = np.add.outer(np.arange(7), np.arange(7)) % 2 == 0
    c["checkerboard_7x7"] = _case(np.stack([board, ~board]))
    c["pool_of_0"] = _case(np.zeros((0, 4, 5), bool))
    return c


def _seeded(i):
    """1 - 6 masks of up to 40 pixels a side: noise of density 0.1 .. 0.95, for every second seed in blocks of up to 4 x 4 pixels so that erosions
    leave something"""
    rng = np.random.RandomState(9100 + i)
    n, h, w = int(rng.randint(1, 7)), int(rng.randint(1, 41)), int(rng.randint(1, 41))
    if i < 3:
        h, w = (40, 40, 1)[i], (40, 1, 40)[i]
    masks = np.zeros((n, h, w), bool)
    for k in range(n):
        density = rng.uniform(0.1, 0.95)
        b = int(rng.randint(2, 5)) if i % 2 else 1
        coarse = rng.random_sample(((h + b - 1) // b, (w + b - 1) // b)) < density
        masks[k] = np.kron(coarse, np.ones((b, b), bool))[:h, :w]
    return _case(masks)


# ---- the largest sides: rectangles [r0, r1) x [c0, c1), results in closed form -------------------------------------------------------------------

def rects_rle(h, w, rects):
    """the canonical RLE dict of a union of disjoint rectangles, none dense"""
    runs = sorted((c * h + r0, c * h + r1) for r0, c0, r1, c1 in rects if r0 < r1 for c in range(c0, c1))
    counts, at = [], 0
    for s, e in runs:
        if counts and s == at:
            counts[-1] += e - s                                     # joined across a column end
        else:
            counts += [s - at, e - s]
        at = e
    if at < h * w or not counts:
        counts.append(h * w - at)                               # no empty closing run: the canonical form
    return {"size": [h, w], "counts": rle.counts_to_string(np.asarray(counts, np.uint32))}


def rects_box_area(rects):
    rects = [r for r in rects if r[0] < r[2] and r[1] < r[3]]
    if not rects:
        return [0, 0, 0, 0], 0
    return ([min(r[0] for r in rects), min(r[1] for r in rects), max(r[2] for r in rects), max(r[3] for r in rects)],
            sum((r[2] - r[0]) * (r[3] - r[1]) for r in rects))


def grown(rect, r, h, w):
    return (max(rect[0] - r, 0), max(rect[1] - r, 0), min(rect[2] + r, h), min(rect[3] + r, w))


def shrunk(rect, r, b, h, w):
    r0 = rect[0] if b and rect[0] == 0 else rect[0] + r
    c0 = rect[1] if b and rect[1] == 0 else rect[1] + r
    r1 = rect[2] if b and rect[2] == h else rect[2] - r
    c1 = rect[3] if b and rect[3] == w else rect[3] - r
    return (r0, c0, r1, c1) if r0 < r1 and c0 < c1 else (0, 0, 0, 0)


# per case: the size and per mask its rectangles, far enough apart that their dilations by LARGEST_RADII stay apart
LARGEST = {
    "strip_32768x1": ((32768, 1), [[(10, 0, 60, 1), (300, 0, 301, 1)], [(0, 0, 40, 1), (32700, 0, 32768, 1)], [(0, 0, 32768, 1)], []]),
    "strip_1x32768": ((1, 32768), [[(0, 10, 1, 60), (0, 300, 1, 301)], [(0, 0, 1, 40), (0, 32700, 1, 32768)], [(0, 0, 1, 32768)], []]),
    "image_2_30": ((32768, 32768), [[(100, 200, 160, 300), (20000, 9000, 20100, 9040)], [(0, 0, 50, 70)], [(32700, 32690, 32768, 32768)],
                                    [(0, 16000, 32768, 16040)]]),
}
LARGEST_RADII = (1, 7, 20)


def largest_inputs(name):
    (h, w), masks = LARGEST[name]
    return [rects_rle(h, w, rects) for rects in masks]


def largest_expected(name, op, r, b):
    """('dilate' by the square, 'erode' by the disk) -> (counts strings, boxes, areas)"""
    (h, w), masks = LARGEST[name]
    out = [[grown(q, r, h, w) if op == "dilate" else shrunk(q, r, b, h, w) for q in rects] for rects in masks]
    stats = [rects_box_area(rects) for rects in out]
    return ([rects_rle(h, w, rects)["counts"] for rects in out], np.asarray([s[0] for s in stats], np.int64).reshape(-1, 4),
            np.asarray([s[1] for s in stats], np.int64))


# ---- access ---------------------------------------------------------------------------------------------------------------------------------------

_HAND = _hand()
HAND = tuple(_HAND)
SEEDED = tuple(f"seed_{i}" for i in range(N_SEEDED))


@functools.lru_cache(maxsize=None)
def get(name):
    return _HAND[name] if name in _HAND else _seeded(int(name.split("_")[1]))


def size(name):
    return tuple(int(v) for v in get(name)["masks"].shape[1:])


@functools.lru_cache(maxsize=None)
def rles(name):
    c = get(name)
    return tuple(c["rles"]) if c["rles"] is not None else tuple(rle.encode(np.asfortranarray(m)) for m in c["masks"])


def combos(name):
    """every (shape, radius, border_value) the case is run at"""
    return [(s, r, b) for s in SHAPES for r in get(name)["radii"] for b in BORDERS]


@functools.lru_cache(maxsize=None)
def expected(name, shape, r, b):
    """{op: (counts strings, boxes int64 [n, 4], areas int64 [n])} from the dense reference; computed once and shared"""
    per_mask = [ref.all_ops(m, shape, r, b) for m in get(name)["masks"]]
    out = {}
    for op in OPS:
        dense = [d[op] for d in per_mask]
        stats = [ref.box_and_area(d) for d in dense]
        out[op] = (tuple(rle.encode(np.asfortranarray(d))["counts"] for d in dense), np.asarray([s[0] for s in stats], np.int64).reshape(-1, 4),
                   np.asarray([s[1] for s in stats], np.int64))
    return out


def run(name, op, shape, r, b, ctx=None):
    return rle.morphology(list(rles(name)), op, shape, r, b, ctx=ctx, size=size(name), return_stats=True)


def result_bytes(res):
    out, boxes, areas = res
    return (tuple(bytes(x["counts"]) for x in out), boxes.tobytes(), areas.tobytes())


def equal_to(res, want, where):
    out, boxes, areas = res
    assert [bytes(x["counts"]) for x in out] == [bytes(c) for c in want[0]], where
    assert boxes.dtype == np.int64 and areas.dtype == np.int64 and boxes.tolist() == want[1].tolist() and areas.tolist() == want[2].tolist(), where


def check_case(name, shape, r, b, ctx=None):
    """every op of one case at one setting against the reference; {op: result}"""
    want, got = expected(name, shape, r, b), {}
    for op in OPS:
        got[op] = run(name, op, shape, r, b, ctx=ctx)
        equal_to(got[op], want[op], (name, op, shape, r, b))
        assert all(x["size"] == list(size(name)) for x in got[op][0])
    return got
