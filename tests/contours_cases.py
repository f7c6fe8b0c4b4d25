"""The case set of amp_mask_contours, shared by tests/test_mask_contours.py (host path) and tests/test_mask_contours_gpu.py (device path).  A case
is {masks: bool [N, h, w], rles: the run lists handed to the call (the encoded masks unless the case brings looser ones)}; every case is run
at both connectivities.  The reference is tests/contours_ref.py, the dense edge walk of one decoded mask; the largest image (2^30 pixels) is
built from separate rectangles whose rings are written down by hand, because nothing dense of that size is made."""
import functools

import numpy as np

from ampis_amd import analyze, rle

import contours_ref as ref

N_SEEDED = 200
CONNECTIVITIES = (1, 2)


def _case(masks, rles=None):
    masks = np.asarray(masks).astype(bool)
    assert masks.ndim == 3
    return {"masks": masks, "rles": rles}


def _one(h, w, *pixels):
    m = np.zeros((1, h, w), bool)
    for r, c in pixels:
        m[0, r, c] = True
    return m


def _comb(teeth):
    """one-pixel teeth on a one-pixel spine: a single ring with 2 * teeth + ... nodes"""
    m = np.zeros((1, 3, 2 * teeth - 1), bool)
    m[0, 2, :] = True
    m[0, :, ::2] = True
    return m


def _spiral(n):
    """a one-pixel arm that winds inwards with a free pixel between its turns: one long ring"""
    m = np.zeros((n, n), bool)
    r, c, dr, dc = 0, 0, 0, 1
    m[0, 0] = True
    moved = True
    while moved:
        moved = False
        for _ in range(2):                        # straight on, or one turn to the right
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if 0 <= nr < n and 0 <= nc < n and not m[nr, nc] and not (0 <= ar < n and 0 <= ac < n and m[ar, ac]):
                r, c, moved = nr, nc, True
                m[r, c] = True
                break
            dr, dc = dc, -dr
    return m[None]


def _hand():
    c = {}
    c["empty"] = _case(np.zeros((1, 5, 6), bool))
    c["full"] = _case(np.ones((1, 5, 6), bool))
    for h, w in ((1, 1), (1, 9), (9, 1)):
        c[f"full_{h}x{w}"] = _case(np.ones((1, h, w), bool))
        c[f"dots_{h}x{w}"] = _case(np.stack([np.arange(h * w).reshape(h, w) % 2 == 0, np.arange(h * w).reshape(h, w) % 3 == 1]))
    c["corner_pixels"] = _case(np.concatenate([_one(4, 5, (0, 0)), _one(4, 5, (0, 4)), _one(4, 5, (3, 0)), _one(4, 5, (3, 4)),
                                               _one(4, 5, (0, 0), (0, 4), (3, 0), (3, 4))]))
    c["two_diagonal_pixels"] = _case(np.concatenate([_one(4, 4, (1, 1), (2, 2)), _one(4, 4, (1, 2), (2, 1)), _one(4, 4, (0, 0), (1, 1))]))
    c["checkerboard_7x7"] = _case(np.stack([np.add.outer(np.arange(7), np.arange(7)) % 2 == 0, np.add.outer(np.arange(7), np.arange(7)) % 2 == 1]))
    frame = np.ones((1, 6, 7), bool); frame[0, 2:4, 2:5] = False
    c["frame_with_hole"] = _case(frame)
    island = np.ones((1, 9, 9), bool); island[0, 2:7, 2:7] = False; island[0, 4, 4] = True
    c["hole_with_island"] = _case(island)
    ch = np.ones((1, 9, 8), bool)                                                       # a hole like a C turned round: its first column holds the two arms
    ch[0, 1:8, 2:6] = False; ch[0, 3:6, 2:5] = True
    c["c_shaped_hole"] = _case(ch)
    dg = np.ones((1, 6, 6), bool); dg[0, 1:3, 1:3] = False; dg[0, 0, 0] = False          # the hole meets the outside zero at a corner only
    dg2 = np.zeros((1, 6, 6), bool); dg2[0, 1:5, 1:5] = True; dg2[0, 2:4, 2:4] = False; dg2[0, 1, 1] = False
    c["hole_touching_outside_diagonally"] = _case(np.concatenate([dg, dg2]))
    c["spiral_33"] = _case(_spiral(33))
    for t in (127, 128, 129, 257):
        c[f"comb_{t}"] = _case(_comb(t))
    cols = np.zeros((1, 5, 4), bool); cols[0, :, 1] = True; cols[0, 3:, 0] = True; cols[0, :2, 2] = True      # runs joined across column ends
    c["runs_joined_across_column_ends"] = _case(np.concatenate([cols, np.ones((1, 5, 4), bool)]))
    loose = [{"size": [4, 3], "counts": np.array([0, 0, 0, 2, 0, 3, 2, 0, 0, 1, 4], np.uint32)},      # zero-length runs, a run across a column end
             {"size": [4, 3], "counts": np.array([3, 0, 0, 4, 5, 0], np.uint32)},
             {"size": [4, 3], "counts": np.array([0, 4, 0, 4, 0, 4], np.uint32)}]         # three pieces that a canonical list holds as one run
    c["zero_length_runs"] = _case(np.stack([rle.decode(r).astype(bool) for r in loose]), loose)
    board = np.add.outer(np.arange(66), np.arange(3)) % 2 == 0
    c["mask_66x3"] = _case(np.stack([board, ~board, np.ones((66, 3), bool)]))
    c["pool_of_0"] = _case(np.zeros((0, 6, 7), bool))
    rng = np.random.default_rng(65)
    c["pool_of_1"] = _case(rng.random((1, 12, 13)) < 0.5)
    c["pool_of_65"] = _case(rng.random((65, 9, 10)) < np.linspace(0.0, 1.0, 65)[:, None, None])
    return c


HAND_CASES = _hand()
HAND = sorted(HAND_CASES)


@functools.lru_cache(maxsize=None)
def _seeded(i):
    rng = np.random.default_rng(73000 + i)
    n, h, w = int(rng.integers(1, 7)), int(rng.integers(1, 41)), int(rng.integers(1, 41))
    return _case(rng.random((n, h, w)) < (0.3, 0.5, 0.7, 0.9)[i % 4])


SEEDED = [f"seed_{i}" for i in range(N_SEEDED)]
LARGEST = ["largest_32768x1", "largest_1x32768", "largest_32768x32768"]

# the rectangles {r0, r1, c0, c1} (ends exclusive) of the 2^30-pixel image: apart from each other, corners included, so each is one ring
BIG = 32768
BIG_RECTS = [(0, 1, 0, 1), (5, 7, 10, 32760), (100, 32700, 32766, 32767), (32767, 32768, 32767, 32768), (32760, 32768, 0, 3), (0, 32768, 32764, 32765)]


def _big_rle():
    """the run list of BIG_RECTS without a dense image: the pieces of every column in order, touching pieces joined"""
    s = np.concatenate([np.arange(c0, c1, dtype=np.int64) * BIG + r0 for r0, r1, c0, c1 in BIG_RECTS])
    e = np.concatenate([np.arange(c0, c1, dtype=np.int64) * BIG + r1 for r0, r1, c0, c1 in BIG_RECTS])
    order = np.argsort(s, kind="stable")
    s, e = s[order], e[order]
    assert (s[1:] >= e[:-1]).all()
    keep = np.ones(len(s), bool)
    keep[1:] = s[1:] > e[:-1]                                      # a piece that starts where the one before ends is the same run
    starts, ends = s[keep], e[np.append(keep[1:], True)]
    bounds = np.stack([starts, ends], axis=1).reshape(-1)
    counts = np.diff(np.concatenate([[0], bounds, [BIG * BIG]]))
    if counts[-1] == 0:
        counts = counts[:-1]
    return {"size": [BIG, BIG], "counts": counts.astype(np.uint32)}


@functools.lru_cache(maxsize=None)
def _large(name):
    if name == LARGEST[2]:
        return {"masks": None, "rles": [_big_rle()]}
    h, w = (BIG, 1) if name == LARGEST[0] else (1, BIG)
    m = np.zeros((2, h * w), bool)
    m[0] = True
    m[1, :3] = True; m[1, 5] = True; m[1, 16380:16390] = True; m[1, 32766:] = True
    return _case(m.reshape(2, h, w))


def get(name):
    if name.startswith("seed_"):
        return _seeded(int(name[5:]))
    return _large(name) if name in LARGEST else HAND_CASES[name]


def _encode(m):
    return rle.string_to_counts(rle.encode(np.asfortranarray(m))["counts"])


@functools.lru_cache(maxsize=None)
def rles(name):
    c = get(name)
    if c["rles"] is not None:
        return c["rles"]
    return [{"size": list(c["masks"].shape[1:]), "counts": _encode(m)} for m in c["masks"]]


def size(name):
    c = get(name)
    return (BIG, BIG) if c["masks"] is None else tuple(int(v) for v in c["masks"].shape[1:])


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """per mask the reference's rings [{'xy', 'area2', 'length'}]; computed once a case and connectivity"""
    c = get(name)
    if c["masks"] is None:                                           # the rectangles: (c0, r0), (c1, r0), (c1, r1), (c0, r1), by (c0, r0)
        out = [{"xy": np.array([(c0, r0), (c1, r0), (c1, r1), (c0, r1)], np.int32), "area2": 2 * (r1 - r0) * (c1 - c0),
                "length": 2 * (r1 - r0) + 2 * (c1 - c0)} for r0, r1, c0, c1 in sorted(BIG_RECTS, key=lambda q: (q[2], q[0]))]
        return [out]
    return [ref.rings(m, connectivity) for m in c["masks"]]


def capacity_bound(name):
    """the capacities the header states: four vertices and two rings per piece, pieces <= runs of ones + columns of the tight box (here: of the
    image, which is no narrower)"""
    pieces = sum(len(r["counts"]) // 2 + int(r["size"][1]) for r in rles(name))
    return 4 * pieces, 2 * pieces


def run(name, connectivity, ctx=None):
    return rle.mask_contours(rles(name), connectivity, ctx=ctx, size=size(name))


def result_bytes(res):
    return [a.tobytes() for a in res]


def check_case(name, connectivity, ctx=None):
    """amp_mask_contours on the case (ctx None: the host path) against the reference ring for ring, and the identities of the definition: the
    areas sum to the mask's, the outer and hole rings are mask_topology's parts and holes, the lengths sum to the crack perimeter counted
    densely, and the stated capacities hold.  Returns the result."""
    res = run(name, connectivity, ctx)
    first, off, ln, area2, length, xy = res
    want = expected(name, connectivity)
    n = len(want)
    assert first.dtype == off.dtype == ln.dtype == area2.dtype == length.dtype == np.int64 and xy.dtype == np.int32, name
    assert first.shape == (n + 1,) and first[0] == 0 and xy.shape == (int(ln.sum()), 2), name
    assert [int(first[i + 1] - first[i]) for i in range(n)] == [len(w) for w in want], (name, connectivity)
    at = 0
    for i in range(n):
        for k, w in enumerate(want[i]):
            r = int(first[i]) + k
            assert int(off[r]) == at and int(ln[r]) == len(w["xy"]), (name, connectivity, i, k)
            assert xy[at: at + len(w["xy"])].tobytes() == w["xy"].tobytes(), (name, connectivity, i, k)
            assert int(area2[r]) == w["area2"] and int(length[r]) == w["length"], (name, connectivity, i, k)
            at += len(w["xy"])
    vcap, rcap = capacity_bound(name)
    assert len(xy) <= vcap and len(off) <= rcap, name
    masks = get(name)["masks"]
    if masks is not None and n:
        topo = analyze.mask_topology(rles(name), connectivity, device="cpu")
        for i in range(n):
            a2, le = area2[first[i]: first[i + 1]], length[first[i]: first[i + 1]]
            assert int(a2.sum()) == 2 * int(masks[i].sum()), (name, connectivity, i)
            assert int((a2 > 0).sum()) == int(topo["n_parts"][i]) and int((a2 < 0).sum()) == int(topo["n_holes"][i]), (name, connectivity, i)
            assert int(le.sum()) == ref.crack_perimeter(masks[i]), (name, connectivity, i)
    return res
