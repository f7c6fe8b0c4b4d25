"""The case set of amp_flatten_instances, shared by tests/test_flatten.py (host path) and tests/test_flatten_gpu.py (device path).  A case is
{masks: bool [N, h, w], rank: uint32 [N] or None, rles: the run lists handed to the call (the encoded masks unless the case brings looser ones)}.

The reference shares no code with the run-based implementation: the dense loop users run today.  order = lexsort((arange(n), rank)), then
labels[mask_i] = i + 1 for i in reversed order; the visible list of instance i is the host codec's rle.encode(labels == i + 1); statistics,
boxes and pixel classes come from the dense arrays.  Two more checks on every case: analyze.label_image_to_rle(labels, 'label') -- the inverse
-- gives the non-empty visible lists in index order, and the visible areas sum to the area of rle.merge(all masks)."""
import functools

import numpy as np

from ampis_amd import analyze, rle

N_SEEDED = 200
TOP = 0xFFFFFFFF


def _case(masks, rank=None, rles=None):
    masks = np.asarray(masks).astype(bool)
    assert masks.ndim == 3
    return {"masks": masks, "rank": None if rank is None else np.asarray(rank, dtype=np.uint32), "rles": rles}


def _ring(h, w, d, t=1):
    """the pixels whose distance to the border of the h x w image is d .. d + t - 1"""
    r, c = np.mgrid[:h, :w]
    k = np.minimum(np.minimum(r, h - 1 - r), np.minimum(c, w - 1 - c))
    return (k >= d) & (k < d + t)


def _edges(h, w, seed):
    """four masks that cross the 64-row and 64-column tile edges where the image has them: everything, a band of columns, a band of rows, noise"""
    rng = np.random.default_rng(seed)
    m = np.zeros((4, h, w), bool)
    m[0] = True
    m[1][:, max(0, min(w - 1, 60)): 69] = True
    m[2][max(0, min(h - 1, 61)): 67, :] = True
    m[3] = rng.random((h, w)) < 0.4
    return _case(m, [3, 1, 1, 0])


def _hand():
    c = {}
    for h, w in ((1, 1), (1, 70), (70, 1), (64, 64), (65, 65), (130, 40), (40, 130)):
        c[f"edges_{h}x{w}"] = _edges(h, w, 7 * h + w)
    blobs = np.zeros((3, 9, 11), bool)
    blobs[0, 1:5, 1:6] = True; blobs[1, 3:8, 4:10] = True; blobs[2, 0:3, 8:11] = True
    full = np.ones((1, 9, 11), bool)
    c["full_under"] = _case(np.concatenate([blobs, full]))                              # index order: the full mask keeps what is left
    c["full_over"] = _case(np.concatenate([full, blobs]))                               # ... or takes everything
    c["full_over_by_rank"] = _case(np.concatenate([blobs, full]), [5, 5, 5, 1])
    c["two_identical"] = _case(np.stack([blobs[0], blobs[0]]))                          # the loser owns nothing
    c["two_identical_second_wins"] = _case(np.stack([blobs[0], blobs[0]]), [9, 2])
    rings = np.stack([_ring(15, 15, 1, 4), _ring(15, 15, 3, 4)])                        # they share the rings at distance 3 and 4
    c["ring_in_ring_outer_on_top"] = _case(rings, [0, 1])
    c["ring_in_ring_inner_on_top"] = _case(rings, [1, 0])
    under = np.ones((5, 4), bool)                                                       # one run across every column end
    cut = np.zeros((5, 4), bool); cut[:, 1] = True                                      # a whole column: the cuts are at column ends
    c["join_across_column_ends"] = _case(np.stack([under, cut]), [1, 0])                # visible: [0, 5) and [10, 20), the second across a column end
    cut2 = np.zeros((5, 4), bool); cut2[0:4, 1] = True
    c["join_across_column_ends_partial"] = _case(np.stack([under, cut2]), [1, 0])       # [0, 5) and [9, 20)
    stripes = np.zeros((6, 5), bool); stripes[4:, :] = True; stripes[:2, :] = True      # every run crosses a column end
    cut3 = np.zeros((6, 5), bool); cut3[:, 2] = True; cut3[0, 3] = True
    c["runs_across_column_ends_cut"] = _case(np.stack([cut3, stripes]))
    empty = np.zeros((1, 9, 11), bool)
    c["empty_first_middle_last"] = _case(np.concatenate([empty, blobs[:2], empty, blobs[2:], empty]), [0, 4, 3, 0, 9, 1])
    c["only_empty"] = _case(np.concatenate([empty, empty]))
    c["no_mask"] = _case(np.zeros((0, 6, 7), bool))
    c["ranks_all_equal"] = _case(np.concatenate([blobs, full]), [7, 7, 7, 7])
    c["ranks_descending"] = _case(np.concatenate([blobs, full]), [9, 6, 4, 2])
    c["ranks_zero_and_top"] = _case(np.concatenate([full, blobs]), [TOP, 0, TOP, 0])
    loose = [{"size": [4, 3], "counts": np.array([0, 0, 0, 2, 0, 3, 2, 0, 0, 1, 4], np.uint32)},      # zero-length runs, a run across a column end
             {"size": [4, 3], "counts": np.array([3, 0, 0, 4, 5, 0], np.uint32)}]
    c["loose_run_lists"] = _case(np.stack([rle.decode(r).astype(bool) for r in loose]), [1, 0], loose)
    rng = np.random.default_rng(300)
    many = np.zeros((300, 70, 70), bool)
    many[:, 30:38, 30:38] = True                                                        # more hits in one tile than any staging of 64 or 256
    many[np.arange(300), 10 + np.arange(300) // 60, np.arange(300) % 60] = True         # and a pixel of its own each
    c["300_on_one_block"] = _case(many, rng.integers(0, 40, 300))
    dots = np.zeros((5041, 71, 71), bool)
    at = np.random.default_rng(5041).permutation(5041)
    dots[np.arange(5041), at // 71, at % 71] = True
    c["5041_single_pixels"] = _case(dots)
    board = np.add.outer(np.arange(66), np.arange(3)) % 2 == 0
    c["checkerboard_66x3"] = _case(np.stack([board, ~board]))                           # the most runs per pixel
    c["checkerboard_66x3_full_under"] = _case(np.stack([np.ones((66, 3), bool), board]), [1, 0])
    # 257 x 26300, the label image in horizontal bands of three owners, six or seven vertical runs a column: 131 500 plane words in 514
    # workgroups, so the first scan of the workgroup sums runs over 1028 entries, and 7 x 26300 - 15000 = 169 100 runs in 661 workgroups, so
    # the second runs over 1322 -- both past the 1024 entries that one round of the one-workgroup scan takes, neither a multiple of it; the
    # last band is the single row of the ragged fifth plane word, one band crosses the word edge 63 | 64
    bands = np.zeros((3, 257, 26300), bool)
    for k, (a, b) in enumerate(((0, 1), (2, 4), (62, 66), (100, 128), (130, 131), (200, 201), (256, 257))):
        bands[k % 2, a:b, :] = True
    bands[2, 90:140, 5000:20000] = True                                                 # on top by rank: it swallows two bands where it lies
    c["two_round_scans"] = _case(bands, [1, 2, 0])
    return c


HAND_CASES = _hand()
HAND = sorted(HAND_CASES)


def _largest(tall):
    """the largest sides, 32768 x 2 or 2 x 32768: three masks whose runs lie around the last rows / columns"""
    h, w = (32768, 2) if tall else (2, 32768)
    m = np.zeros((3, h, w), bool)
    m[0] = True
    if tall:
        m[1][32700:, 0] = True; m[1][:100, 1] = True; m[2][32767, :] = True; m[2][16384:16450, 1] = True
    else:
        m[1][:, 32700:] = True; m[2][1, 32767] = True; m[2][:, 16384:16450] = True
    return _case(m, [2, 1, 0])


LARGEST = ["largest_32768x2", "largest_2x32768"]


@functools.lru_cache(maxsize=None)
def _seeded(i):
    rng = np.random.default_rng(52000 + i)
    h, w, n = int(rng.integers(1, 141)), int(rng.integers(1, 141)), int(rng.integers(1, 13))
    if i % 2 == 0:
        masks = rng.random((n, h, w)) < float(rng.choice([0.05, 0.3, 0.6]))
    else:                                        # rectangles: long runs, real overlaps
        masks = np.zeros((n, h, w), bool)
        for m in masks:
            r0, c0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            m[r0: r0 + int(rng.integers(1, h + 1)), c0: c0 + int(rng.integers(1, w + 1))] = True
        masks &= rng.random((n, h, w)) < 0.97
    rank = None if i % 5 == 0 else rng.integers(0, int(rng.choice([2, 4, 1000])), n)     # ties
    return _case(masks, rank)


@functools.lru_cache(maxsize=None)
def _large(name):
    return _largest(name == LARGEST[0])


def get(name):
    if name.startswith("seed_"):
        return _seeded(int(name[5:]))
    return _large(name) if name in LARGEST else HAND_CASES[name]


def names():
    return HAND + [f"seed_{i}" for i in range(N_SEEDED)]


def _encode(m):
    return rle.string_to_counts(rle.encode(np.asfortranarray(m))["counts"])


@functools.lru_cache(maxsize=None)
def rles(name):
    c = get(name)
    if c["rles"] is not None:
        return c["rles"]
    return [{"size": list(c["masks"].shape[1:]), "counts": _encode(m)} for m in c["masks"]]


def size(name):
    return tuple(int(v) for v in get(name)["masks"].shape[1:])


def capacity_bound(name):
    """the capacity the header states: 2 x the sum of the input lists' lengths"""
    return 2 * sum(len(r["counts"]) for r in rles(name))


@functools.lru_cache(maxsize=None)
def expected(name):
    """{'labels' int32 [h, w], 'counts' list of uint32 arrays, 'stats' [n, 2], 'boxes' [n, 4], 'pixels' [3]} by the dense loop; once a case"""
    c = get(name)
    masks = c["masks"]
    n, h, w = masks.shape
    rank = np.arange(n) if c["rank"] is None else c["rank"]
    order = np.lexsort((np.arange(n), rank))
    labels = np.zeros((h, w), np.int32)
    for i in order[::-1]:
        labels[masks[i]] = i + 1
    counts, stats, boxes = [], np.zeros((n, 2), np.int64), np.zeros((n, 4), np.int64)
    for i in range(n):
        vis = labels == i + 1
        counts.append(_encode(vis))
        stats[i] = (int(masks[i].sum()), int(vis.sum()))
        if vis.any():
            rr, cc = np.flatnonzero(vis.any(axis=1)), np.flatnonzero(vis.any(axis=0))
            boxes[i] = (rr[0], cc[0], rr[-1] + 1, cc[-1] + 1)
    cover = masks.sum(axis=0, dtype=np.int64) if n else np.zeros((h, w), np.int64)
    pixels = np.array([(cover == 0).sum(), (cover == 1).sum(), (cover >= 2).sum()], np.int64)
    labels.setflags(write=False)
    return {"labels": labels, "counts": counts, "stats": stats, "boxes": boxes, "pixels": pixels}


def run(name, ctx=None, emit=True, return_labels=True):
    return rle.flatten_instances(rles(name), get(name)["rank"], ctx=ctx, emit=emit, return_labels=return_labels, size=size(name))


def check_case(name, ctx=None):
    """amp_flatten_instances on the case (ctx None: the host path) against the reference -- labels, every visible list byte for byte, stats,
    boxes, pixels --, the inverse through label_image_to_rle, the area of the union, the stated capacity bound, and the statistics-only call.
    Returns the result."""
    res = run(name, ctx)
    stats, boxes, pixels, counts, labels = res
    want = expected(name)
    n, (h, w) = len(want["counts"]), size(name)
    assert labels.dtype == np.int32 and labels.shape == (h, w) and labels.tobytes() == want["labels"].tobytes(), name
    assert stats.dtype == np.int64 and stats.tolist() == want["stats"].tolist(), name
    assert boxes.dtype == np.int64 and boxes.tolist() == want["boxes"].tolist(), name
    assert pixels.dtype == np.int64 and pixels.tolist() == want["pixels"].tolist() and int(pixels.sum()) == h * w, name
    assert len(counts) == n
    for i, (got, wanted) in enumerate(zip(counts, want["counts"])):
        assert got.dtype == np.uint32 and got.tobytes() == wanted.astype(np.uint32).tobytes(), (name, i)
    assert sum(len(x) for x in counts) <= capacity_bound(name), name                    # the bound of the header (the wrapper's capacity is this bound)
    # the inverse: the label image read back gives the non-empty visible lists in index order
    back, _, areas, ids = analyze.label_image_to_rle(labels, "label", device="cpu")
    owners = [i for i in range(n) if stats[i, 1] > 0]
    assert ids.tolist() == [i + 1 for i in owners] and areas.tolist() == [int(stats[i, 1]) for i in owners], name
    assert [r["counts"] for r in back] == [rle.counts_to_string(counts[i]) for i in owners], name
    # the visible masks tile the union
    union = rle.area(rle.merge(rles(name))) if n else 0
    assert int(stats[:, 1].sum()) == union == int(pixels[1] + pixels[2]), name
    only = run(name, ctx, emit=False, return_labels=False)
    assert only[3] is None and all(a.tobytes() == b.tobytes() for a, b in zip(only[:3], res[:3])), name
    return res


def result_bytes(res):
    return [a.tobytes() for a in res[:3]] + [a.tobytes() for a in res[3]] + [res[4].tobytes()]
