"""The case set of amp_rle_overlap_groups, shared by tests/test_rle_overlap.py (host path) and tests/test_rle_overlap_gpu.py (device path).
A case is a list of groups (A masks, B masks) as RLE dicts plus the expected [na, nb] pixel counts and the areas, which come from a brute-force
numpy evaluation on the decoded bitmaps ((A[:, None] & B[None]).sum) -- computed once per process -- or, for the one image too large to decode,
from the closed form.  The smallest shapes at which the run-list arithmetic can go wrong: see the comment of each case."""
import functools

import numpy as np

from ampis_amd import rle

H, W = 40, 50


def enc(m):
    return rle.encode(np.asfortranarray(np.asarray(m).astype(np.uint8)))


def from_positions(h, w, spans):
    """mask of the column-major pixel positions [s, e) of `spans`"""
    flat = np.zeros(h * w, bool)
    for s, e in spans:
        flat[s:e] = True
    return flat.reshape(w, h).T.copy()


def k_runs(k, phase=0, on=2, period=3):
    """k runs of `on` ones, one every `period` pixels from `phase` on"""
    return from_positions(H, W, [(phase + period * i, phase + period * i + on) for i in range(k)])


def disc(h, w, cy, cx, ry, rx=None):
    yy, xx = np.ogrid[:h, :w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / (rx or ry)) ** 2 <= 1.0


def brute(a, b):
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int64)
    a, b = np.asarray(a, bool).reshape(len(a), -1), np.asarray(b, bool).reshape(len(b), -1)
    return (a[:, None] & b[None]).sum(axis=2, dtype=np.int64)


def group(a, b, shape):
    """(A rles, B rles, expected inter, expected areas of A, of B) of bool masks a, b of one `shape`"""
    a, b = [np.asarray(m, bool) for m in a], [np.asarray(m, bool) for m in b]
    assert all(m.shape == shape for m in a + b)
    return ([enc(m) for m in a], [enc(m) for m in b], brute(a, b), np.array([m.sum() for m in a], np.int64), np.array([m.sum() for m in b], np.int64))


def _stripes(h, w, n, by_rows):
    out = []
    for i in range(n):
        idx = np.arange(h if by_rows else w)
        on = ((idx + i) % (2 + i % 5)) == 0
        on[0] = on[-1] = True                                # every box is the whole image
        m = np.zeros((h, w), bool)
        if by_rows:
            m[on, :] = True
        else:
            m[:, on] = True
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    z = lambda: np.zeros((H, W), bool)
    full = np.ones((H, W), bool)
    c = {}
    # 1, 63, 64, 65 and 129 runs of ones on both sides: the lanes' stride over the shorter list ends before / on / after one round of 64, and
    # every pair takes the branch "A has fewer runs" or the other; the B lists are out of phase, so runs overlap partly, fully and not at all
    counts = (1, 63, 64, 65, 129)
    c["run_counts"] = [group([k_runs(k) for k in counts], [k_runs(k, phase=1) for k in counts] + [k_runs(k, phase=7, on=4, period=5) for k in counts], (H, W))]
    # a run that crosses column borders (rows 37 .. 39 of column 3, all of column 4, rows 0 .. 4 of column 5) against boxes and single columns
    cross = from_positions(H, W, [(3 * H + 37, 5 * H + 5)])
    col4, box = z(), z()
    col4[:, 4] = True
    box[35:, 2:6] = True
    c["column_crossing"] = [group([cross, col4], [cross, col4, box, full], (H, W))]
    # one-pixel masks in the corners and the middle, the full image, empty masks (rows and columns of zeros)
    px = []
    for r, q in ((0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1), (17, 23)):
        m = z()
        m[r, q] = True
        px.append(m)
    c["pixels_full_empty"] = [group(px + [full, z()], [z()] + px + [full], (H, W))]
    # the end of a run of one mask is the start of a run of the other (no common pixel), by one more (one common pixel), and equal masks
    a = from_positions(H, W, [(100, 150), (400, 410)])
    c["touching_and_equal"] = [group([a, a], [from_positions(H, W, [(150, 400)]), from_positions(H, W, [(149, 401)]), a,
                                              from_positions(H, W, [(0, 100), (150, 400), (410, H * W)])], (H, W))]
    # dense: row stripes against column stripes, every tight box is the whole image, the box test rejects nothing
    c["dense_stripes"] = [group(_stripes(H, W, 9, True), _stripes(H, W, 70, False), (H, W))]
    # tiles that are no multiple of 64: 3 x 67 and 70 x 1
    r = np.random.default_rng(20261017)
    blob = lambda: disc(H, W, r.integers(0, H), r.integers(0, W), r.integers(2, 9), r.integers(2, 9))
    c["tile_3x67"] = [group([blob() for _ in range(3)], [blob() for _ in range(67)], (H, W))]
    c["tile_70x1"] = [group([blob() for _ in range(70)], [blob()], (H, W))]
    # three groups of different sizes in one call, one without A masks and one without B masks: the blocks of `inter` follow each other
    rb = lambda h, w: disc(h, w, r.integers(0, h), r.integers(0, w), r.integers(2, 12), r.integers(2, 12))
    c["three_groups"] = [group([rb(33, 17) for _ in range(5)], [rb(33, 17) for _ in range(66)], (33, 17)),
                         group([], [rb(9, 70) for _ in range(3)], (9, 70)),
                         group([rb(64, 65) for _ in range(4)], [], (64, 65)),
                         group([rb(64, 65) for _ in range(2)], [rb(64, 65) for _ in range(3)], (64, 65))]
    c["no_groups"] = []
    # run positions beyond 2^20 on a micrograph-sized image
    h, w = 1024, 1536
    big_a = [disc(h, w, 955, 1465, 60, 62), disc(h, w, 500, 1100, 200, 150)]
    big_b = [disc(h, w, 962, 1472, 58, 61), disc(h, w, 600, 1200, 90), np.ones((h, w), bool)]
    assert big_a[0].T.reshape(-1).nonzero()[0].min() > 1 << 20
    c["large_offsets"] = [group(big_a, big_b, (h, w))]
    # the size limit: one run of 2^30 ones against itself (never decoded)
    n = 32768
    one = {"size": [n, n], "counts": np.array([0, n * n], np.uint32)}
    c["full_image_at_the_limit"] = [([one], [one], np.array([[n * n]], np.int64), np.array([n * n], np.int64), np.array([n * n], np.int64))]
    return c


NAMES = ("run_counts", "column_crossing", "pixels_full_empty", "touching_and_equal", "dense_stripes", "tile_3x67", "tile_70x1", "three_groups",
         "no_groups", "large_offsets", "full_image_at_the_limit")


def check_case(name, ctx=None):
    """amp_rle_overlap_groups on all groups of the case in ONE call (ctx None: the host path): every count and area exactly.  Returns the arrays."""
    groups = cases()[name]
    inters, aa, ab = rle.overlap_groups([g[0] for g in groups], [g[1] for g in groups], ctx=ctx)
    assert len(inters) == len(aa) == len(ab) == len(groups)
    for k, g in enumerate(groups):
        assert inters[k].dtype == np.int64 and inters[k].shape == g[2].shape, (name, k, inters[k].shape)
        assert np.array_equal(inters[k], g[2]), (name, k, np.argwhere(inters[k] != g[2])[:5])
        assert np.array_equal(aa[k], g[3]) and np.array_equal(ab[k], g[4]), (name, k)
    return inters, aa, ab
