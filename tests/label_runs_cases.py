"""The case set of amp_label_runs, shared by tests/test_label_runs.py (host path) and tests/test_label_runs_gpu.py (device path).  A case is
{image, kind: 'binary' | 'label', connectivity}.  The reference shares no code with the run-based implementation: scipy.ndimage.label with
the cross or the full 3 x 3 structure ('binary') or np.unique ('label', id 0 skipped only when it is the smallest id, as the reference does),
then per instance the host codec on the dense mask rle.encode(np.asfortranarray(lab == v)), data_utils.extract_boxes and the pixel sum."""
import functools

import numpy as np
from scipy import ndimage

from ampis_amd import rle
from ampis_amd.data_utils import extract_boxes

N_SEEDED = 200
STRUCTURE = {1: ndimage.generate_binary_structure(2, 1), 2: np.ones((3, 3), int)}


def _binary(img, connectivity=2):
    return {"image": np.asarray(img, np.uint8), "kind": "binary", "connectivity": connectivity}


def _label(img):
    return {"image": np.asarray(img, np.int32), "kind": "label", "connectivity": 2}


def _tall(h):
    """A bar down column 1 across every 64-row word edge, a piece that ends on row 63 and one that starts on row 64 (where there is one)."""
    m = np.zeros((h, 5), np.uint8)
    m[1:h - 1, 1] = 1
    m[max(h - 70, 0):64, 3] = 1
    m[64:h, 4] = 1
    m[0, 3] = 1
    return m


def _spiral(n):
    """A one-pixel-wide spiral walked from the corner inwards, one clear pixel between its windings: one component, the longest chain of unions."""
    m = np.zeros((n, n), np.uint8)
    r, c, dr, dc = 0, 0, 0, 1
    m[0, 0] = 1
    inside = lambda y, x: 0 <= y < n and 0 <= x < n
    while True:
        for _ in range(2):                # straight on, else one turn to the right
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if inside(nr, nc) and not m[nr, nc] and not (inside(ar, ac) and m[ar, ac]):
                break
            dr, dc = dc, -dr
        else:
            return m
        r, c = nr, nc
        m[r, c] = 1


def _serpentine(n):
    m = np.zeros((n, n), np.uint8)
    m[:, ::2] = 1
    for k, c in enumerate(range(1, n, 2)):
        m[n - 1 if k % 2 == 0 else 0, c] = 1
    return m


def _rings(n):
    m = np.zeros((n, n), np.uint8)
    for k in range(0, n // 2, 2):
        m[k, k:n - k] = m[n - 1 - k, k:n - k] = 1
        m[k:n - k, k] = m[k:n - k, n - 1 - k] = 1
    return m


def _hand():
    c = {}
    c["one_set"] = _binary([[1]])
    c["one_clear"] = _binary([[0]])
    c["row_1x7"] = _binary([[1, 1, 0, 1, 0, 1, 1]])
    c["row_1x7_4"] = _binary([[1, 1, 0, 1, 0, 1, 1]], 1)
    c["col_7x1"] = _binary([[1], [1], [0], [1], [0], [1], [1]])
    c["empty"] = _binary(np.zeros((9, 11)))
    c["full"] = _binary(np.ones((9, 11)))
    for h in (63, 64, 65, 129):
        c[f"tall_{h}"] = _binary(_tall(h))
        c[f"tall_{h}_4"] = _binary(_tall(h), 1)
    diag = np.zeros((4, 4)); diag[1, 1] = diag[2, 2] = 1
    anti = np.zeros((4, 4)); anti[1, 2] = anti[2, 1] = 1
    c["diagonal_8"], c["diagonal_4"] = _binary(diag, 2), _binary(diag, 1)
    c["antidiagonal_8"], c["antidiagonal_4"] = _binary(anti, 2), _binary(anti, 1)
    board = (np.add.outer(np.arange(16), np.arange(16)) % 2 == 0)
    c["checkerboard_8"], c["checkerboard_4"] = _binary(board, 2), _binary(board, 1)
    wrap = np.zeros((6, 5)); wrap[5, 1] = wrap[0, 2] = 1; wrap[4:, 3] = 1; wrap[:2, 4] = 1      # last row of column c, first row of column c + 1
    c["column_wrap_8"], c["column_wrap_4"] = _binary(wrap, 2), _binary(wrap, 1)
    u = np.zeros((12, 9)); u[:, 1] = u[:, 7] = 1; u[11, 1:8] = 1; u[2:6, 4] = 1
    c["u_shape"] = _binary(u)
    ut = np.zeros((9, 12)); ut[1, :] = ut[7, :] = 1; ut[1:8, 11] = 1; ut[4, 2:6] = 1          # the arms meet only in the last column
    c["u_last_column"], c["u_last_column_4"] = _binary(ut, 2), _binary(ut, 1)
    comb = np.zeros((21, 30)); comb[::2, :] = 1; comb[:, 29] = 1
    c["comb_last_column"], c["comb_last_column_4"] = _binary(comb, 2), _binary(comb, 1)
    c["comb_last_row"] = _binary(comb.T.copy(), 1)
    c["spiral_65"], c["spiral_65_4"] = _binary(_spiral(65), 2), _binary(_spiral(65), 1)
    c["serpentine_65"], c["serpentine_65_4"] = _binary(_serpentine(65), 2), _binary(_serpentine(65), 1)
    c["rings_33"], c["rings_33_4"] = _binary(_rings(33), 2), _binary(_rings(33), 1)
    big = np.zeros((130, 130)); big[::3, :] = 1; big[:, 64] = 1; big[129, :] = 1; big[5:9, 100:104] = 0
    c["grid_130"] = _binary(big, 1)
    parts = np.zeros((10, 12), np.int32); parts[0:3, 0:3] = 7; parts[6:9, 8:11] = 7; parts[4, :] = 100; parts[0:2, 6:8] = 3; parts[9, 0] = 41
    c["label_parts"] = _label(parts)
    neg = parts.copy(); neg[8, 3:6] = -5
    c["label_negative"] = _label(neg)
    c["label_every_pixel"] = _label(np.random.default_rng(5).permutation(81).reshape(9, 9) + 1)
    c["label_every_pixel_0"] = _label(np.arange(81).reshape(9, 9))
    far = np.zeros((7, 6), np.int32); far[0, :] = 2 ** 31 - 1; far[6, :] = 2 ** 31 - 2; far[2:5, 1] = 1; far[2:5, 3] = 2 ** 30
    c["label_near_max"] = _label(far)
    far = far.copy(); far[3, 5] = -2 ** 31; far[5, 0:2] = -2 ** 31 + 1
    c["label_near_both_ends"] = _label(far)
    c["label_all_zero"] = _label(np.zeros((5, 4)))
    c["label_wrap"] = _label(np.array([[1, 2, 2], [1, 1, 2], [2, 1, 1]]))
    c["two_round_scans"] = _binary(_bands(257, 26300), 1)
    return c


def _bands(h, w):
    """Seven horizontal bands, so seven vertical runs in every column but one: the last band in the single row of the ragged fifth plane word,
    one across the word edge 63 | 64, one cut in two (eight instances).  At 257 x 26300: 131 500 plane words in 514 workgroups, so the first
    scan of the workgroup sums runs over 1028 entries, and 184 099 runs in 720 workgroups, so the second runs over 1440 -- both past the 1024
    entries that one round of the one-workgroup scan takes, neither a multiple of it."""
    m = np.zeros((h, w), np.uint8)
    for a, b in ((0, 1), (2, 4), (62, 66), (100, 128), (130, 131), (200, 201), (h - 1, h)):
        m[a:b, :] = 1
    m[130, w // 2] = 0                            # two instances from one band
    return m


HAND_CASES = _hand()
HAND = sorted(HAND_CASES)


@functools.lru_cache(maxsize=None)
def _seeded(i):
    rng = np.random.default_rng(9000 + i)
    h, w = (int(v) for v in rng.integers(1, 97, 2))
    density = float(rng.uniform(0.05, 0.95))
    if i % 2 == 0:
        blobs = ndimage.uniform_filter(rng.random((h, w)), size=1 + i % 5, mode="constant")
        thr = np.quantile(blobs, 1.0 - density)
        return _binary(blobs >= thr, 1 + (i // 2) % 2)
    ids = rng.integers(-2 if i % 4 == 3 else 0, 2 + i % 9, (h, w))
    ids[rng.random((h, w)) >= density] = 0
    return _label(ids * (1 + 1000 * (i % 3)))


def get(name):
    return _seeded(int(name[5:])) if name.startswith("seed_") else HAND_CASES[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(ids [N], boxes float64 [N, 4], areas [N], list of uint32 counts, int32 label image) by the reference; computed once a case."""
    c = get(name)
    img = c["image"]
    if c["kind"] == "binary":
        lab, n = ndimage.label(img != 0, structure=STRUCTURE[c["connectivity"]])
        ids = list(range(1, n + 1))
        labels = lab.astype(np.int32)
    else:
        lab = img
        u = np.unique(img)
        ids = [int(v) for v in (u[1:] if u.size and u[0] == 0 else u)]
        labels = np.zeros(img.shape, np.int32)
        for k, v in enumerate(ids):
            labels[img == v] = k + 1
    masks = [lab == v for v in ids]
    counts = [rle.string_to_counts(rle.encode(np.asfortranarray(m))["counts"]) for m in masks]
    boxes = np.array([extract_boxes(m)[0] for m in masks], np.float64).reshape(-1, 4)
    return np.array(ids, np.int64), boxes, np.array([int(m.sum()) for m in masks], np.int64), counts, labels


def run(name, ctx=None):
    """rle.label_runs on the case with the label image: (ids, boxes, areas, pool, off, len, labels)"""
    c = get(name)
    zero_bg = not (c["kind"] == "label" and c["image"].size and int(c["image"].min()) < 0)
    return rle.label_runs(c["image"], c["kind"], c["connectivity"], zero_bg, ctx=ctx, return_labels=True)


def check_case(name, ctx=None):
    """amp_label_runs on the case (ctx None: the host path) against the reference: ids, boxes, areas, every counts array byte for byte and the
    label image.  Returns the result."""
    res = run(name, ctx)
    ids, bx, areas, pool, off, ln, labels = res
    want_ids, want_boxes, want_areas, want_counts, want_labels = expected(name)
    assert ids.dtype == np.int32 and ids.tolist() == want_ids.tolist(), name
    assert areas.tolist() == want_areas.tolist(), name
    boxes = np.stack([bx[:, 1], bx[:, 0], bx[:, 3] - 1, bx[:, 2] - 1], axis=1).astype(np.float64).reshape(-1, 4)
    assert boxes.tobytes() == want_boxes.tobytes(), name
    assert len(off) == len(ln) == len(want_counts)
    at = 0
    for i, want in enumerate(want_counts):
        assert int(off[i]) == at, (name, i)                         # back to back, in instance order
        assert pool[at: at + int(ln[i])].tobytes() == want.astype(np.uint32).tobytes(), (name, i)
        at += int(ln[i])
    assert at == len(pool)
    assert labels.dtype == np.int32 and labels.shape == want_labels.shape and labels.tobytes() == np.ascontiguousarray(want_labels).tobytes(), name
    return res


def result_bytes(res):
    return [np.ascontiguousarray(a).tobytes() for a in res]
