"""The reference of tests/test_region_props.py and tests/test_region_props_gpu.py: skimage.measure.regionprops' definitions (rc coordinates,
0.16 and later) evaluated the way skimage evaluates them, on dense masks, independently of the run-length / bit-plane method of the library:

  * the sums from np.nonzero in Python integers;
  * the perimeter from scipy.ndimage.binary_erosion + convolve with [[10, 2, 10], [2, 1, 2], [10, 2, 10]] + bincount, skimage's codes grouped into
    the three weight classes;
  * the convex area from a brute-force test of every pixel centre of the box against every edge of a plain-Python integer hull (Andrew's chain
    over the edge midpoints, in half-pixel units, of the pixels skimage's possible_hull keeps: the first and last of every row and column);
  * convex_area_qhull: skimage's own formulation -- qhull on the offset points and `equations . x + d < 1e-10` -- which the tests hold equal to
    the integer form on every mask they use;
  * exact_floats: the derived floats in exact rationals / 60-digit decimals.
skimage itself is not available to these tests, so this file, not a recorded vector, is what the library is held to (unpinned parity).
The test masks live here too, each with its reference integers computed once per process."""
import functools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import scipy.ndimage as ndi
import scipy.spatial

getcontext().prec = 60

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
KERNEL = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
FLOAT_KEYS = ("centroid-0", "centroid-1", "eccentricity", "equivalent_diameter", "extent", "major_axis_length", "minor_axis_length", "orientation",
              "perimeter", "solidity")


def perimeter_classes(mask):
    if not mask.any():
        return 0, 0, 0
    border = mask & ~ndi.binary_erosion(mask, CROSS, border_value=0)
    hist = np.bincount(ndi.convolve(border.astype(np.int64), KERNEL, mode="constant", cval=0).ravel(), minlength=50)
    return int(hist[[5, 7, 15, 17, 25, 27]].sum()), int(hist[[21, 33]].sum()), int(hist[[13, 23]].sum())


def _hull_candidates(mask):
    """Half-pixel (Y, X) edge midpoints of the first and last pixel of every row and column (skimage's possible_hull + offset_coordinates)."""
    pix = set()
    for r in np.flatnonzero(mask.any(axis=1)).tolist():
        c = np.flatnonzero(mask[r])
        pix.update(((r, int(c[0])), (r, int(c[-1]))))
    for c in np.flatnonzero(mask.any(axis=0)).tolist():
        r = np.flatnonzero(mask[:, c])
        pix.update(((int(r[0]), c), (int(r[-1]), c)))
    pts = set()
    for r, c in pix:
        pts.update(((2 * r - 1, 2 * c), (2 * r + 1, 2 * c), (2 * r, 2 * c - 1), (2 * r, 2 * c + 1)))
    return sorted(pts)


def _integer_hull(pts):
    """Andrew's monotone chain on sorted integer points -> the hull's vertices in one orientation, collinear points dropped."""
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _box(mask):
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1


def convex_area_integer(mask):
    """Pixel centres (2 r, 2 c) of the box with cross >= 0 against every edge of the integer hull."""
    if not mask.any():
        return 0
    hull = _integer_hull(_hull_candidates(mask))
    r0, c0, r1, c1 = _box(mask)
    Y, X = np.meshgrid(2 * np.arange(r0, r1, dtype=np.int64), 2 * np.arange(c0, c1, dtype=np.int64), indexing="ij")
    edges = list(zip(hull, hull[1:] + hull[:1]))
    turn = 1 if sum(a[0] * b[1] - a[1] * b[0] for a, b in edges) > 0 else -1      # the orientation the chain came out in
    inside = np.ones(Y.shape, bool)
    for (ay, ax), (by, bx) in edges:
        inside &= turn * ((by - ay) * (X - ax) - (bx - ax) * (Y - ay)) >= 0
    return int(inside.sum())


def convex_area_qhull(mask):
    """skimage.morphology.convex_hull_image(mask, offset_coordinates=True).sum(): qhull on the offset points, a centre counts when
    equations . x + d < 1e-10 for every facet."""
    if not mask.any():
        return 0
    pts = np.array(_hull_candidates(mask), dtype=np.float64) / 2.0
    eq = scipy.spatial.ConvexHull(pts).equations
    r0, c0, r1, c1 = _box(mask)
    grid = np.stack(np.meshgrid(np.arange(r0, r1, dtype=np.float64), np.arange(c0, c1, dtype=np.float64), indexing="ij"), axis=-1).reshape(-1, 2)
    return int(np.all(grid @ eq[:, :2].T + eq[:, 2] < 1e-10, axis=1).sum())


def ref_integers(mask):
    """(bbox, [13 integers]) of one dense bool mask: what amp_mask_region_props must return."""
    mask = np.asarray(mask, bool)
    if not mask.any():
        return (0, 0, 0, 0), [0] * 13
    rr, cc = (v.tolist() for v in np.nonzero(mask))
    sums = [len(rr), sum(rr), sum(cc), sum(r * r for r in rr), sum(r * c for r, c in zip(rr, cc)), sum(c * c for c in cc)]
    return _box(mask), sums + list(perimeter_classes(mask)) + [convex_area_integer(mask), 0, 0, 0]


# ---- the derived floats, exactly -------------------------------------------------------------------------------------------------------------

def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


def _atan(x):
    """atan of a Decimal: three argument halvings atan(x) = 2 atan(x / (1 + sqrt(1 + x^2))), then the series.  |x| <= 1."""
    for _ in range(3):
        x = x / (1 + (1 + x * x).sqrt())
    term, total, k, x2 = x, x, 1, x * x
    while abs(term) > Decimal(10) ** -58:
        term = -term * x2
        k += 2
        total += term / k
    return 8 * total


PI = 4 * _atan(Decimal(1))


def _atan2(y, x):
    if x == 0 and y == 0:
        return Decimal(0)
    if abs(y) <= abs(x):
        a = _atan(y / x)
        return a if x > 0 else (a + PI if y >= 0 else a - PI)
    a = _atan(x / y)
    return PI / 2 - a if y > 0 else -PI / 2 - a


def exact_floats(bbox, vals):
    """The float columns from the 13 integers by the contract's formulae, as Decimals at 60 digits (None where the contract says NaN)."""
    N, sr, sc, srr, src, scc, p1, p2, p3, hull = (int(v) for v in vals[:10])
    r2 = Decimal(2).sqrt()
    out = {"perimeter": p1 + p2 * r2 + p3 * (1 + r2) / 2, "equivalent_diameter": (4 * Decimal(N) / PI).sqrt()}
    if N == 0:
        out.update({k: None for k in FLOAT_KEYS if k not in out})
        return out
    A, C, B = N * scc - sc * sc, N * srr - sr * sr, -(N * src - sr * sc)
    a, b, c = Fraction(A, N * N), Fraction(B, N * N), Fraction(C, N * N)
    root = _dec(b * b + ((a - c) / 2) ** 2).sqrt()
    l1 = _dec((a + c) / 2) + root
    l2 = _dec(a * c - b * b) / l1 if l1 else Decimal(0)
    out.update({"centroid-0": _dec(Fraction(sr, N)), "centroid-1": _dec(Fraction(sc, N)),
                "extent": _dec(Fraction(N, (bbox[2] - bbox[0]) * (bbox[3] - bbox[1]))), "solidity": _dec(Fraction(N, hull)),
                "major_axis_length": 4 * l1.sqrt(), "minor_axis_length": 4 * l2.sqrt(), "eccentricity": (2 * root / l1).sqrt() if l1 else Decimal(0),
                "orientation": (-PI / 4 if B < 0 else PI / 4) if A == C else _atan2(_dec(-2 * b), _dec(c - a)) / 2})
    return out


def float_error(key, got, exact):
    """(error, bound): |got - exact| and 8 ulp of the exact value -- for the orientation 8 * 2^-52 absolute.  Derived, not measured: no column
    passes through more than eight correctly rounded operations after the exact integers."""
    err = abs(Decimal(got) - exact)
    if key == "orientation":
        return err, Decimal(8) * Decimal(2) ** -52
    return err, 8 * Decimal(math.ulp(float(exact)))


# ---- the test masks --------------------------------------------------------------------------------------------------------------------------

def _named():
    H, W = 40, 50
    z = lambda: np.zeros((H, W), bool)
    out = {}
    m = z(); m[17, 29] = True; out["one_pixel"] = m
    m = z(); m[9, 4:27] = True; out["row_1x23"] = m
    m = z(); m[np.arange(5, 25), np.arange(11, 31)] = True; out["diagonal_20"] = m
    m = z(); m[20:23, 30:33] = True; out["square_3x3"] = m
    out["empty"] = z()
    out["full_image"] = ~z()
    m = z(); m[5:30, 8:40] = True; m[12:20, 15:28] = False; m[24, 30] = False; out["hole"] = m
    m = z(); m[3:9, 4:12] = True; m[25:38, 30:47] = True; m[30, 20] = True; out["two_parts"] = m
    m = z(); m[0, 7] = m[H - 1, 33] = m[13, 0] = m[28, W - 1] = True; m[10:30, 10:40] = True; out["touches_all_borders"] = m
    m = z(); m[H - 3:, 5] = True; m[:2, 6] = True; out["runs_wrap_columns"] = m
    r = np.random.default_rng(474)
    for rows in (63, 64, 65, 129):                                    # a box that ends before, on and after a 64-row word, and spans three
        for r0 in (0, 5):
            h = rows + r0 + (0 if r0 == 0 else 3)
            yy, xx = np.ogrid[:h, :37]
            m = ((yy - (r0 + (rows - 1) / 2)) / (rows / 2)) ** 2 + ((xx - 18) / 14.0) ** 2 <= 1.0
            m &= r.random((h, 37)) < 0.85
            m[r0:r0 + rows, 18] = True
            assert _box(m)[0] == r0 and _box(m)[2] == r0 + rows
            out[f"rows_{rows}_at_{r0}"] = m
    return out


HAND = ("one_pixel", "row_1x23", "diagonal_20", "square_3x3")


def blob_batch():
    """200 seeded blob masks on 96 x 130, built like _batch() of tests/test_edge_distance_gpu.py: one to three ellipses each."""
    r = np.random.default_rng(20240608)
    h, w = 96, 130
    yy, xx = np.ogrid[:h, :w]

    def blob(k):
        m = np.zeros((h, w), bool)
        for _ in range(k):
            m |= ((yy - r.integers(0, h)) / r.integers(2, 40)) ** 2 + ((xx - r.integers(0, w)) / r.integers(2, 50)) ** 2 <= 1.0
        return m
    return [blob(int(r.integers(1, 4))) for _ in range(200)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (mask, bbox, [13 integers]): the named masks and the batch ('blob/000' ..), references computed once."""
    masks = dict(_named())
    masks.update({f"blob/{i:03d}": m for i, m in enumerate(blob_batch())})
    return {k: (m,) + ref_integers(m) for k, m in masks.items()}


NAMED = tuple(_named())
