"""The dense references of amp_mask_distance (tests/mask_distance_cases.py).  Two independent ones, neither looks at run lists:
  * scipy_d2: scipy.ndimage.distance_transform_edt(..., return_indices=True) on one decoded mask, padded by one zero for border_value 0; the
    squared distances are formed as integers from the indices of the nearest background pixel, never from the float distances;
  * brute_d2: every mask pixel against every background pixel (and the ring outside the image for border_value 0), for sides up to about 12.
scipy leaves a mask without background undefined; both references return NONE on every pixel there, which is the call's stated departure.
walk_d2 is a third evaluation, the Python transcription of the rule of csrc/mask_distance.h with switches that seed one defect each
(tests/test_mask_distance_ref.py shows that the references tell every defect from the rule)."""
import numpy as np
from scipy import ndimage

NONE = 0xFFFFFFFF


def scipy_d2(mask, border_value):
    """int64 [h, w]: the squared distance of every mask pixel to the nearest pixel that is not in the mask, 0 outside the mask"""
    mask = np.asarray(mask, bool)
    m = np.pad(mask, 1) if border_value == 0 else mask
    if m.all():
        return np.full(mask.shape, NONE, np.int64)
    idx = ndimage.distance_transform_edt(m, return_distances=False, return_indices=True)
    rr, cc = np.indices(m.shape)
    d2 = (idx[0].astype(np.int64) - rr) ** 2 + (idx[1].astype(np.int64) - cc) ** 2
    d2[~m] = 0
    return d2[1:-1, 1:-1] if border_value == 0 else d2


def brute_d2(mask, border_value):
    mask = np.asarray(mask, bool)
    m = np.pad(mask, 1) if border_value == 0 else mask
    bg = np.argwhere(~m)
    out = np.zeros(m.shape, np.int64)
    for r, c in np.argwhere(m):
        out[r, c] = int(((bg[:, 0] - r) ** 2 + (bg[:, 1] - c) ** 2).min()) if len(bg) else NONE
    return out[1:-1, 1:-1] if border_value == 0 else out


def walk_d2(mask, border_value, g_off_by_one=False, ignore_border=False):
    """The rule of mask_distance.h, pixel by pixel: the column distance g = min(r - s + 1, e - r) in the piece [s, e) of a column, a side at the
    image's edge not counting with border_value 1; d2 = min over the columns of dx^2 + g^2, columns -1 and w giving dx^2 with border_value 0;
    the walk outwards stops when dx^2 reaches the best value.  g_off_by_one: g = min(r - s, e - r); ignore_border: border_value taken as 1."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    border = 1 if ignore_border else border_value
    g2 = np.zeros((h, w), np.int64)                                  # g^2 of every mask pixel, NONE when no side counts
    for c in range(w):
        r = 0
        while r < h:
            if not mask[r, c]:
                r += 1
                continue
            s = r
            while r < h and mask[r, c]:
                r += 1
            e = r
            for y in range(s, e):
                sides = ([] if border and s == 0 else [y - s + (0 if g_off_by_one else 1)]) + ([] if border and e == h else [e - y])
                g2[y, c] = min(sides) ** 2 if sides else NONE
    out = np.zeros((h, w), np.int64)
    for r, c in np.argwhere(mask):
        best, dx = int(g2[r, c]), 1
        while dx * dx < best:
            if border and c - dx < 0 and c + dx >= w:
                break
            for cc in (c - dx, c + dx):
                if 0 <= cc < w:
                    cand = dx * dx + int(g2[r, cc]) if g2[r, cc] != NONE else NONE
                else:
                    cand = NONE if border else dx * dx
                best = min(best, cand)
            dx += 1
        out[r, c] = best
    return out


def box(mask):
    """the tight box [r0, c0, r1, c1] with exclusive ends, zeros for an empty mask"""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return [int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1] if len(rows) else [0, 0, 0, 0]


def outputs(mask, d2, ncurves=(), row_major_tie=False):
    """What the call returns for one mask whose squared distances are d2: {'stats': [d2_max, pos, sum_d2, area], 'box', 'map': uint32 crop,
    'curve': {ncurve: list}}.  pos = col * h + row of the first pixel in column-major order that attains d2_max; row_major_tie seeds the
    defect of taking the first in row-major order."""
    mask, d2 = np.asarray(mask, bool), np.asarray(d2, np.int64)
    h = mask.shape[0]
    b = box(mask)
    area = int(mask.sum())
    vals = d2[mask]
    if area == 0:
        stats = [0, 0, 0, 0]
    else:
        top = int(vals.max())
        rows, cols = np.nonzero(mask & (d2 == top))
        k = int(np.argmin(rows * mask.shape[1] + cols if row_major_tie else cols * h + rows))
        stats = [top, int(cols[k]) * h + int(rows[k]), int(vals[vals != NONE].sum()), area]
    ordered = np.sort(vals)                                          # the pixels with d2 > r^2: those behind the last value <= r^2
    curve = {n: (area - np.searchsorted(ordered, np.arange(n, dtype=np.int64) ** 2, side="right")).tolist() for n in ncurves}
    return {"stats": stats, "box": b, "map": d2[b[0]: b[2], b[1]: b[3]].astype(np.uint32), "curve": curve}
