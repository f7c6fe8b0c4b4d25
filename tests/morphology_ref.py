"""The dense reference of amp_mask_morphology (tests/morphology_cases.py): scipy.ndimage.binary_dilation / binary_erosion on one decoded mask with
the structuring element built from the half heights hh(dx), and their compositions for the opening, the closing and the two bands.  Nothing
here looks at run lists; the result is encoded with rle.encode by the caller."""
import math

import numpy as np
from scipy import ndimage

OPS = ("dilate", "erode", "open", "close", "band_in", "band_out")
SHAPES = ("square", "diamond", "disk")


def half_height(shape, r, dx):
    dx = abs(int(dx))
    if shape == "square":
        return r
    if shape == "diamond":
        return r - dx
    return math.isqrt(r * r - dx * dx)


def element(shape, r):
    """bool [2 r + 1, 2 r + 1], indexed [dy + r, dx + r]"""
    fp = np.zeros((2 * r + 1, 2 * r + 1), bool)
    for dx in range(-r, r + 1):
        hh = half_height(shape, r, dx)
        fp[r - hh: r + hh + 1, dx + r] = True
    return fp


def dilate(mask, fp):
    return ndimage.binary_dilation(mask, structure=fp)


def erode(mask, fp, border_value):
    return ndimage.binary_erosion(mask, structure=fp, border_value=border_value)


def all_ops(mask, shape, r, border_value):
    """{op: bool [h, w]} of one mask"""
    mask = np.asarray(mask, bool)
    fp = element(shape, r)
    d, e = dilate(mask, fp), erode(mask, fp, border_value)
    return {"dilate": d, "erode": e, "open": dilate(e, fp), "close": erode(d, fp, border_value), "band_in": mask & ~e, "band_out": d & ~mask}


def box_and_area(mask):
    """the tight box {r0, c0, r1, c1} with exclusive ends as the run lists report it -- a run that crosses a column end covers the first and the
    last row, which the pixels of those two columns do anyway -- and the pixel count"""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    if len(rows) == 0:
        return [0, 0, 0, 0], 0
    return [int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1], int(mask.sum())
