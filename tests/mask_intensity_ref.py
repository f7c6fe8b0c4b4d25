"""The dense references of amp_mask_intensity (tests/mask_intensity_cases.py).  Two independent ones, neither looks at run lists:
  * index_vals / index_hist: img[mask] on one decoded mask, the sums formed in Python integers from uint64 products;
  * ndimage_vals / ndimage_hist: scipy.ndimage.sum / minimum / maximum / histogram over a label array (the mask as label 1).  scipy sums in
    float64, which is exact below 2^53: the function asserts that its sums stay there, so it serves every case but the one of large sums.
walk_vals is a third evaluation, the Python transcription of the rule of csrc/mask_intensity_host.hip -- the runs of ones cut at the column
ends, position p = pixel (p mod h, p div h) -- with switches that seed one defect each (tests/test_mask_intensity_ref.py shows that the
references tell every defect from the rule)."""
import numpy as np
from scipy import ndimage

NVALS = 8


def as_hwc(img):
    img = np.asarray(img)
    return img.reshape(img.shape[0], img.shape[1], -1)


def index_vals(mask, img):
    """[C][8] Python integers {N, sum v, sum v^2, sum r v, sum c v, min, max, 0} of one bool mask [h, w]; zeros for an empty mask"""
    mask, img = np.asarray(mask, bool), as_hwc(img)
    rr, cc = np.nonzero(mask)
    out = []
    for ch in range(img.shape[2]):
        v = img[:, :, ch][mask].astype(np.uint64)
        if v.size == 0:
            out.append([0] * NVALS)
            continue
        out.append([int(v.size), int(v.sum()), int((v * v).sum()), int((rr.astype(np.uint64) * v).sum()), int((cc.astype(np.uint64) * v).sum()),
                    int(v.min()), int(v.max()), 0])
    return out


def index_hist(mask, img, shift):
    """[C][nbins] counts of v >> shift over the mask's pixels"""
    mask, img = np.asarray(mask, bool), as_hwc(img)
    nbins = 1 << (8 * img.dtype.itemsize - shift)
    return [np.bincount(img[:, :, ch][mask].astype(np.int64) >> shift, minlength=nbins).tolist() for ch in range(img.shape[2])]


def ndimage_vals(mask, img):
    mask, img = np.asarray(mask, bool), as_hwc(img)
    lab = mask.astype(np.int32)
    if not mask.any():
        return [[0] * NVALS for _ in range(img.shape[2])]
    rows, cols = np.indices(mask.shape)
    out = []
    for ch in range(img.shape[2]):
        v = img[:, :, ch].astype(np.float64)
        sums = [ndimage.sum(np.ones_like(v), lab, 1), ndimage.sum(v, lab, 1), ndimage.sum(v * v, lab, 1), ndimage.sum(rows * v, lab, 1),
                ndimage.sum(cols * v, lab, 1)]
        assert all(float(s) < 2.0 ** 53 and float(s) == int(s) for s in sums), "scipy's float64 sums are exact below 2^53 only"
        out.append([int(s) for s in sums] + [int(ndimage.minimum(img[:, :, ch], lab, 1)), int(ndimage.maximum(img[:, :, ch], lab, 1)), 0])
    return out


def ndimage_hist(mask, img, shift):
    mask, img = np.asarray(mask, bool), as_hwc(img)
    depth = 8 * img.dtype.itemsize
    nbins = 1 << (depth - shift)
    if not mask.any():
        return [[0] * nbins for _ in range(img.shape[2])]
    return [np.asarray(ndimage.histogram(img[:, :, ch], 0, 1 << depth, nbins, mask.astype(np.int32), 1)).astype(np.int64).tolist()
            for ch in range(img.shape[2])]


def walk_vals(counts, img, swap_rc=False, column_end_off_by_one=False, square_in_32_bits=False):
    """The rule of the host path on a COCO run list (zeros first) of the image's size: [C][8].  swap_rc: the row taken for the column and the
    other way round; column_end_off_by_one: a column taken to end one pixel late, at (c + 1) h + 1, so the first row of the next column is
    read as row h of this one (wrapped into the image: row h - 1); square_in_32_bits: v * v formed in a signed 32-bit integer."""
    img = as_hwc(img)
    h, w, C = img.shape
    acc = [[0, 0, 0, 0, 0, None, None, 0] for _ in range(C)]
    pos = 0
    for j, run in enumerate(int(x) for x in counts):
        s, e = pos, pos + run
        pos = e
        if not j & 1:
            continue
        p = s
        while p < e:
            c = p // h
            stop = min(e, (c + 1) * h + (1 if column_end_off_by_one else 0))
            for q in range(p, stop):
                r = min(q - c * h, h - 1)
                rr, qc = (c, r) if swap_rc else (r, c)
                for ch in range(C):
                    v = int(img[min(r, h - 1), c, ch])
                    a = acc[ch]
                    vv = (((v * v + (1 << 31)) % (1 << 32)) - (1 << 31)) % (1 << 64) if square_in_32_bits else v * v      # wrapped, sign-extended
                    a[0] += 1; a[1] += v; a[2] = (a[2] + vv) % (1 << 64); a[3] += rr * v; a[4] += qc * v
                    a[5] = v if a[5] is None else min(a[5], v)
                    a[6] = v if a[6] is None else max(a[6], v)
            p = stop
    return [[0] * NVALS if a[0] == 0 else a for a in acc]
