"""The case set of amp_mask_intensity, shared by tests/test_mask_intensity.py (host path) and tests/test_mask_intensity_gpu.py (device path).  A
case is a pool {masks: bool [N, h, w], rles: the run lists handed to the call (the encoded masks unless the case brings looser ones), img: the
uint8 or uint16 image [h, w] or [h, w, C]}; every case is run without a histogram and at two hist_shifts of its depth.  The reference is
tests/mask_intensity_ref.py's img[mask] with exact integer sums (its scipy.ndimage twin is held to it in tests/test_mask_intensity_ref.py);
the seeded pools are those of tests/morphology_cases.py under seeded images.  The hand cases are the smallest at which the kernels can go
wrong: the edges of the 64 x 64 transpose tile, runs across column ends, the cut between two work items of CHUNK pixel ranks."""
import functools

import numpy as np

from ampis_amd import rle

import mask_intensity_ref as ref
import morphology_cases as mc

CHUNK = rle.INTENSITY_CHUNK
SHIFTS = {8: (None, 0, 7), 16: (None, 4, 15)}
KINDS = ("u8", "rgb8", "u16")
N_SEEDED = mc.N_SEEDED


def _case(masks, img, rles=None):
    masks, img = np.asarray(masks).astype(bool), np.asarray(img)
    assert masks.ndim == 3 and img.dtype in (np.uint8, np.uint16) and img.shape[:2] == masks.shape[1:]
    return {"masks": masks, "img": img, "rles": rles}


def _image(seed, h, w, dtype, channels=0):
    """seeded noise over the whole range of the dtype, every channel its own; channels 0: a grey image [h, w]"""
    rng = np.random.RandomState(7300 + seed)
    top = 256 if dtype == np.uint8 else 65536
    return rng.randint(0, top, (h, w, channels) if channels else (h, w)).astype(dtype)


def _noise(seed, n, h, w, density=0.5):
    return np.random.RandomState(7100 + seed).random_sample((n, h, w)) < density


def _at(h, w, positions):
    """the mask [h, w] of the given positions col * h + row (a slice or an index array)"""
    m = np.zeros(h * w, bool)
    m[positions] = True
    return m.reshape(w, h).T.copy()


def _first(h, w, k, start=0):
    """k pixels in column-major order from position start: one run"""
    return _at(h, w, slice(start, start + k))


def _hand():
    c = {}
    c["image_1x1"] = _case([[[False]], [[True]]], np.array([[201]], np.uint8))
    c["image_1x65"] = _case(np.stack([np.ones((1, 65), bool), (np.arange(65) % 3 != 0)[None, :]]), _image(1, 1, 65, np.uint16, 3))
    c["image_65x1"] = _case(np.stack([np.ones((65, 1), bool), (np.arange(65) % 3 != 0)[:, None]]), _image(2, 65, 1, np.uint8, 2))
    layouts = [(np.uint8, 0), (np.uint8, 3), (np.uint16, 0), (np.uint16, 2), (np.uint8, 4), (np.uint16, 4), (np.uint8, 2), (np.uint16, 3), (np.uint8, 1)]
    k = 0
    for h in (63, 64, 65):                                           # the edges of the transpose tile in each direction
        for w in (63, 64, 65):
            dtype, ch = layouts[k]
            stripes = np.zeros((h, w), bool); stripes[:, ::2] = True; stripes[-1, :] = True
            c[f"tile_{h}x{w}"] = _case(np.concatenate([np.ones((1, h, w), bool), _noise(10 + k, 1, h, w), stripes[None]]), _image(10 + k, h, w, dtype, ch))
            k += 1
    ends = np.zeros((3, 6, 5), bool)
    ends[0, 4:, 1] = True; ends[0, :2, 2] = True                     # one run that goes on across the end of column 1
    ends[1, 3:, 2] = True                                            # a run that ends exactly at a column end
    ends[2, :, 0] = True; ends[2, :, 1] = True; ends[2, 0, 2] = True # two whole columns and one pixel: one run over two column ends
    c["runs_at_column_ends"] = _case(ends, _image(30, 6, 5, np.uint8, 3))
    c["runs_at_column_ends_u16"] = _case(ends, _image(31, 6, 5, np.uint16))
    big = np.stack([np.ones((70, 70), bool), _first(70, 70, CHUNK), _first(70, 70, CHUNK + 1), _first(70, 70, 2 * CHUNK + 1),
                    _first(70, 70, CHUNK + 40, 333)])
    c["work_item_cuts_one_run"] = _case(big, _image(32, 70, 70, np.uint8))        # a run of 4900 straddles the cuts at CHUNK and 2 CHUNK
    many = _noise(33, 1, 70, 70, 0.7)[0]
    order = np.flatnonzero(many.T.reshape(-1))                       # its pixels in column-major order
    c["work_item_cuts_many_runs"] = _case(np.stack([many, _at(70, 70, order[:CHUNK]), _at(70, 70, order[:CHUNK + 3])]), _image(33, 70, 70, np.uint16, 2))
    odd = np.stack([_at(9, 7, slice(1, None, 4)) | _at(9, 7, slice(2, None, 4)),      # runs of 2 that start at positions 1, 5, 9, ...
                    _at(9, 7, slice(3, None, 6))])                                    # single pixels at odd positions
    c["runs_starting_at_odd_positions_u8"] = _case(odd, _image(34, 9, 7, np.uint8))
    c["runs_starting_at_odd_positions_u16"] = _case(odd, _image(35, 9, 7, np.uint16))
    blob = np.zeros((3, 9, 8), bool); blob[0, 1:8, 1:7] = True; blob[1, :, 2:5] = True; blob[2, 4, :] = True; blob[2, 0:6, 3] = True
    c["zero_length_runs"] = _case(blob, _image(36, 9, 8, np.uint8, 3), rles=[mc.loosen(rle.encode(np.asfortranarray(m))) for m in blob])
    three = np.zeros((3, 8, 9), bool); three[0, 1:6, 1:6] = True; three[2, 3:8, 3:9] = True
    c["an_empty_mask_between_two_others"] = _case(three, _image(37, 8, 9, np.uint16, 2))
    over2 = np.zeros((3, 9, 10), bool); over2[0, 1:7, 1:7] = True; over2[1, 3:9, 4:10] = True; over2[2, 1:7, 1:7] = True
    c["overlapping_masks"] = _case(over2, _image(38, 9, 10, np.uint8))
    some = _noise(39, 2, 11, 13)
    c["constant_0_u8"] = _case(some, np.zeros((11, 13), np.uint8))
    c["constant_0_u16"] = _case(some, np.zeros((11, 13, 2), np.uint16))
    c["constant_255"] = _case(some, np.full((11, 13, 3), 255, np.uint8))
    c["constant_65535"] = _case(some, np.full((11, 13), 65535, np.uint16))
    sq = np.zeros((1, 8, 9), bool); sq[0, 2:6, 3:7] = True
    lo_hi = np.full((8, 9), 100, np.uint8); lo_hi[2, 3] = 0; lo_hi[5, 6] = 255       # the first and the last pixel of the mask in column-major order
    c["min_on_the_first_and_max_on_the_last_pixel"] = _case(sq, lo_hi)
    hi_lo = np.full((8, 9), 30000, np.uint16); hi_lo[2, 3] = 65535; hi_lo[5, 6] = 0
    c["max_on_the_first_and_min_on_the_last_pixel"] = _case(sq, hi_lo)
    for ch in (1, 2, 3, 4):
        img = _image(40 + ch, 12, 10, np.uint8 if ch % 2 else np.uint16, ch)
        img[:, :, ch - 1] = img[:, :, ch - 1] // 2 + 7                # no two channels alike
        c[f"channels_{ch}"] = _case(_noise(40 + ch, 3, 12, 10), img)
    return c


_HAND = _hand()
HAND = tuple(_HAND)
SEEDED = tuple(f"seed_{i}_{kind}" for i in range(N_SEEDED) for kind in KINDS)


@functools.lru_cache(maxsize=None)
def get(name):
    if name in _HAND:
        return _HAND[name]
    _, i, kind = name.split("_")
    masks = mc.get(f"seed_{i}")["masks"]
    h, w = masks.shape[1:]
    return _case(masks, _image(1000 + int(i), h, w, np.uint16 if kind == "u16" else np.uint8, 3 if kind == "rgb8" else 0))


def depth(name):
    return 8 * get(name)["img"].dtype.itemsize


@functools.lru_cache(maxsize=None)
def rles(name):
    c = get(name)
    return tuple(c["rles"]) if c["rles"] is not None else tuple(rle.encode(np.asfortranarray(m)) for m in c["masks"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """{'vals': [N][C][8] Python integers, 'hist': {shift: [N][C][nbins]}} from img[mask]; computed once and shared"""
    c = get(name)
    return {"vals": [ref.index_vals(m, c["img"]) for m in c["masks"]],
            "hist": {s: [ref.index_hist(m, c["img"], s) for m in c["masks"]] for s in SHIFTS[depth(name)] if s is not None}}


def run(name, shift=None, ctx=None):
    return rle.mask_intensity(list(rles(name)), get(name)["img"], shift, ctx=ctx)


def result_bytes(res):
    vals, hist = res
    return (vals.shape, vals.tobytes(), None if hist is None else (hist.shape, hist.tobytes()))


def equal_to(res, want, shift, channels, d, where):
    vals, hist = res
    n = len(want["vals"])
    assert vals.dtype == np.uint64 and vals.shape == (n, channels, 8), where
    assert vals.tolist() == want["vals"], where
    if shift is None:
        assert hist is None, where
    else:
        assert hist.dtype == np.uint32 and hist.shape == (n, channels, 1 << (d - shift)), where
        assert hist.tolist() == want["hist"][shift], where
        assert hist.sum(axis=2).tolist() == [[v[0]] * channels for v in vals[:, 0].tolist()], where      # every pixel in one bin


def check_case(name, ctx=None):
    """one case without a histogram and at both hist_shifts of its depth against the reference; [result bytes]"""
    want, out = expected(name), []
    channels = ref.as_hwc(get(name)["img"]).shape[2]
    for shift in SHIFTS[depth(name)]:
        res = run(name, shift, ctx=ctx)
        equal_to(res, want, shift, channels, depth(name), (name, shift))
        out.append(result_bytes(res))
    return out


# ---- large sums: a 4096 x 4096 uint16 image of 65535 under one full mask, in closed form ------------------------------------------------------------

LARGE_SIDE = 4096


def large_inputs():
    n = LARGE_SIDE
    return [{"size": [n, n], "counts": np.array([0, n * n], np.uint32)}], np.full((n, n), 65535, np.uint16)


def large_expected():
    """sum v^2 = 2^24 (2^16 - 1)^2 is beyond 2^53: Python integers"""
    n, v = LARGE_SIDE, 65535
    rows = n * (n * (n - 1) // 2)                                    # the sum of the row (or column) index over all pixels
    return [[[n * n, n * n * v, n * n * v * v, rows * v, rows * v, v, v, 0]]]
