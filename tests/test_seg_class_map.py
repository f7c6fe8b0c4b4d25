"""amp_seg_class_map on the host (no GPU needed): the NULL-context path against the dense NumPy reference (tests/seg_class_ref.py) for every
case of tests/seg_class_cases.py in both modes -- every count byte for byte, every pixel count integer for integer --, the layout of the
output through the raw C call, and every refusal with its message and untouched output buffers."""
import ctypes as C

import numpy as np
import pytest

from ampis_amd import rle
from ampis_amd._lib import lib

import seg_class_cases as cs


@pytest.mark.parametrize("mode", cs.MODES)
@pytest.mark.parametrize("name", cs.HAND)
def test_host_equals_the_dense_reference(name, mode):
    cs.check_case(name, mode)


def test_the_8x8_case_holds_every_code():
    _, pixels, code = cs.expected("all_codes_8x8", "all")
    assert sorted(np.unique(code).tolist()) == list(range(8)) and (pixels > 0).all()
    counts, px = cs.check_case("all_codes_8x8", "all")
    assert (px > 0).all() and all(len(c) >= 2 for c in counts)


def test_the_first_count_is_the_zero_run():
    counts, _ = cs.check_case("first_pixel", "reduced")
    assert counts[0][0] == 0 and counts[1][0] > 0                    # the TP class owns pixel 0
    counts, _ = cs.check_case("last_pixel", "reduced")
    assert len(counts[0]) % 2 == 0                                   # the TP class owns the last pixel: the list ends with a run of ones
    counts, px = cs.check_case("no_pairs", "all")
    assert [c.tolist() for c in counts] == [[cs.H * cs.W]] * 7 and px.tolist() == [cs.H * cs.W] + [0] * 7


@pytest.mark.parametrize("chunk", range(8))
def test_host_equals_the_dense_reference_on_seeded_cases(chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        for mode in cs.MODES:
            cs.check_case(f"seed_{i}", mode)


def test_seeded_cases_cover_what_they_should():
    sizes = [cs.seeded_case(i)["size"] for i in range(cs.N_SEEDED)]
    assert max(h for h, _ in sizes) <= 96 and max(w for _, w in sizes) <= 96 and any(h > 64 for h, _ in sizes) and any(h == 64 for h, _ in sizes)
    pairs = [cs.seeded_case(i)["pairs"] for i in range(cs.N_SEEDED)]
    assert any(len(p) == 0 for p in pairs) and any(len(set(p)) < len(p) for p in pairs)
    seen = np.zeros(8, bool)
    for i in range(cs.N_SEEDED):
        seen |= cs.expected(f"seed_{i}", "all")[1] > 0
    assert seen.all()


def check_full_image_at_the_size_limit(ctx=None):
    """32768 x 32768 = 2^30 pixels, never decoded: the full image against the full image without its first and its last pixel.  Positions up to
    2^30, 2^24 plane words a plane, every column a full run of 512 words."""
    n = 32768
    g = {"size": [n, n], "counts": np.array([0, n * n], np.uint32)}
    q = {"size": [n, n], "counts": np.array([1, n * n - 2, 1], np.uint32)}
    counts, pixels = rle.seg_class_map([g], [q], [(0, 0)], "reduced", ctx=ctx)
    assert [c.tolist() for c in counts] == [[1, n * n - 2, 1], [0, 1, n * n - 2, 1], [n * n], [n * n]]
    assert pixels.tolist() == [0, n * n - 2, 2, 0, 0, 0, 0, 0]


def test_host_full_image_at_the_size_limit():
    check_full_image_at_the_size_limit()


def raw_call(g_lists, p_lists, pairs, h, w, mode=0, cap=None, ctx=None, ng=None, npred=None, n=None, null=()):
    """The C call on lists of uint32 run lists; returns (status, counts, counts_off, pixels) with the buffers pre-filled with marks."""
    gp, go, gl = rle._pool([np.asarray(x, np.uint32) for x in g_lists])
    pp, po, pl = rle._pool([np.asarray(x, np.uint32) for x in p_lists])
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    pg, pq = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    counts = np.full(64 if cap is None else max(cap, 1), 0xDEADBEEF, np.uint32)
    coff, pixels = np.full(8, 77, np.uint64), np.full(8, 77, np.uint64)
    args = {"gpool": gp, "goff": go, "glen": gl, "ppool": pp, "poff": po, "plen": pl, "pair_g": pg, "pair_p": pq, "counts": counts,
            "counts_off": coff, "pixels": pixels}
    a = {k: (None if k in null else v.ctypes.data_as(C.c_void_p)) for k, v in args.items()}
    st = lib().amp_seg_class_map(ctx.handle if ctx is not None else None, a["gpool"], a["goff"], a["glen"], len(g_lists) if ng is None else ng,
                                 a["ppool"], a["poff"], a["plen"], len(p_lists) if npred is None else npred, a["pair_g"], a["pair_p"],
                                 len(pairs) if n is None else n, h, w, mode, a["counts"], len(counts) if cap is None else cap, a["counts_off"],
                                 a["pixels"])
    return st, counts, coff, pixels


def test_layout_of_the_raw_call():
    """2 x 3 image, pixels 0 .. 5 column-major.  g = pixels 0 .. 3, q = pixels 2 .. 4: FN 0, 1; TP 2, 3; FP 4; background 5"""
    st, counts, coff, pixels = raw_call([[0, 4, 2]], [[2, 3, 1]], [(0, 0)], 2, 3, mode=0)
    assert st == 0, lib().amp_last_error()
    assert coff[:5].tolist() == [0, 3, 6, 9, 10]
    assert counts[:10].tolist() == [2, 2, 2] + [0, 2, 4] + [4, 1, 1] + [6]
    assert pixels.tolist() == [1, 2, 2, 0, 1, 0, 0, 0]
    assert set(counts[10:].tolist()) == {0xDEADBEEF} and coff[5:].tolist() == [77] * 3
    st, counts, coff, pixels = raw_call([[0, 4, 2]], [[2, 3, 1]], [(0, 0)], 2, 3, mode=1)
    assert st == 0 and coff.tolist() == [0, 3, 6, 7, 10, 11, 12, 13]
    assert counts[:13].tolist() == [2, 2, 2] + [0, 2, 4] + [6] + [4, 1, 1] + [6] * 3
    # masks that no pair names are never read: a malformed one and an empty list pass
    st, counts, coff, pixels = raw_call([[0, 4, 2], [1, 2]], [[], [2, 3, 1]], [(0, 1)], 2, 3, mode=0)
    assert st == 0 and counts[:10].tolist() == [2, 2, 2] + [0, 2, 4] + [4, 1, 1] + [6]


# (status, part of the message, arguments).  -1 = AMP_ERR_ARG, -3 = AMP_ERR_NOMEM
HOSTILE = [
    (-1, "the runs of ground-truth mask 0 (pair 0) cover 5 pixels, the image has 6", dict(g=[[2, 3]], p=[[6]], pairs=[(0, 0)])),
    (-1, "the runs of predicted mask 1 (pair 1) cover more than the image's 6 pixels",
     dict(g=[[6]], p=[[6], [0xFFFFFFFF, 7]], pairs=[(0, 0), (0, 1)])),
    (-1, "pair 1 names predicted mask 0, which has an empty run list", dict(g=[[6], [6]], p=[[], [6]], pairs=[(0, 1), (1, 0)])),
    (-1, "pair 0 names ground-truth mask 0, which has an empty run list", dict(g=[[]], p=[[6]], pairs=[(0, 0)])),
    (-1, "pair 1 = (1, 0) outside 1 x 1 masks", dict(g=[[6]], p=[[6]], pairs=[(0, 0), (1, 0)])),
    (-1, "pair 0 = (0, -1) outside 1 x 1 masks", dict(g=[[6]], p=[[6]], pairs=[(0, -1)])),
    (-1, "image size 0 x 3", dict(g=[[6]], p=[[6]], pairs=[(0, 0)], h=0)),
    (-1, "image size 32769 x 1", dict(g=[[32769]], p=[[32769]], pairs=[(0, 0)], h=32769, w=1)),
    (-1, "image size 32768 x 32769", dict(g=[[6]], p=[[6]], pairs=[], h=32768, w=32769)),
    (-1, "mode = 2", dict(g=[[6]], p=[[6]], pairs=[(0, 0)], mode=2)),
    (-1, "n = -1", dict(g=[[6]], p=[[6]], pairs=[], n=-1)),
    (-1, "null argument", dict(g=[[6]], p=[[6]], pairs=[(0, 0)], null=("plen",))),
    (-1, "null argument", dict(g=[[6]], p=[[6]], pairs=[(0, 0)], null=("pixels",))),
    (-3, "counts_cap = 19, 20 are needed", dict(g=[[1, 2, 3]], p=[[0, 2, 4]], pairs=[(0, 0)], cap=19)),       # 4 x (1 + 2 + 2)
    (-3, "counts_cap = 6, 7 are needed", dict(g=[[6]], p=[[6]], pairs=[], mode=1, cap=6)),
]


def test_the_limit_is_two_to_the_thirty_pixels():
    """32768 x 32768 = 2^30 pixels is inside the limits: the call gets as far as the runs, which cover 6 pixels"""
    st, counts, coff, pixels = raw_call([[6]], [[6]], [(0, 0)], 32768, 32768)
    assert st == -1 and "cover 6 pixels, the image has 1073741824" in lib().amp_last_error().decode()


def check_hostile(status, what, kw, ctx=None):
    st, counts, coff, pixels = raw_call(kw["g"], kw["p"], kw["pairs"], kw.get("h", 2), kw.get("w", 3), mode=kw.get("mode", 0), cap=kw.get("cap"),
                                        ctx=ctx, n=kw.get("n"), null=kw.get("null", ()))
    assert st == status and what in lib().amp_last_error().decode(), (st, lib().amp_last_error())
    assert set(counts.tolist()) == {0xDEADBEEF} and set(coff.tolist()) == {77} and set(pixels.tolist()) == {77}


@pytest.mark.parametrize("status, what, kw", HOSTILE, ids=[f"{i}-{h[1][:24]}" for i, h in enumerate(HOSTILE)])
def test_hostile_arguments_are_refused_with_their_message(status, what, kw):
    check_hostile(status, what, kw)


def test_python_wrapper():
    c = cs.get("two_gt_one_pred")
    counts, pixels = rle.seg_class_map(c["gt"], c["pred"], c["pairs"], "all")
    again, _ = rle.seg_class_map(c["gt"], c["pred"], np.asarray(c["pairs"]), 1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(counts, again))
    assert pixels[5] > 0                                             # TP of one pair, FP of the other
    with pytest.raises(ValueError, match="mode = 'some'"):
        rle.seg_class_map(c["gt"], c["pred"], c["pairs"], "some")
    with pytest.raises(AssertionError, match="size="):
        rle.seg_class_map(c["gt"], c["pred"], [], "all")
