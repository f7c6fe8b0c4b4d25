"""amp_rle_overlap_groups on the host (no GPU needed): the NULL-context path against a brute-force numpy evaluation on decoded bitmaps for every
case of tests/rle_overlap_cases.py -- every count and area exactly --, the layout of the grouped output through the raw C call, the Python
wrappers, and every refusal with its message."""
import ctypes as C

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import AmpError, lib

import rle_overlap_cases as cs


@pytest.mark.parametrize("name", cs.NAMES)
def test_host_counts_equal_the_brute_force(name):
    cs.check_case(name)


def raw_call(a_lists, b_lists, a_first, b_first, gh, gw, ngroups=None, inter_cap=None, ctx=None, null=()):
    """The C call on lists of uint32 run lists; returns (status, inter, area_a, area_b).  null: argument names passed as NULL."""
    ap, ao, al = rle._pool([np.asarray(x, np.uint32) for x in a_lists])
    bp, bo, bl = rle._pool([np.asarray(x, np.uint32) for x in b_lists])
    af, bf = np.asarray(a_first, np.int32), np.asarray(b_first, np.int32)
    gh, gw = np.asarray(gh, np.int32).reshape(-1), np.asarray(gw, np.int32).reshape(-1)
    ng = len(gh) if ngroups is None else ngroups
    total = int(sum((int(af[g + 1]) - int(af[g])) * (int(bf[g + 1]) - int(bf[g])) for g in range(max(min(ng, len(af) - 1), 0))))
    inter = np.full(max(total, 1), 0xDEADBEEF, np.uint32)
    aa, ab = np.full(max(len(a_lists), 1), 77, np.uint64), np.full(max(len(b_lists), 1), 77, np.uint64)
    args = {"apool": ap, "aoff": ao, "alen": al, "bpool": bp, "boff": bo, "blen": bl, "a_first": af, "b_first": bf, "gh": gh, "gw": gw}
    p = {k: (None if k in null else v.ctypes.data_as(C.c_void_p)) for k, v in args.items()}
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    st = lib().amp_rle_overlap_groups(ctx.handle if ctx is not None else None, p["apool"], p["aoff"], p["alen"], p["bpool"], p["boff"], p["blen"],
                                      p["a_first"], p["b_first"], p["gh"], p["gw"], ng, None if "inter" in null else vp(inter),
                                      total if inter_cap is None else inter_cap, vp(aa), vp(ab))
    return st, inter, aa, ab


def test_grouped_layout_of_the_raw_call():
    """two groups, 2 x 3 on a 2 x 3 image and 1 x 2 on a 4 x 1 image: the second block starts at 6, pairs across groups are never formed"""
    a = [[0, 6], [1, 2, 3], [1, 2, 1]]                   # full; pixels 1, 2; | rows 1, 2 of the 4 x 1 image
    b = [[0, 1, 5], [6], [2, 4], [0, 4], [2, 1, 1]]      # pixel 0; empty; pixels 2 .. 5; | full; row 2
    st, inter, aa, ab = raw_call(a, b, [0, 2, 3], [0, 3, 5], [2, 4], [3, 1])
    assert st == 0, lib().amp_last_error()
    assert inter.tolist() == [1, 0, 4, 0, 0, 1, 2, 1]
    assert aa.tolist() == [6, 2, 2] and ab.tolist() == [1, 0, 4, 4, 1]


def test_output_is_untouched_when_the_call_is_refused():
    st, inter, aa, ab = raw_call([[0, 6]], [[0, 5]], [0, 1], [0, 1], [2], [3])
    assert st != 0 and inter.tolist() == [0xDEADBEEF] and aa.tolist() == [77] and ab.tolist() == [77]


HOSTILE = [
    ("image size 0 x 3 of group 0", dict(a=[[0]], b=[[0]], af=[0, 1], bf=[0, 1], gh=[0], gw=[3])),
    ("image size 32769 x 1 of group 0", dict(a=[[32769]], b=[[32769]], af=[0, 1], bf=[0, 1], gh=[32769], gw=[1])),
    ("image size 32768 x 32769 of group 1", dict(a=[[6]], b=[[6]], af=[0, 1, 1], bf=[0, 1, 1], gh=[2, 32768], gw=[3, 32769])),
    ("mask 1 of pool A (group 1) has an empty run list", dict(a=[[6], []], b=[[6], [6]], af=[0, 1, 2], bf=[0, 1, 2], gh=[2, 2], gw=[3, 3])),
    ("the runs of mask 0 of pool B (group 0) cover 5 pixels, the image has 6", dict(a=[[6]], b=[[2, 3]], af=[0, 1], bf=[0, 1], gh=[2], gw=[3])),
    ("the runs of mask 1 of pool A (group 0) cover more than the image's 6 pixels",
     dict(a=[[6], [0xFFFFFFFF, 7]], b=[[6]], af=[0, 2], bf=[0, 1], gh=[2], gw=[3])),
    ("the runs of mask 1 of pool B (group 1) cover 6 pixels, the image has 8",          # right for group 0's image, wrong for its own
     dict(a=[[6], [8]], b=[[6], [6]], af=[0, 1, 2], bf=[0, 1, 2], gh=[2, 2], gw=[3, 4])),
    ("a_first[2] = 0 is below a_first[1] = 1", dict(a=[[6]], b=[[6]], af=[0, 1, 0], bf=[0, 1, 1], gh=[2, 2], gw=[3, 3])),
    ("b_first[1] = -1 is below b_first[0] = 0", dict(a=[[6]], b=[[6]], af=[0, 1], bf=[0, -1], gh=[2], gw=[3])),
    ("a_first[0] = 1, b_first[0] = 0 (group 0 starts at mask 0)", dict(a=[[6], [6]], b=[[6]], af=[1, 2], bf=[0, 1], gh=[2], gw=[3])),
    ("inter_cap = 1, the groups have 2 pairs", dict(a=[[6]], b=[[6], [6]], af=[0, 1], bf=[0, 2], gh=[2], gw=[3], inter_cap=1)),
    ("ngroups = -1", dict(a=[[6]], b=[[6]], af=[0, 1], bf=[0, 1], gh=[2], gw=[3], ngroups=-1)),
    ("null argument", dict(a=[[6]], b=[[6]], af=[0, 1], bf=[0, 1], gh=[2], gw=[3], null=("gw",))),
    ("null argument", dict(a=[[6]], b=[[6]], af=[0, 1], bf=[0, 1], gh=[2], gw=[3], null=("blen",))),
    ("null argument", dict(a=[[6]], b=[[6]], af=[0, 1], bf=[0, 1], gh=[2], gw=[3], null=("inter",))),
]


def check_hostile(what, kw, ctx=None):
    st, inter, aa, ab = raw_call(kw["a"], kw["b"], kw["af"], kw["bf"], kw["gh"], kw["gw"], ngroups=kw.get("ngroups"), inter_cap=kw.get("inter_cap"),
                                 ctx=ctx, null=kw.get("null", ()))
    assert st == -1 and what in lib().amp_last_error().decode(), (st, lib().amp_last_error())           # AMP_ERR_ARG
    assert set(inter.tolist()) == {0xDEADBEEF} and set(aa.tolist()) == {77} and set(ab.tolist()) == {77}


@pytest.mark.parametrize("what, kw", HOSTILE, ids=[f"{i}-{h[0][:24]}" for i, h in enumerate(HOSTILE)])
def test_hostile_arguments_are_refused_with_their_message(what, kw):
    check_hostile(what, kw)


def test_python_wrappers():
    g = cs.cases()["tile_3x67"][0]
    inters, aa, ab = rle.overlap_groups([g[0]], [g[1]])
    m = analyze.overlap_matrix(g[0], g[1], device="cpu")
    assert m.dtype == np.int64 and np.array_equal(m, g[2]) and np.array_equal(m, inters[0])
    masks = np.stack([rle.decode(r).astype(bool) for r in g[0]])
    assert np.array_equal(analyze.overlap_matrix(masks, g[1], device="cpu"), g[2])                 # anything masks_to_rle accepts
    assert analyze.overlap_matrix([], g[1], device="cpu").shape == (0, 67) and analyze.overlap_matrix(g[0], [], device="cpu").shape == (3, 0)
    assert rle.overlap_groups([], []) == ([], [], [])
    with pytest.raises(ValueError, match="device = 'tpu'"):
        analyze.overlap_matrix(g[0], g[1], device="tpu")
    with pytest.raises(ValueError, match="overlap_matrix: a / b hold masks of different sizes"):
        analyze.overlap_matrix(g[0], [cs.enc(np.ones((5, 5), bool))], device="cpu")
    with pytest.raises(ValueError, match="group 1 holds masks of different sizes"):
        rle.overlap_groups([g[0], g[0]], [g[1], [cs.enc(np.ones((5, 5), bool))]])
    with pytest.raises(AmpError, match="empty run list"):
        rle.overlap_groups([[{"size": [2, 3], "counts": np.zeros(0, np.uint32)}]], [[{"size": [2, 3], "counts": np.array([6], np.uint32)}]])


def test_device_cuda_without_a_device_is_an_error(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g = cs.cases()["tile_70x1"][0]
    with pytest.raises(AmpError, match="no HIP device"):
        analyze.overlap_matrix(g[0], g[1], device="cuda")
    assert np.array_equal(analyze.overlap_matrix(g[0], g[1], device="auto"), g[2])                  # 'auto' falls to the host
