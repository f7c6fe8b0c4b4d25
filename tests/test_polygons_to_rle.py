"""rle.polygons_to_rle / amp_polygons_to_rle on the host: every hand, seeded and micrograph case of tests/polygon_cases.py equals, byte for byte,
(a) the oracle's rleFrPoly united by the oracle's dense merge and (b) the per-polygon composition rle.merge(rle.frPyObjects(...)) it replaces;
boxes and areas are rle.bbox / rle.area of those lists; the capacity protocol, every refusal, and the callers that now make one call per image
(analyze.masks_to_rle, det_seg_scores, the Visualizer).  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import AmpError, lib
from ampis_amd.structures import PolygonMasks

import polygon_cases as pc
import seg_perf_data as D

HAND = [c[0] for c in pc.hand_cases()]
MICRO = [c[0] for c in pc.micrograph_cases()]


def check_case(name, ctx=None):
    """the call on case `name` == (a) == (b), strings, boxes and areas; returns the result"""
    h, w, insts = pc.all_cases()[name]
    got, boxes, areas = rle.polygons_to_rle(insts, h, w, ctx=ctx, return_boxes=True)
    a, b = pc.references(name)
    strings = [bytes(r["counts"]) for r in got]
    assert a == b, f"{name}: the two references disagree"
    assert strings == b, f"{name}: differs from the composition at instances {[i for i in range(len(b)) if strings[i] != b[i]][:8]}"
    assert all(r["size"] == [h, w] for r in got)
    want = [pc.box_and_area(r) for r in got]
    assert boxes.dtype == np.int32 and boxes.tolist() == [bx for bx, _ in want], name
    assert areas.dtype == np.uint32 and areas.tolist() == [ar for _, ar in want], name
    return got


@pytest.mark.parametrize("name", HAND)
def test_hand_case_equals_both_references(name):
    check_case(name)


def test_hand_cases_show_what_they_are_named_for():
    runs = lambda name, i=0: rle.string_to_counts(rle.polygons_to_rle(pc.all_cases()[name][2], *pc.all_cases()[name][:2])[i]["counts"]).tolist()
    assert runs("rect_covers_pixel_0")[0] == 0                                   # a leading run of zeros of length 0 is kept
    c = runs("rect_reaches_last_pixel")
    assert len(c) % 2 == 0 and sum(c) == 64                                      # the list ends with a run of ones: a toggle at h * w
    assert runs("entirely_outside") == [37 * 53] and runs("entirely_outside", 1) == [37 * 53]
    assert len(runs("zigzag")) == 19571
    assert runs("same_polygon_twice") == runs("same_polygon_three_times")       # a union, not a parity, across polygons
    assert len(pc.all_cases()["seventy_polygons"][2][0]) == 70 and len(pc.all_cases()["many_instances"][2]) == 5000
    for side in ("left", "right", "top", "bottom", "all"):
        assert rle.area(rle.polygons_to_rle(pc.all_cases()["overhang_" + side][2], 37, 53)[0]) > 0


def test_seeded_cases_equal_both_references():
    empty = first = 0
    for i in range(pc.SEEDS):
        got = check_case(f"seed_{i}")
        c = rle.string_to_counts(got[0]["counts"])
        empty += len(c) == 1
        first += c[0] == 0
    assert empty < pc.SEEDS // 4 and first > pc.SEEDS // 10, (empty, first)      # the generator does produce masks, and masks that start at pixel 0


def test_seeded_cases_in_one_call_equal_the_calls_one_by_one():
    for size in pc.SEED_SIZES:
        names = [f"seed_{i}" for i in range(pc.SEEDS) if pc.SEED_SIZES[i % len(pc.SEED_SIZES)] == size]
        insts = [pc.all_cases()[n][2][0] for n in names]
        got = rle.polygons_to_rle(insts, *size)
        assert [bytes(r["counts"]) for r in got] == [pc.references(n)[1][0] for n in names]


@pytest.mark.parametrize("name", MICRO)
def test_micrograph_equals_both_references(name):
    got = check_case(name)
    assert len(got) in (219, 351)


def _call(xy, poff, first, n, h, w, cap, ctx=None, null=()):
    """amp_polygons_to_rle with raw arrays; null: argument names to pass as NULL.  -> (status, outputs dict)"""
    arrs = {"xy": np.ascontiguousarray(xy, np.float64), "poly_off": np.ascontiguousarray(poff, np.uint64), "inst_first": np.ascontiguousarray(first, np.int32),
            "counts": np.full(max(cap, 1) + 8, 0xDEADBEEF, np.uint32), "counts_off": np.full(max(n, 1), 77, np.uint64),
            "counts_len": np.full(max(n, 1), -5, np.int32), "boxes": np.full((max(n, 1), 4), -5, np.int32), "areas": np.full(max(n, 1), 99, np.uint32),
            "need": np.full(1, 12345, np.uint64)}
    p = {k: (None if k in null else v.ctypes.data_as(C.c_void_p)) for k, v in arrs.items()}
    st = lib().amp_polygons_to_rle(ctx.handle if ctx is not None else None, p["xy"], p["poly_off"], p["inst_first"], n, h, w, p["counts"], cap,
                                   p["counts_off"], p["counts_len"], p["boxes"], p["areas"], p["need"])
    return st, arrs


def _error():
    return lib().amp_last_error().decode()


def capacity_protocol(ctx=None):
    h, w, insts = pc.all_cases()["nested_overlapping_disjoint"]
    flat = [p for inst in insts for p in inst]
    xy, poff = np.concatenate(flat), np.concatenate([[0], np.cumsum([len(p) for p in flat])])
    first = np.concatenate([[0], np.cumsum([len(i) for i in insts])])
    n = len(insts)
    want = [rle.string_to_counts(c) for c in pc.references("nested_overlapping_disjoint")[1]]
    total = sum(len(c) for c in want)
    st, a = _call(xy, poff, first, n, h, w, total - 1, ctx)
    assert st == -3 and int(a["need"][0]) == total and "counts_cap" in _error()                  # AMP_ERR_NOMEM, the need, and nothing else written
    assert (a["counts"] == 0xDEADBEEF).all() and (a["counts_off"] == 77).all() and (a["counts_len"] == -5).all()
    assert (a["boxes"] == -5).all() and (a["areas"] == 99).all()
    st, a = _call(xy, poff, first, n, h, w, total, ctx)
    assert st == 0 and int(a["need"][0]) == total
    assert a["counts"][:total].tolist() == np.concatenate(want).tolist()
    assert (a["counts"][total:] == 0xDEADBEEF).all()                                              # the words behind the result are untouched
    assert a["counts_len"].tolist() == [len(c) for c in want] and a["counts_off"].tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want])[:-1]]).tolist()
    st, a = _call(xy, poff, first, 0, h, w, 0, ctx)                                               # no instance: nothing needed, nothing written
    assert st == 0 and int(a["need"][0]) == 0 and (a["counts"] == 0xDEADBEEF).all()
    # instances that do not start at polygon 0 of the pool
    st, a = _call(xy, poff, first[1:], n - 1, h, w, total, ctx)
    assert st == 0 and a["counts"][: int(a["need"][0])].tolist() == np.concatenate(want[1:]).tolist()


def test_capacity_protocol_on_the_host():
    capacity_protocol()


SQ = [1.0, 1, 8, 1, 8, 8, 1, 8]
REFUSALS = [
    ("n = -1", dict(n=-1)),
    ("image size 0 x 10", dict(h=0)),
    ("image size 10 x 0", dict(w=0)),
    ("image size 32768 x 32769", dict(h=32768, w=32769)),
    ("null argument need", dict(null="need")),
    ("null argument xy", dict(null="xy")),
    ("null argument poly_off", dict(null="poly_off")),
    ("null argument inst_first", dict(null="inst_first")),
    ("null argument counts", dict(null="counts")),
    ("null argument counts_off", dict(null="counts_off")),
    ("null argument counts_len", dict(null="counts_len")),
    ("null argument boxes", dict(null="boxes")),
    ("null argument areas", dict(null="areas")),
    ("poly_off[2] = 4 is below poly_off[1] = 8", dict(poff=[0, 8, 4])),
    ("polygon 1 has 7 coordinates", dict(xy=SQ + SQ[:7], poff=[0, 8, 15])),
    ("polygon 0 has 0 coordinates", dict(poff=[0, 0, 8])),
    ("instance 1 has no polygon", dict(first=[0, 1, 1, 2], n=3)),
    ("instance 0 has no polygon", dict(first=[1, 0, 2])),
    ("inst_first[0] = -1", dict(first=[-1, 1, 2])),
    ("coordinate xy[3] = nan", dict(xy=SQ[:3] + [float("nan")] + SQ[4:] + SQ)),
    ("coordinate xy[9] = inf", dict(xy=SQ + SQ[:1] + [float("inf")] + SQ[2:])),
    ("coordinate xy[0] = -1e+06", dict(xy=[-1000000.5] + SQ[1:] + SQ)),
    ("coordinate xy[15] = 1e+06", dict(xy=SQ + SQ[:7] + [1000001.0])),
]


def refusal(what, kw, ctx=None):
    kw = dict(kw)
    null = (kw.pop("null"),) if "null" in kw else ()
    args = dict(xy=SQ + SQ, poff=[0, 8, 16], first=[0, 1, 2], n=2, h=10, w=10)
    args.update(kw)
    st, a = _call(args["xy"], args["poff"], args["first"], args["n"], args["h"], args["w"], 64, ctx, null)
    assert st == -1 and what in _error(), (st, _error())                                          # AMP_ERR_ARG naming the offender
    assert (a["counts"] == 0xDEADBEEF).all() and (a["counts_off"] == 77).all() and (a["counts_len"] == -5).all()
    assert (a["boxes"] == -5).all() and (a["areas"] == 99).all() and int(a["need"][0]) == 12345   # nothing written


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_arguments_are_refused_with_their_message(what, kw):
    refusal(what, kw)


def test_a_coordinate_at_the_limit_is_taken_and_the_wrapper_raises_beyond_it():
    big = [[[-1.0e6, -1.0e6, 1.0e6, -1.0e6, 1.0e6, 1.0e6, -1.0e6, 1.0e6]]]
    got = rle.polygons_to_rle(big, 6, 7)
    assert [bytes(r["counts"]) for r in got] == pc.ref_composition(big, 6, 7) and rle.area(got[0]) == 42
    with pytest.raises(AmpError, match="coordinate xy"):
        rle.polygons_to_rle([[[0, 0, 5, 0, 2.0e6, 5]]], 6, 7)
    assert rle.polygons_to_rle([], 6, 7) == []


def test_masks_to_rle_and_det_seg_scores_on_polygon_ground_truth():
    for fn in D.file_names():
        polys, _, size = D.gt_polygons(fn)
        got = analyze.masks_to_rle(PolygonMasks(polys), size, device="cpu")
        assert [bytes(r["counts"]) for r in got] == pc.references(fn)[1] and all(r["size"] == list(size) for r in got)
        pred, _ = D.pred_rles(fn)
        composed = [{"size": list(size), "counts": c} for c in pc.references(fn)[1]]
        s1 = analyze.det_seg_scores(PolygonMasks(polys), pred, size=size, device="cpu")
        s2 = analyze.det_seg_scores(composed, pred)
        assert s1.keys() == s2.keys()
        for k in s1:
            assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k])), k
        m1 = analyze.rle_instance_matcher(PolygonMasks(polys), pred, size=size, device="cpu")
        m2 = analyze.rle_instance_matcher(composed, pred)
        assert all(np.array_equal(m1[k], m2[k]) for k in m2)
    with pytest.raises(ValueError, match="device = 'tpu'"):
        analyze.masks_to_rle(PolygonMasks([[SQ]]), (10, 10), device="tpu")


def test_the_visualizer_draws_polygons_like_the_composition_run_lists():
    from ampis_amd.utils.visualizer import Visualizer
    h, w = 37, 53
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    insts = [pc.all_cases()[f"seed_{i}"][2][0] for i in range(0, 60, 6)]                          # the 37 x 53 seeds
    composed = [{"size": [h, w], "counts": pc.references(f"seed_{i}")[1][0]} for i in range(0, 60, 6)]
    colors = [tuple(c) for c in rng.uniform(0, 1, size=(len(insts), 3))]
    dense = rle.decode(composed[3]).astype(bool)
    mixed_a = [[p.tolist() for p in inst] for inst in insts]
    mixed_a[3], mixed_a[5] = dense, composed[5]                                                   # other kinds of item stay where they are
    mixed_b = list(composed)
    mixed_b[3] = dense
    outs = []
    for masks in ([[p.tolist() for p in inst] for inst in insts], composed, mixed_a, mixed_b):
        v = Visualizer(img.copy())
        v.render_device = "cpu"
        assert [bytes(r["counts"]) for r in v._rle_list(masks)] == [bytes(r["counts"]) for r in composed]
        outs.append(v.overlay_instances(masks=masks, assigned_colors=colors).get_image())
    assert all(np.array_equal(outs[0], o) for o in outs[1:]) and not np.array_equal(outs[0], img)
