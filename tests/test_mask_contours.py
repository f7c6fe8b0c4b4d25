"""amp_mask_contours on the host (no GPU needed): the NULL-context path against the dense edge walk of tests/contours_ref.py on every case of
tests/contours_cases.py at both connectivities, ring for ring, with the identities of the definition (areas, mask_topology's parts and holes,
the crack perimeter); the exact way back through polygons_to_rle -- the parity of all rings is the mask, the union of the outer rings the
hole-filled mask --; the capacity protocol and every refusal through the raw C call with sentinel words behind the buffers; the Python surface:
rle.mask_contours, analyze.mask_contours, analyze.masks_to_polygons."""
import ctypes as C

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import lib
from ampis_amd.structures import PolygonMasks

import contours_cases as cs


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("name", cs.HAND)
def test_host_equals_the_reference(name, connectivity):
    cs.check_case(name, connectivity)


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("chunk", range(8))
def test_host_equals_the_reference_on_seeded_cases(chunk, connectivity):
    for name in cs.SEEDED[chunk * 25: chunk * 25 + 25]:
        cs.check_case(name, connectivity)


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("name", cs.LARGEST)
def test_the_largest_sides(name, connectivity):
    res = cs.check_case(name, connectivity)
    if name == cs.LARGEST[2]:                                        # positions up to 2^30: the last pixel of the image is a ring of its own
        assert res[5][-4:].tolist() == [[32767, 32767], [32768, 32767], [32768, 32768], [32767, 32768]]


def _ring_count(name, connectivity, i=0):
    return len(cs.expected(name, connectivity)[i])


def test_the_cases_are_what_their_names_say():
    full = cs.expected("full", 2)[0]
    assert len(full) == 1 and full[0]["xy"].tolist() == [[0, 0], [6, 0], [6, 5], [0, 5]] and full[0]["area2"] == 60 and full[0]["length"] == 22
    assert cs.expected("empty", 1) == [[]]
    assert [_ring_count("two_diagonal_pixels", 2, i) for i in range(3)] == [1, 1, 1]
    assert [_ring_count("two_diagonal_pixels", 1, i) for i in range(3)] == [2, 2, 2]
    assert all(len(r["xy"]) == 8 for m in cs.expected("two_diagonal_pixels", 2) for r in m)
    assert all(len(r["xy"]) == 4 for m in cs.expected("two_diagonal_pixels", 1) for r in m)
    assert _ring_count("checkerboard_7x7", 1) == 25 and _ring_count("checkerboard_7x7", 2) == 13      # all saddles: 25 pixels, or one part with 12 holes
    assert sum(r["area2"] < 0 for r in cs.expected("checkerboard_7x7", 2)[0]) == 12
    assert [r["area2"] < 0 for r in cs.expected("frame_with_hole", 2)[0]] == [False, True]
    assert [r["area2"] for r in cs.expected("hole_with_island", 2)[0]] == [162, -50, 2]
    for k, holes in ((2, 1), (1, 0)):                                # the hole that meets the outside at a corner is one at connectivity 2 only
        for i in range(2):
            assert sum(r["area2"] < 0 for r in cs.expected("hole_touching_outside_diagonally", k)[i]) == holes
    assert _ring_count("spiral_33", 2) == 1 and len(cs.expected("spiral_33", 2)[0][0]["xy"]) > 60
    for t in (127, 128, 129, 257):                                   # one ring; its nodes straddle the powers of two of the jumping rounds
        (ring,) = cs.expected(f"comb_{t}", 2)[0]
        assert len(ring["xy"]) == 4 * t
    c_hole = cs.get("c_shaped_hole")["masks"][0]
    assert (np.diff(c_hole[:, 2].astype(int)) != 0).sum() == 4 and sum(r["area2"] < 0 for r in cs.expected("c_shaped_hole", 2)[0]) == 1
    assert len(cs.get("pool_of_0")["masks"]) == 0 and len(cs.get("pool_of_65")["masks"]) == 65
    assert [len(r["counts"]) for r in cs.rles("zero_length_runs")] == [11, 6, 6]
    sizes = [cs.get(s)["masks"].shape for s in cs.SEEDED]
    assert max(s[1] for s in sizes) == 40 and max(s[2] for s in sizes) == 40 and {s[0] for s in sizes} == set(range(1, 7))
    assert sum(r["area2"] < 0 for s in cs.SEEDED for m in cs.expected(s, 2) for r in m) > 500


def _dense(rles):
    return np.stack([rle.decode(r).astype(bool) for r in rles]) if rles else np.zeros((0, 1, 1), bool)


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("chunk", range(4))
def test_the_parity_of_all_rings_is_the_mask(chunk, connectivity):
    """every ring through polygons_to_rle as an instance of one polygon; the XOR of the decoded rings is the mask, holes and islands included"""
    for name in cs.SEEDED[chunk * 50: chunk * 50 + 50]:
        masks, (h, w) = cs.get(name)["masks"], cs.size(name)
        first, off, ln, _, _, xy = cs.run(name, connectivity)
        rings = [[xy[off[r]: off[r] + ln[r]].astype(np.float64).reshape(-1)] for r in range(len(off))]
        dense = _dense(rle.polygons_to_rle(rings, h, w)) if rings else np.zeros((0, h, w), bool)
        for i in range(len(masks)):
            got = np.zeros((h, w), bool)
            for r in range(first[i], first[i + 1]):
                got ^= dense[r]
            assert (got == masks[i]).all(), (name, connectivity, i)


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("chunk", range(4))
def test_the_union_of_the_outer_rings_is_the_hole_filled_mask(chunk, connectivity):
    for name in cs.SEEDED[chunk * 50: chunk * 50 + 50]:
        size = cs.size(name)
        polys, has_holes = analyze.masks_to_polygons(cs.rles(name), connectivity, device="cpu", return_has_holes=True)
        filled = analyze.clean_masks(cs.rles(name), area_threshold=None, connectivity=connectivity, device="cpu")
        back = analyze.masks_to_rle(PolygonMasks(polys), size, device="cpu")
        assert [r["counts"] for r in back] == [r["counts"] for r in filled], (name, connectivity)
        topo = analyze.mask_topology(cs.rles(name), connectivity, device="cpu")
        assert has_holes.tolist() == (topo["n_holes"] > 0).tolist() and [len(p) for p in polys] == topo["n_parts"].tolist(), (name, connectivity)


SENTINEL = 0x5EA1ED
GUARD = 8
OUTPUTS = ("ring_first", "ring_off", "ring_len", "ring_area2", "ring_length", "xy", "need")


def raw_call(counts_list, h, w, connectivity=2, ring_cap=16, xy_cap=64, ctx=None, null=(), n=None):
    """The C call with marked buffers and GUARD sentinel words behind each: (status, dict of buffers)."""
    pool, off, ln = rle._pool([np.asarray(c, np.uint32) for c in counts_list])
    nn = len(counts_list) if n is None else n
    k = max(nn, 0)
    buf = {"ring_first": np.full(k + 1 + GUARD, SENTINEL, np.uint64), "ring_off": np.full(ring_cap + GUARD, SENTINEL, np.uint64),
           "ring_len": np.full(ring_cap + GUARD, SENTINEL, np.int32), "ring_area2": np.full(ring_cap + GUARD, SENTINEL, np.int64),
           "ring_length": np.full(ring_cap + GUARD, SENTINEL, np.int64), "xy": np.full(2 * xy_cap + GUARD, SENTINEL, np.int32),
           "need": np.full(2 + GUARD, SENTINEL, np.uint64), "pool": pool, "off": off, "len": ln}
    a = {key: (None if key in null else v.ctypes.data_as(C.c_void_p)) for key, v in buf.items()}
    st = lib().amp_mask_contours(ctx.handle if ctx is not None else None, a["pool"], a["off"], a["len"], nn, h, w, connectivity, a["ring_first"],
                                 a["ring_off"], a["ring_len"], a["ring_area2"], a["ring_length"], ring_cap, a["xy"], xy_cap, a["need"])
    return st, buf


def untouched(buf, but=()):
    return all(set(v.tolist()) == {SENTINEL} for k, v in buf.items() if k in OUTPUTS and k not in but)


def check_capacity_protocol(ctx=None, name="seed_7", connectivity=2):
    lists, (h, w) = [r["counts"] for r in cs.rles(name)], cs.size(name)
    want = [r for m in cs.expected(name, connectivity) for r in m]
    n, rings, vertices = len(lists), len(want), sum(len(r["xy"]) for r in want)
    assert rings > 1 and vertices > 8
    message = f"{vertices} vertices in {rings} rings are needed"
    for rcap, vcap in ((0, 0), (rings - 1, vertices), (rings, vertices - 1)):            # either one short: refused, nothing but the need written
        st, buf = raw_call(lists, h, w, connectivity, rcap, vcap, ctx=ctx)
        assert st == -3 and f"xy_cap = {vcap}, ring_cap = {rcap}; {message}" in lib().amp_last_error().decode(), (rcap, vcap)
        assert buf["need"][:2].tolist() == [vertices, rings] and set(buf["need"][2:].tolist()) == {SENTINEL} and untouched(buf, but=("need",))
    st, ok = raw_call(lists, h, w, connectivity, rings, vertices, ctx=ctx)               # exactly the need
    assert st == 0, lib().amp_last_error()
    assert ok["need"][:2].tolist() == [vertices, rings]
    assert ok["xy"][:2 * vertices].tobytes() == np.concatenate([r["xy"] for r in want]).astype(np.int32).tobytes()
    assert ok["ring_len"][:rings].tolist() == [len(r["xy"]) for r in want] and ok["ring_area2"][:rings].tolist() == [r["area2"] for r in want]
    assert ok["ring_length"][:rings].tolist() == [r["length"] for r in want]
    assert ok["ring_off"][:rings].tolist() == np.cumsum([0] + [len(r["xy"]) for r in want[:-1]]).tolist()
    assert ok["ring_first"][:n + 1].tolist() == np.cumsum([0] + [len(m) for m in cs.expected(name, connectivity)]).tolist()
    for k, used in (("ring_first", n + 1), ("ring_off", rings), ("ring_len", rings), ("ring_area2", rings), ("ring_length", rings),
                    ("xy", 2 * vertices), ("need", 2)):
        assert set(ok[k][used:].tolist()) == {SENTINEL}, k          # nothing behind the result
    return ok


def test_capacity_protocol_on_the_host():
    check_capacity_protocol()
    check_capacity_protocol(name="checkerboard_7x7", connectivity=1)


def test_the_stated_capacity_always_suffices():
    """four vertices and two rings per piece, pieces <= runs of ones + columns.  check_case asserts it on every case; here how close
    the cases come -- a checkerboard column needs all four vertices of every piece -- and a call with exactly the stated capacity."""
    worst = 0.0
    for name in cs.HAND + cs.SEEDED:
        for k in cs.CONNECTIVITIES:
            got = sum(len(r["xy"]) for m in cs.expected(name, k) for r in m)
            bound = cs.capacity_bound(name)[0]
            assert got <= bound, name
            worst = max(worst, got / bound) if bound else worst
    assert 0.5 < worst <= 1.0
    name = "mask_66x3"
    vcap, rcap = cs.capacity_bound(name)
    st, buf = raw_call([r["counts"] for r in cs.rles(name)], 66, 3, 1, rcap, vcap)
    assert st == 0 and int(buf["need"][0]) <= vcap and int(buf["need"][1]) <= rcap


# (part of the message, arguments): all AMP_ERR_ARG
GOOD = [[2, 3, 1]]                                                   # a 2 x 3 image
REFUSALS = [
    ("n = -1", dict(n=-1)),
    ("image size 0 x 3", dict(h=0, w=3)),
    ("image size 2 x -7", dict(h=2, w=-7)),
    ("image size 32769 x 2", dict(h=32769, w=2)),
    ("image size 1 x 32769", dict(h=1, w=32769)),
    ("image size 32768 x 32769", dict(h=32768, w=32769)),
    ("connectivity = 0", dict(connectivity=0)),
    ("connectivity = 3", dict(connectivity=3)),
    ("null argument pool", dict(null=("pool",))),
    ("null argument off", dict(null=("off",))),
    ("null argument len", dict(null=("len",))),
    ("null argument ring_first", dict(null=("ring_first",))),
    ("null argument ring_first", dict(null=("ring_first",), counts_list=[], n=0)),
    ("null argument ring_off", dict(null=("ring_off",))),
    ("null argument ring_len", dict(null=("ring_len",))),
    ("null argument ring_area2", dict(null=("ring_area2",))),
    ("null argument ring_length", dict(null=("ring_length",))),
    ("null argument xy", dict(null=("xy",))),
    ("null argument need", dict(null=("need",))),
    ("mask 0 has an empty run list", dict(counts_list=[[]])),
    ("the runs of mask 1 cover more than the image's 6 pixels", dict(counts_list=[[6], [2, 3, 2]])),
    ("the runs of mask 1 cover 5 pixels, the image has 6", dict(counts_list=[[0, 6], [2, 3]])),
    ("the runs of mask 0 cover 6 pixels, the image has 8", dict(h=2, w=4)),      # a run list of another image size
]


def check_refusal(what, kw, ctx=None):
    kw = dict(kw)
    st, buf = raw_call(kw.pop("counts_list", GOOD), kw.pop("h", 2), kw.pop("w", 3), ctx=ctx, **kw)
    msg = lib().amp_last_error().decode()
    assert st == -1 and what in msg, (st, msg)
    assert untouched(buf)


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_with_their_message(what, kw):
    check_refusal(what, kw)


def test_no_mask_and_empty_masks_are_valid_calls():
    st, buf = raw_call([], 3, 5, n=0, null=("pool", "off", "len"), ring_cap=0, xy_cap=0)
    assert st == 0 and buf["need"][:2].tolist() == [0, 0] and buf["ring_first"][0] == 0 and untouched(buf, but=("need", "ring_first"))
    st, buf = raw_call([[15], [15]], 3, 5, ring_cap=0, xy_cap=0)
    assert st == 0 and buf["need"][:2].tolist() == [0, 0] and buf["ring_first"][:3].tolist() == [0, 0, 0]
    assert untouched(buf, but=("need", "ring_first")) and set(buf["ring_first"][3:].tolist()) == {SENTINEL}
    first, off, ln, area2, length, xy = rle.mask_contours([], size=(3, 5))
    assert first.tolist() == [0] and len(off) == len(ln) == len(area2) == len(length) == 0 and xy.shape == (0, 2)
    with pytest.raises(ValueError, match="size=\\(height, width\\) is required"):
        rle.mask_contours([])
    with pytest.raises(ValueError, match="masks of different sizes"):
        rle.mask_contours([{"size": [2, 3], "counts": np.array([6], np.uint32)}, {"size": [3, 2], "counts": np.array([6], np.uint32)}])


PUBLIC = ["frame_with_hole", "hole_with_island", "two_diagonal_pixels", "empty", "pool_of_0", "pool_of_65", "seed_3", "seed_10"]


def public_results(name, connectivity, device):
    masks = cs.get(name)["masks"]
    rings = analyze.mask_contours(masks, connectivity, device=device)
    polys, holes = analyze.masks_to_polygons(masks, connectivity, device=device, return_has_holes=True)
    return rings, polys, holes


def public_bytes(res):
    rings, polys, holes = res
    return ([(r["xy"].tobytes(), r["hole"], r["area"], r["length"]) for m in rings for r in m], [[p.tobytes() for p in m] for m in polys], holes.tobytes())


def check_public_functions(names, device):
    for name in names:
        for k in cs.CONNECTIVITIES:
            rings, polys, holes = public_results(name, k, device)
            want = cs.expected(name, k)
            assert len(rings) == len(polys) == len(holes) == len(want)
            for got, wanted, poly, hole in zip(rings, want, polys, holes):
                assert [r["xy"].tolist() for r in got] == [r["xy"].tolist() for r in wanted]
                assert all(r["xy"].dtype == np.int32 and r["xy"].shape[1] == 2 for r in got)
                assert [(r["hole"], r["area"], r["length"]) for r in got] == [(r["area2"] < 0, abs(r["area2"]) // 2, r["length"]) for r in wanted]
                outer = [r["xy"] for r in wanted if r["area2"] > 0]
                assert len(poly) == len(outer) and all(p.dtype == np.float64 and p.tolist() == o.reshape(-1).tolist() for p, o in zip(poly, outer))
                assert bool(hole) == any(r["area2"] < 0 for r in wanted)


def test_mask_contours_and_masks_to_polygons():
    check_public_functions(PUBLIC, "cpu")
    polys = analyze.masks_to_polygons(cs.get("frame_with_hole")["masks"], device="cpu")               # without has_holes: the polygons alone
    assert [[p.tolist() for p in m] for m in polys] == [[[0, 0, 7, 0, 7, 6, 0, 6]]]


def test_every_mask_form_is_accepted():
    masks, size = cs.get("seed_3")["masks"], cs.size("seed_3")
    want = public_bytes(public_results("seed_3", 2, "cpu"))
    polys = analyze.masks_to_polygons(cs.rles("seed_3"), device="cpu")
    assert [[p.tobytes() for p in m] for m in polys] == want[1]
    filled = _dense(analyze.clean_masks(masks, area_threshold=None, device="cpu"))
    again = analyze.masks_to_polygons(PolygonMasks(polys), size=size, device="cpu")    # polygons in, the same polygons out
    assert [[p.tobytes() for p in m] for m in again] == [[p.tobytes() for p in m] for m in analyze.masks_to_polygons(filled, device="cpu")]
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError, match="connectivity"):
            analyze.mask_contours(masks, bad, device="cpu")
    with pytest.raises(ValueError, match="device"):
        analyze.masks_to_polygons(masks, device="gpu")
    with pytest.raises(ValueError, match="masks of different sizes"):
        analyze.mask_contours([cs.rles("seed_3")[0], cs.rles("seed_10")[0]], device="cpu")
