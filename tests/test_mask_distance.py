"""amp_mask_distance on the host (no GPU needed): the NULL-context path against scipy on one decoded mask (tests/mask_distance_ref.py) on every
case of tests/mask_distance_cases.py -- both border values, ncurve 0, 1, 9 and 1025, with and without the map --, byte for byte: stats, boxes,
curve and map; the largest sides against their closed forms; the identities with the project's own erosion; the capacity protocol and every
refusal through the raw C call with sentinel words behind the buffers; the Python surface: rle.mask_distance, analyze.mask_distance_maps /
inscribed_circles / erosion_curve and region_properties' inscribed_radius."""
import ctypes as C

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import lib

import mask_distance_cases as cs

N_CHUNKS = 10
PER_CHUNK = cs.N_SEEDED // N_CHUNKS


@pytest.mark.parametrize("name", cs.HAND)
def test_host_equals_the_reference(name):
    for b in cs.BORDERS:
        cs.check_case(name, b)


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_host_equals_the_reference_on_seeded_cases(chunk):
    for name in cs.SEEDED[chunk * PER_CHUNK: (chunk + 1) * PER_CHUNK]:
        for b in cs.BORDERS:
            cs.check_case(name, b)


def check_largest(name, ctx=None):
    out = []
    for b in cs.BORDERS:
        sz, ins, want = cs.largest(name, b)
        for ncurve in cs.LARGEST_NCURVES:
            res = rle.mask_distance(ins, b, ncurve, True, ctx=ctx, size=sz)
            cs.equal_to(res, want, ncurve, (name, b, ncurve))
            out.append(cs.result_bytes(res))
    return out


@pytest.mark.parametrize("name", cs.LARGEST)
def test_the_largest_sides(name):
    check_largest(name)


def check_the_2_30_image(ctx=None):
    """the frame with a square in every corner: statistics and curve only, its map would be the image; three small rectangles with positions of
    30 bits: everything"""
    out = []
    for b in cs.BORDERS:
        stats, boxes, curve, maps = rle.mask_distance(cs.frame_inputs(), b, 9, False, ctx=ctx)
        want = cs.frame_expected(b, 9)
        assert maps is None and (stats.tolist(), boxes.tolist(), curve.tolist()) == want, b
        far = rle.mask_distance(cs.far_inputs(), b, 9, True, ctx=ctx)
        cs.equal_to(far, cs.far_expected(b), 9, ("far", b))
        out += [stats.tobytes(), boxes.tobytes(), curve.tobytes(), cs.result_bytes(far)]
    return out


def test_the_2_30_image():
    check_the_2_30_image()


def test_the_cases_are_what_their_names_say():
    assert cs.expected("full_image", 1)[0]["stats"] == [cs.NONE, 0, 0, 30] and cs.expected("full_image", 0)[0]["stats"][0] == 9
    assert cs.expected("square_2x2", 0)[0]["map"].tolist() == [[1, 1], [1, 1]]
    assert any(0 in rle._counts(r)[1:-1].tolist() for r in cs.rles("zero_length_runs"))
    assert cs.expected("an_empty_mask_between_two_others", 0)[1]["stats"] == [0, 0, 0, 0]
    ring = cs.expected("ring", 1)[0]
    h = cs.size("ring")[0]
    r, c = ring["stats"][1] % h, ring["stats"][1] // h               # the deepest pixel lies between the hole and the outside
    assert 6 < (r - 8) ** 2 + (c - 8) ** 2 < 60
    far = cs.expected("background_in_a_far_column_only", 1)[0]["map"]
    assert far[2, 0] == 35 * 35 and far[0, 0] == 35 * 35 + 4 and far[2, 39] == 16 and cs.expected("background_in_a_far_column_only", 0)[0]["stats"][0] == 9
    tall = cs.get("piece_130_rows_tall")["masks"]
    assert tall[0, 2:132, 1].all() and tall[0].any(axis=1).sum() == 130
    sizes = [cs.size(s) for s in cs.SEEDED]
    assert max(s[0] for s in sizes) == 40 and max(s[1] for s in sizes) == 40


# ---- identities with the project's own erosion -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(4))
def test_the_curve_is_the_area_of_the_disk_erosion(chunk):
    for name in cs.SEEDED[chunk * 10: chunk * 10 + 10] + (cs.HAND if chunk == 0 else ()):
        masks = list(cs.rles(name))
        if not masks:
            continue
        stats, _, curve, _ = rle.mask_distance(masks, 0, 8, size=cs.size(name))
        for r in range(8):
            eroded = analyze.erode_masks(masks, "disk", r, border_value=0, device="cpu", return_stats=True)[1]["area"]
            assert curve[:, r].tolist() == eroded.tolist(), (name, r)
            assert (stats[:, 0] > r * r).tolist() == (eroded > 0).tolist(), (name, r)      # d2_max > r^2 exactly when something survives


# ---- the raw C call: capacities and refusals ------------------------------------------------------------------------------------------------------

SENTINEL = 0xA5A5A5A5
TAIL = 8


def raw_call(counts_list, h, w, border_value=0, ncurve=3, map_cap=64, ctx=None, n=None, null=()):
    """the call on buffers with TAIL sentinel words behind what the call may write; (status, buffers)"""
    k = len(counts_list)
    n = k if n is None else n
    pool, off, ln = rle._pool([np.asarray(c, np.uint32) for c in counts_list])
    m = max(k, 1)
    buf = {"stats": np.full(4 * m + TAIL, SENTINEL, np.uint64), "boxes": np.full(4 * m + TAIL, SENTINEL, np.int64),
           "curve": np.full(m * max(ncurve, 0) + TAIL, SENTINEL, np.uint64), "map": np.full(map_cap + TAIL, SENTINEL, np.uint32),
           "map_off": np.full(m + TAIL, SENTINEL, np.uint64), "need": np.full(1 + TAIL, SENTINEL, np.uint64)}
    ins = {"pool": pool, "off": off, "len": ln}
    p = lambda name: None if name in null else (ins[name] if name in ins else buf[name]).ctypes.data_as(C.c_void_p)
    st = lib().amp_mask_distance(ctx.handle if ctx is not None else None, p("pool"), p("off"), p("len"), n, h, w, border_value, p("stats"),
                                 p("boxes"), p("curve"), ncurve, p("map"), map_cap, p("map_off"), p("need"))
    return st, buf


def untouched(buf, but=()):
    return all(set(a.tolist()) <= {SENTINEL} for name, a in buf.items() if name not in but)


def check_capacity_protocol(ctx=None, name="seed_7", b=0, ncurve=9):
    counts = [rle._counts(r) for r in cs.rles(name)]
    (h, w), n = cs.size(name), len(counts)
    want = cs.expected(name, b)
    need = sum(x["map"].size for x in want)
    assert need > 1
    st, buf = raw_call(counts, h, w, b, ncurve, map_cap=0, ctx=ctx)
    assert st == -3 and int(buf["need"][0]) == need and untouched(buf, but=("need",))
    assert f"map_cap = 0; {need} counts are needed" in lib().amp_last_error().decode()
    st, short = raw_call(counts, h, w, b, ncurve, map_cap=need - 1, ctx=ctx)             # one word short: refused, the need again, nothing else written
    assert st == -3 and int(short["need"][0]) == need and untouched(short, but=("need",))
    assert f"map_cap = {need - 1}; {need} counts are needed" in lib().amp_last_error().decode()
    st, buf = raw_call(counts, h, w, b, ncurve, map_cap=need, ctx=ctx)                   # exactly the need
    assert st == 0 and int(buf["need"][0]) == need
    assert set(buf["map"][need:].tolist()) == {SENTINEL} and set(buf["map_off"][n:].tolist()) == {SENTINEL}           # the words behind the result
    assert set(buf["stats"][4 * n:].tolist()) == {SENTINEL} and set(buf["boxes"][4 * n:].tolist()) == {SENTINEL}
    assert set(buf["curve"][n * ncurve:].tolist()) == {SENTINEL} and set(buf["need"][1:].tolist()) == {SENTINEL}
    assert buf["map_off"][:n].tolist() == np.concatenate([[0], np.cumsum([x["map"].size for x in want])[:-1]]).tolist()
    assert buf["map"][:need].tolist() == np.concatenate([x["map"].reshape(-1) for x in want]).tolist()
    assert buf["stats"][:4 * n].reshape(n, 4).tolist() == [x["stats"] for x in want] and buf["boxes"][:4 * n].reshape(n, 4).tolist() == [x["box"] for x in want]
    assert buf["curve"][:n * ncurve].reshape(n, ncurve).tolist() == [x["curve"][ncurve] for x in want]
    st, none = raw_call(counts, h, w, b, ncurve, map_cap=0, ctx=ctx, null=("map", "map_off", "need"))    # without a map nothing of it is used
    assert st == 0 and untouched(none, but=("stats", "boxes", "curve")) and none["stats"].tobytes() == buf["stats"].tobytes()
    return buf


def test_capacity_protocol_on_the_host():
    check_capacity_protocol()
    check_capacity_protocol(name="checkerboard", b=1, ncurve=1)


GOOD = [[2, 3, 1]]                                                   # a 2 x 3 image
REFUSALS = [
    ("n = -1", dict(n=-1)),
    ("image size 0 x 3", dict(h=0, w=3)),
    ("image size 2 x -7", dict(h=2, w=-7)),
    ("image size 32769 x 2", dict(h=32769, w=2)),
    ("image size 1 x 32769", dict(h=1, w=32769)),
    ("image size 32768 x 32769", dict(h=32768, w=32769)),
    ("border_value = 2", dict(border_value=2)),
    ("border_value = -1", dict(border_value=-1)),
    ("ncurve = -1", dict(ncurve=-1)),
    ("ncurve = 1026", dict(ncurve=1026)),
    ("null argument curve with ncurve = 3", dict(null=("curve",))),
    ("map_cap = 64 with a null map", dict(null=("map",))),
    ("null argument need", dict(null=("need",))),
    ("null argument need", dict(null=("need",), counts_list=[], n=0)),
    ("null argument pool", dict(null=("pool",))),
    ("null argument off", dict(null=("off",))),
    ("null argument len", dict(null=("len",))),
    ("null argument stats", dict(null=("stats",))),
    ("null argument boxes", dict(null=("boxes",))),
    ("null argument map_off", dict(null=("map_off",))),
    ("mask 0 has an empty run list", dict(counts_list=[[]])),
    ("the runs of mask 1 cover more than the image's 6 pixels", dict(counts_list=[[6], [2, 3, 2]])),
    ("the runs of mask 1 cover 5 pixels, the image has 6", dict(counts_list=[[0, 6], [2, 3]])),
    ("the runs of mask 0 cover 6 pixels, the image has 8", dict(h=2, w=4)),      # a run list of another image size
]


def check_refusal(what, kw, ctx=None):
    kw = dict(kw)
    st, buf = raw_call(kw.pop("counts_list", GOOD), kw.pop("h", 2), kw.pop("w", 3), ctx=ctx, **kw)
    msg = lib().amp_last_error().decode()
    assert st == -1 and msg.startswith("amp_mask_distance: ") and what in msg, (st, msg)
    assert untouched(buf)


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_with_their_message(what, kw):
    check_refusal(what, kw)


def test_no_mask_empty_and_full_masks_are_valid_calls():
    st, buf = raw_call([], 3, 5, n=0, null=("pool", "off", "len", "stats", "boxes", "map_off"), map_cap=0)
    assert st == 0 and int(buf["need"][0]) == 0 and untouched(buf, but=("need",))
    st, buf = raw_call([], 3, 5, n=0, ncurve=0, map_cap=0, null=("pool", "off", "len", "stats", "boxes", "curve", "map", "map_off", "need"))
    assert st == 0 and untouched(buf)
    st, buf = raw_call([[15], [0, 15]], 3, 5, border_value=1, ncurve=2, map_cap=15)
    assert st == 0 and buf["stats"][:8].tolist() == [0, 0, 0, 0, cs.NONE, 0, 0, 15] and buf["boxes"][:8].tolist() == [0, 0, 0, 0, 0, 0, 3, 5]
    assert buf["curve"][:4].tolist() == [0, 0, 15, 15] and buf["map"][:15].tolist() == [cs.NONE] * 15 and buf["map_off"][:2].tolist() == [0, 0]
    st, buf = raw_call([[15], [0, 15]], 3, 5, border_value=0, ncurve=3, map_cap=15)
    assert st == 0 and buf["stats"][4:8].tolist() == [4, 1 * 3 + 1, 12 + 3 * 4, 15] and buf["curve"][3:6].tolist() == [15, 3, 0]
    assert buf["map"][:15].reshape(3, 5).tolist() == [[1] * 5, [1, 4, 4, 4, 1], [1] * 5]
    stats, boxes, curve, maps = rle.mask_distance([], 0, 4, True)
    assert stats.shape == (0, 4) and boxes.shape == (0, 4) and curve.shape == (0, 4) and maps == [] and rle.mask_distance([], size=(3, 5))[3] is None
    with pytest.raises(ValueError, match="masks of different sizes"):
        rle.mask_distance([{"size": [2, 3], "counts": np.array([6], np.uint32)}, {"size": [3, 2], "counts": np.array([6], np.uint32)}])
    for kw in (dict(border_value=2), dict(border_value=True), dict(ncurve=-1), dict(ncurve=1026), dict(ncurve=1.5), dict(ncurve=True)):
        with pytest.raises(ValueError, match="mask_distance: "):
            rle.mask_distance(list(cs.rles("full_image")), **kw)


# ---- the public functions --------------------------------------------------------------------------------------------------------------------------

PUBLIC = ("maps", "maps_squared", "circles", "curve", "rprops")


def public_pool():
    """a disk, an empty mask, the full image and an L of one 12 x 14 image"""
    m = np.zeros((4, 12, 14), bool)
    yy, xx = np.indices((12, 14))
    m[0] = (yy - 5) ** 2 + (xx - 6) ** 2 <= 16
    m[2] = True
    m[3, 1:10, 2:5] = True; m[3, 7:10, 2:12] = True
    return m


def public_results(name, device, b=1):
    m = public_pool()
    if name == "maps":
        return analyze.mask_distance_maps(m, b, device=device)
    if name == "maps_squared":
        return analyze.mask_distance_maps(m, b, squared=True, device=device)
    if name == "circles":
        return analyze.inscribed_circles(m, b, device=device)
    if name == "curve":
        return analyze.erosion_curve(m, 6, b, device=device)
    return analyze.region_properties(m, keys=["area", "inscribed_radius"], device=device)


def public_bytes(res):
    if isinstance(res, np.ndarray):
        return (str(res.dtype), res.shape, res.tobytes())
    if isinstance(res, dict):
        return tuple((k, public_bytes(v)) for k, v in res.items())
    if isinstance(res, (list, tuple)) and not (res and isinstance(res[0], (int, np.integer))):
        return tuple(public_bytes(v) for v in res)
    return res


def check_public_functions(device):
    m = public_pool()
    want = {b: [cs.ref.outputs(x, cs.ref.scipy_d2(x, b), (7,)) for x in m] for b in cs.BORDERS}
    for b in cs.BORDERS:
        maps = public_results("maps", device, b)
        sq = public_results("maps_squared", device, b)
        assert [x["bbox"] for x in maps] == [tuple(w["box"]) for w in want[b]] == [x["bbox"] for x in sq]
        for got, got2, w in zip(maps, sq, want[b]):
            assert got2["distance"].dtype == np.uint32 and got2["distance"].tobytes() == w["map"].tobytes()
            assert got["distance"].dtype == np.float64 and got["distance"].shape == w["map"].shape
            root = np.sqrt(w["map"].astype(np.float64))
            root[w["map"] == cs.NONE] = np.inf
            assert got["distance"].tobytes() == root.tobytes()
        assert maps[1]["bbox"] == (0, 0, 0, 0) and maps[1]["distance"].shape == (0, 0)
        assert np.isinf(maps[2]["distance"]).all() == (b == 1)
        circ = public_results("circles", device, b)
        assert list(circ) == ["d2", "radius", "row", "col", "center_xy"]
        assert all(circ[k].dtype == np.int64 and circ[k].shape == (4,) for k in ("d2", "row", "col"))
        assert circ["radius"].dtype == np.float64 and circ["center_xy"].dtype == np.float64 and circ["center_xy"].shape == (4, 2)
        assert circ["d2"].tolist() == [w["stats"][0] for w in want[b]]
        assert circ["row"].tolist() == [w["stats"][1] % 12 if w["stats"][3] else -1 for w in want[b]]
        assert circ["col"].tolist() == [w["stats"][1] // 12 if w["stats"][3] else -1 for w in want[b]]
        assert circ["radius"][0] == np.sqrt(float(want[b][0]["stats"][0])) and circ["radius"][1] == 0.0 and circ["row"][1] == circ["col"][1] == -1
        assert np.isnan(circ["center_xy"][1]).all() and circ["center_xy"][0].tolist() == [circ["col"][0] + 0.5, circ["row"][0] + 0.5]
        assert (circ["radius"][2] == np.inf and circ["d2"][2] == cs.NONE and (circ["row"][2], circ["col"][2]) == (0, 0)) if b else circ["radius"][2] == 6.0
        curve = public_results("curve", device, b)
        assert curve.dtype == np.int64 and curve.shape == (4, 7) and curve.tolist() == [w["curve"][7] for w in want[b]]
    rp = public_results("rprops", device)
    assert list(rp) == ["area", "inscribed_radius"] and rp["area"].dtype == np.int64 and rp["inscribed_radius"].dtype == np.float64
    assert rp["inscribed_radius"].tolist() == public_results("circles", device, 0)["radius"].tolist() and rp["inscribed_radius"][1] == 0.0
    assert rp["area"].tolist() == [w["stats"][3] for w in want[0]]


def test_public_functions_on_the_host():
    check_public_functions("cpu")


def test_the_existing_columns_of_region_properties_are_unchanged():
    assert analyze.RPROPS_DISTANCE_KEYS == ("inscribed_radius",)
    assert analyze.RPROPS_DEFAULT_KEYS == ["area", "equivalent_diameter", "major_axis_length", "perimeter", "solidity", "orientation"]
    assert "inscribed_radius" not in analyze.RPROPS_KEYS + analyze.RPROPS_TOPOLOGY_KEYS
    m = public_pool()
    assert list(analyze.region_properties(m, device="cpu")) == analyze.RPROPS_DEFAULT_KEYS
    both = analyze.region_properties(m, keys=["solidity", "inscribed_radius", "euler_number", "bbox"], device="cpu")
    alone = analyze.region_properties(m, keys=["solidity", "euler_number", "bbox"], device="cpu")
    assert list(both) == ["solidity", "inscribed_radius", "euler_number", "bbox-0", "bbox-1", "bbox-2", "bbox-3"]
    assert all(both[k].tobytes() == alone[k].tobytes() for k in alone)
    with pytest.raises(ValueError, match="unsupported key 'radius'"):
        analyze.region_properties(m, keys=["radius"], device="cpu")


def test_public_arguments_are_checked_first():
    m = public_pool()
    for fn, kw in ((analyze.mask_distance_maps, dict(border_value=2)), (analyze.inscribed_circles, dict(border_value=True)),
                   (analyze.erosion_curve, dict(max_radius=3, border_value=-1)), (analyze.erosion_curve, dict(max_radius=-1)),
                   (analyze.erosion_curve, dict(max_radius=1025)), (analyze.erosion_curve, dict(max_radius=2.0)),
                   (analyze.inscribed_circles, dict(device="gpu")), (analyze.mask_distance_maps, dict(device="tpu"))):
        with pytest.raises(ValueError, match=fn.__name__ + ": "):
            fn(m, **kw)
    two = [rle.encode(np.asfortranarray(np.ones((2, 3), bool))), rle.encode(np.asfortranarray(np.ones((3, 2), bool)))]
    for fn in (analyze.mask_distance_maps, analyze.inscribed_circles, lambda x, device: analyze.erosion_curve(x, 2, device=device)):
        with pytest.raises(ValueError, match="masks of different sizes"):
            fn(two, device="cpu")
    assert analyze.mask_distance_maps([], size=(4, 5), device="cpu") == [] and analyze.erosion_curve([], 3, size=(4, 5), device="cpu").shape == (0, 4)
    assert analyze.inscribed_circles([], size=(4, 5), device="cpu")["center_xy"].shape == (0, 2)
    assert analyze.erosion_curve(m, 1024, device="cpu").shape == (4, 1025)
