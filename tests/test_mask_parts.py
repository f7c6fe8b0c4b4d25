"""amp_mask_parts on the host (no GPU needed): the NULL-context path against the scipy.ndimage.label reference of tests/mask_parts_cases.py on every
hand-made and seeded case -- the statistics and every counts array byte for byte, for the parts and for the holes --, the capacity protocol and
every refusal through the raw C call with sentinel words behind the buffers, and the Python surface: rle.mask_parts, analyze.mask_topology,
analyze.clean_masks and the euler_number / filled_area columns of region_properties, compute_rprops and regionprops_table; one spheroidite
annotation taken as ONE mask against label_image_to_rle."""
import ctypes as C
import types

import numpy as np
import pytest
from scipy import ndimage

from ampis_amd import analyze, rle
from ampis_amd._lib import AmpError, lib

import mask_parts_cases as cs
from test_label_runs import ANNOTATIONS, annotation


@pytest.mark.parametrize("name", cs.HAND)
def test_host_equals_the_reference(name):
    cs.check_case(name)


@pytest.mark.parametrize("chunk", range(8))
def test_host_equals_the_reference_on_seeded_cases(chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        cs.check_case(f"seed_{i}")


def test_the_cases_are_what_their_names_say():
    parts = lambda name, i=0: cs.expected(name)[1][0][i].tolist()
    holes = lambda name, i=0: cs.expected(name)[0][0][i].tolist()
    counts = lambda name, colour, i=0: cs.expected(name)[colour][1][i].tolist()
    assert parts("one_pixel") == [1, 1, 1, 0] and holes("one_pixel") == [0, 0, 0, 0] and counts("one_pixel", 1) == [0, 1]
    assert parts("empty") == holes("empty") == [0, 0, 0, 0] and counts("empty", 1) == counts("empty", 0) == [99]
    assert parts("full") == [1, 99, 99, 0] and counts("full", 1) == [0, 99] and counts("full_64x3", 0) == [0, 192]
    assert parts("ring") == [1, 16, 16, 0] and holes("ring") == [1, 9, 9, 9]
    assert holes("ring_keep_hole") == [1, 9, 9, 0] and holes("ring_fill_hole") == [1, 9, 9, 9]        # 9 < 9 is false
    assert parts("ring_min_size_equal") == [1, 16, 16, 0] and parts("ring_min_size_above") == [1, 16, 16, 16]
    assert counts("ring_min_size_above", 1) == [49]
    assert parts("ring_in_ring") == [3, 73, 48, 0] and holes("ring_in_ring") == [2, 96, 72, 0]
    clean, stats = cs.expected("ring_in_ring_clean")["clean"]
    assert clean[0].sum() == 169 and clean[0][1:14, 1:14].all() and stats.tolist() == [[1, 1, 2, 97]]
    clean, stats = cs.expected("ring_in_ring_small_holes")["clean"]                                  # the grown inner hole has 25 pixels: 25 < 25 is false
    assert stats.tolist() == [[1, 1, 0, 0]] and not clean[0][7, 7]
    assert holes("c_closed_by_border") == holes("c_closed_by_border_4") == [0, 0, 0, 0]
    assert holes("hole_corner_8") == [1, 1, 1, 1] and holes("hole_corner_4") == [0, 0, 0, 0]
    assert holes("diamond_at_corner_8") == [1, 1, 1, 1] and holes("diamond_at_corner_4") == [0, 0, 0, 0]
    assert (parts("diamond_at_corner_8")[0], parts("diamond_at_corner_4")[0]) == (1, 4)
    assert (parts("board_2x2_8")[0], parts("board_2x2_4")[0], holes("board_2x2_8")[0], holes("board_2x2_4")[0]) == (1, 2, 0, 0)
    assert (parts("board_8x8_8")[0], holes("board_8x8_8")[0]) == (1, 18) and (parts("board_8x8_4")[0], holes("board_8x8_4")[0]) == (32, 0)
    assert parts("two_equal_parts") == [3, 9, 4, 5] and cs.expected("two_equal_parts")["clean"][0][0][1:3, 1:3].all()
    assert parts("two_equal_parts_row_first") == [2, 8, 4, 4] and cs.expected("two_equal_parts_row_first")["clean"][0][0][4, 1:5].all()
    assert parts("serpentine_65x33")[0] == 1 and parts("serpentine_65x33_complement")[0] == 16
    assert parts("board_130x40_8")[:2] == [1, 2600] and parts("board_130x40_4")[0] == 2600 and holes("board_130x40_8")[0] == 128 * 38 // 2
    assert holes("touches_all_borders") == [1, 67, 67, 67] and parts("touches_all_borders")[0] == 2
    assert parts("empty_columns_between") == [2, 24, 12, 12] and holes("empty_columns_between")[0] == 0
    assert len(cs.get("twelve_masks")["masks"]) == 12
    seeded = [cs.get(f"seed_{i}") for i in range(cs.N_SEEDED)]
    assert {c["connectivity"] for c in seeded} == {1, 2} and {c["keep_largest"] for c in seeded} == {False, True}
    assert any(c["area_threshold"] is None for c in seeded) and any(c["masks"].shape[1] in cs.TALL for c in seeded)
    assert {len(c["masks"]) for c in seeded} == set(range(1, 13))
    assert sum(int(cs.expected(f"seed_{i}")[0][0][:, 0].sum()) for i in range(cs.N_SEEDED)) > 500      # the seeded cases hold real holes


def test_a_call_that_flips_nothing_gives_the_canonical_form_of_its_input():
    m = {"size": [4, 3], "counts": np.array([0, 0, 0, 2, 0, 3, 2, 0, 0, 1, 4], np.uint32)}           # zero-length runs, a run across a column end
    dense = rle.decode(m)
    want = rle.string_to_counts(rle.encode(dense)["counts"])
    for colour in (1, 0):
        for conn in (1, 2):
            stats, (got,) = rle.mask_parts([m], colour, conn)
            assert got.tobytes() == want.tobytes() and stats[0, 3] == 0
    assert rle.mask_parts([m], 1)[0][0].tolist() == [1, 6, 6, 0]


SENTINEL = 0x5EA1ED


def raw_call(counts_list, h, w, colour=1, connectivity=2, threshold=0, keep_largest=0, out_cap=64, ctx=None, null=(), n=None):
    """The C call with marked buffers and GUARD sentinel words behind each capacity: (status, dict of buffers)."""
    pool, off, ln = rle._pool([np.asarray(c, np.uint32) for c in counts_list])
    nn = len(counts_list) if n is None else n
    guard = 8
    buf = {"stats": np.full(4 * max(nn, 0) + guard, SENTINEL, np.uint64), "out_pool": np.full(out_cap + guard, SENTINEL, np.uint32),
           "out_off": np.full(max(nn, 0) + guard, SENTINEL, np.uint64), "out_len": np.full(max(nn, 0) + guard, SENTINEL, np.int32),
           "need": np.full(1 + guard, SENTINEL, np.uint64), "pool": pool, "off": off, "len": ln}
    a = {k: (None if k in null else v.ctypes.data_as(C.c_void_p)) for k, v in buf.items()}
    st = lib().amp_mask_parts(ctx.handle if ctx is not None else None, a["pool"], a["off"], a["len"], nn, h, w, colour, connectivity, threshold,
                              keep_largest, a["stats"], a["out_pool"], out_cap, a["out_off"], a["out_len"], a["need"])
    return st, buf


def untouched(buf, but=()):
    return all(set(v.tolist()) == {SENTINEL} for k, v in buf.items() if k not in ("pool", "off", "len") and k not in but)


def check_capacity_protocol(ctx=None):
    masks = cs.get("twelve_masks")["masks"][:4]
    lists = [rle.string_to_counts(rle.encode(np.asfortranarray(m))["counts"]) for m in masks]
    h, w = masks[0].shape
    st, buf = raw_call(lists, h, w, 0, 2, 0xFFFFFFFF, out_cap=0, ctx=ctx)                             # fill every hole
    assert st == -3 and "counts are needed" in lib().amp_last_error().decode() and untouched(buf, but=("need",))
    total = int(buf["need"][0])
    want = [cs.ref_call(m, 0, 2, None, False) for m in masks]
    want_counts = [rle.string_to_counts(rle.encode(np.asfortranarray(r[1]))["counts"]) for r in want]
    assert total == sum(len(c) for c in want_counts) and set(buf["need"][1:].tolist()) == {SENTINEL}
    st, ok = raw_call(lists, h, w, 0, 2, 0xFFFFFFFF, out_cap=total, ctx=ctx)                          # exactly the need
    assert st == 0, lib().amp_last_error()
    assert ok["need"][0] == total and ok["out_pool"][:total].tobytes() == np.concatenate(want_counts).astype(np.uint32).tobytes()
    assert ok["out_len"][:4].tolist() == [len(c) for c in want_counts] and ok["out_off"][:4].tolist() == np.cumsum([0] + [len(c) for c in want_counts[:-1]]).tolist()
    assert ok["stats"][:16].reshape(4, 4).tolist() == [r[0] for r in want]
    for k, used in (("stats", 16), ("out_pool", total), ("out_off", 4), ("out_len", 4), ("need", 1)):
        assert set(ok[k][used:].tolist()) == {SENTINEL}, k          # nothing behind the result
    st, buf = raw_call(lists, h, w, 0, 2, 0xFFFFFFFF, out_cap=total - 1, ctx=ctx)                     # one less: refused, nothing written
    assert st == -3 and f"{total} counts are needed" in lib().amp_last_error().decode()
    assert buf["need"][0] == total and untouched(buf, but=("need",))
    st, only = raw_call(lists, h, w, 0, 2, 0xFFFFFFFF, out_cap=0, ctx=ctx, null=("out_pool", "out_off", "out_len", "need"))     # statistics only
    assert st == 0 and only["stats"].tobytes() == ok["stats"].tobytes() and untouched(only, but=("stats",))
    return ok


def test_capacity_protocol_on_the_host():
    check_capacity_protocol()


def test_the_sufficient_capacity_of_the_wrapper_is_never_exceeded():
    """sum(len + box width + 1): a flip adds boundaries only at column ends inside the tight box (checked on the case that adds the most)"""
    for name in ("board_130x40_4_keep", "full_64x3", "twelve_masks", "serpentine_65x33_complement"):
        c = cs.get(name)
        for colour in (1, 0):
            got = cs.run(name)[colour][1]
            for m, r, out in zip(c["masks"], cs.rles(name), got):
                cols = np.flatnonzero(m.any(axis=0))
                width = int(cols[-1] - cols[0] + 1) if len(cols) else 0
                assert len(out) <= len(rle.string_to_counts(r["counts"])) + width + 1


# (part of the message, arguments): all AMP_ERR_ARG
GOOD = [[2, 3, 1]]                                                   # a 2 x 3 image
REFUSALS = [
    ("n = -1", dict(n=-1)),
    ("image size 0 x 3", dict(h=0, w=3)),
    ("image size 2 x -7", dict(h=2, w=-7)),
    ("image size 32769 x 2", dict(h=32769, w=2)),
    ("image size 1 x 32769", dict(h=1, w=32769)),
    ("colour = 2", dict(colour=2)),
    ("colour = -1", dict(colour=-1)),
    ("connectivity = 0", dict(connectivity=0)),
    ("connectivity = 3", dict(connectivity=3)),
    ("keep_largest = 2", dict(keep_largest=2)),
    ("keep_largest = 1 with colour = 0", dict(colour=0, keep_largest=1)),
    ("null argument pool", dict(null=("pool",))),
    ("null argument off", dict(null=("off",))),
    ("null argument len", dict(null=("len",))),
    ("null argument stats", dict(null=("stats",))),
    ("null argument out_off", dict(null=("out_off",))),
    ("null argument out_len", dict(null=("out_len",))),
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


def test_the_wrapper_refuses_masks_of_different_sizes():
    a, b = rle.encode(np.ones((3, 4), np.uint8)), rle.encode(np.ones((4, 3), np.uint8))
    with pytest.raises(ValueError, match="different sizes"):
        rle.mask_parts([a, b], 1)
    for fn in (analyze.mask_topology, analyze.clean_masks):
        with pytest.raises(ValueError, match="different sizes"):
            fn([a, b], device="cpu")
    with pytest.raises(AmpError, match="colour = 5"):
        rle.mask_parts([a], 5)
    stats, counts = rle.mask_parts([], 1)
    assert stats.shape == (0, 4) and counts == [] and rle.mask_parts([], 0, emit=False)[1] is None


def check_largest_image(ctx=None):
    """32768 x 32768 = 2^30 pixels, the largest image the call takes: positions up to 2^30 and one piece per column"""
    n, side = 2 ** 30, 32768
    p = 32766 * side + 32766                                         # the pixel (32766, 32766)
    size = [side, side]
    masks = [{"size": size, "counts": np.array([0, n], np.uint32)}, {"size": size, "counts": np.array([0, p, 1, n - p - 1], np.uint32)},
             {"size": size, "counts": np.array([n - 1, 1], np.uint32)}, {"size": size, "counts": np.array([n], np.uint32)}]
    stats, counts = rle.mask_parts(masks, 0, 2, None, ctx=ctx)
    assert stats.tolist() == [[0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert [c.tolist() for c in counts] == [[0, n], [0, n], [n - 1, 1], [n]]
    stats, counts = rle.mask_parts(masks, 1, 1, 2, ctx=ctx)
    assert stats.tolist() == [[1, n, n, 0], [1, n - 1, n - 1, 0], [1, 1, 1, 1], [0, 0, 0, 0]]
    assert [c.tolist() for c in counts] == [[0, n], [0, p, 1, n - p - 1], [n], [n]]
    return stats, counts


def test_the_largest_image():
    check_largest_image()


def check_topology_and_cleaning(names, device):
    """mask_topology, clean_masks and the region_properties columns on the named cases against the reference"""
    for name in names:
        c, want = cs.get(name), cs.expected(name)
        k = c["connectivity"]
        topo = analyze.mask_topology(c["masks"], k, device=device)
        assert list(topo) == ["n_parts", "n_holes", "euler_number", "area", "filled_area", "largest_part_area"]
        assert all(v.dtype == np.int64 and v.shape == (len(c["masks"]),) for v in topo.values())
        parts = np.array([cs.ref_call(m, 1, k, 0, False)[0] for m in c["masks"]]).reshape(-1, 4)
        holes = np.array([cs.ref_call(m, 0, k, 0, False)[0] for m in c["masks"]]).reshape(-1, 4)
        assert topo["n_parts"].tolist() == parts[:, 0].tolist() and topo["n_holes"].tolist() == holes[:, 0].tolist(), name
        assert topo["euler_number"].tolist() == (parts[:, 0] - holes[:, 0]).tolist() and topo["area"].tolist() == parts[:, 1].tolist()
        assert topo["filled_area"].tolist() == (parts[:, 1] + holes[:, 1]).tolist() and topo["largest_part_area"].tolist() == parts[:, 2].tolist()
        got, stats = analyze.clean_masks(cs.rles(name), c["min_size"], c["area_threshold"], c["keep_largest"], k, device=device, return_stats=True)
        assert list(stats) == ["parts_removed", "pixels_removed", "holes_filled", "pixels_filled"]
        assert np.stack(list(stats.values()), axis=1).tolist() == want["clean"][1].tolist(), name
        assert got == [rle.encode(np.asfortranarray(m)) for m in want["clean"][0]], name
        assert got == analyze.clean_masks(c["masks"], c["min_size"], c["area_threshold"], c["keep_largest"], k, device=device)
        if k == 2:
            table = analyze.region_properties(c["masks"], ["area", "euler_number", "filled_area"], device=device)
            assert list(table) == ["area", "euler_number", "filled_area"] and table["euler_number"].dtype == table["filled_area"].dtype == np.int64
            assert table["euler_number"].tolist() == topo["euler_number"].tolist() and table["filled_area"].tolist() == topo["filled_area"].tolist()
            assert table["filled_area"].tolist() == [int(ndimage.binary_fill_holes(m).sum()) for m in c["masks"]], name


def test_mask_topology_clean_masks_and_the_new_columns():
    check_topology_and_cleaning(cs.HAND + [f"seed_{i}" for i in range(0, cs.N_SEEDED, 4)], "cpu")


def test_filled_area_equals_binary_fill_holes_and_euler_number_the_quad_count():
    for i in range(0, cs.N_SEEDED, 3):
        masks = cs.get(f"seed_{i}")["masks"]
        for k in (1, 2):
            topo = analyze.mask_topology(masks, k, device="cpu")
            if k == 2:
                assert topo["filled_area"].tolist() == [int(ndimage.binary_fill_holes(m).sum()) for m in masks]
            for m, e in zip(masks, topo["euler_number"].tolist()):   # the 2 x 2 quad counts of skimage's euler_number (Gray's formula)
                p = np.pad(m, 1).astype(int)
                q = p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:]
                diag = ((q == 2) & (p[:-1, :-1] == p[1:, 1:])).sum()
                assert 4 * e == (q == 1).sum() - (q == 3).sum() + (-2 if k == 2 else 2) * diag, (i, k)


def test_nothing_to_do_is_the_canonical_form_and_steps_are_skipped(monkeypatch):
    calls = []
    real = rle.mask_parts
    monkeypatch.setattr(rle, "mask_parts", lambda *a, **kw: (calls.append((a[1], kw.get("emit", True))), real(*a, **kw))[1])
    r = cs.rles("ring_in_ring")
    loose = [{"size": r[0]["size"], "counts": np.concatenate([rle.string_to_counts(r[0]["counts"])[:1], [0, 0], rle.string_to_counts(r[0]["counts"])[1:]])}]
    assert analyze.clean_masks(loose, device="cpu") == r and calls == [(1, True)]
    del calls[:]
    assert analyze.clean_masks(r, min_size=1, area_threshold=1, device="cpu") == r and calls == [(1, True)]      # nothing is smaller than one pixel
    del calls[:]
    analyze.clean_masks(r, min_size=2, device="cpu")
    analyze.clean_masks(r, area_threshold=None, device="cpu")
    analyze.clean_masks(r, keep_largest=True, area_threshold=5, device="cpu")
    assert calls == [(1, True), (0, True), (1, True), (0, True)]     # at most two calls, a step that changes nothing is skipped
    del calls[:]
    analyze.mask_topology(r, device="cpu")
    assert calls == [(1, False), (0, False)]                         # two statistics-only calls
    assert analyze.clean_masks([], device="cpu") == [] and all(len(v) == 0 for v in analyze.mask_topology([], device="cpu").values())


def test_python_surface_refusals():
    r = cs.rles("ring")
    for fn, kw, match in ((analyze.mask_topology, dict(connectivity=3), "connectivity = 3"), (analyze.mask_topology, dict(device="gpu"), "device = 'gpu'"),
                          (analyze.clean_masks, dict(connectivity=0), "connectivity = 0"), (analyze.clean_masks, dict(device="tpu"), "device = 'tpu'"),
                          (analyze.clean_masks, dict(min_size=-1), "min_size = -1"), (analyze.clean_masks, dict(area_threshold=-2), "area_threshold = -2"),
                          (analyze.clean_masks, dict(min_size=None), "min_size = None")):
        with pytest.raises(ValueError, match=match):
            fn(r, **kw)
    with pytest.raises(ValueError, match="'feret_diameter_max'"):    # still refused, and before the device is looked at
        analyze.region_properties(r, keys=["euler_number", "feret_diameter_max"], device="no such device")
    assert analyze.RPROPS_TOPOLOGY_KEYS == ("euler_number", "filled_area") and not set(analyze.RPROPS_TOPOLOGY_KEYS) & set(analyze.RPROPS_KEYS)
    assert len(analyze.RPROPS_KEYS) == 13


def test_compute_rprops_and_regionprops_table_take_the_new_keys():
    masks = cs.get("twelve_masks")["masks"]
    inst = types.SimpleNamespace(masks=cs.rles("twelve_masks"), image_size=masks.shape[1:], class_idx=np.arange(12))
    iset = types.SimpleNamespace(instances=inst, rprops=None)
    df = analyze.compute_rprops(iset, keys=["area", "perimeter", "euler_number", "filled_area"], return_df=True, device="cpu")
    assert list(df.columns) == ["area", "perimeter", "euler_number", "filled_area", "class_idx"] and iset.rprops is df
    topo = analyze.mask_topology(masks, device="cpu")
    assert df["euler_number"].tolist() == topo["euler_number"].tolist() and df["filled_area"].tolist() == topo["filled_area"].tolist()
    assert df["euler_number"].tolist()[:5] == [1, 1, 0, 1, 0] and df["filled_area"].tolist()[:5] == [169, 1, 0, 225, 25]      # the empty mask: 0 and 0
    lab = np.zeros((9, 9), int)
    lab[1:6, 1:6] = 3; lab[2:5, 2:5] = 0; lab[3, 3] = 7; lab[8, 0] = lab[6, 8] = 3                    # label 3: a ring and two specks, label 7 inside it
    table = analyze.regionprops_table(lab, ["area", "euler_number", "filled_area"])
    assert table["area"].tolist() == [18, 1] and table["euler_number"].tolist() == [2, 1] and table["filled_area"].tolist() == [27, 1]


def check_annotation_as_one_mask(device):
    """One spheroidite annotation as ONE mask: its parts are the instances label_image_to_rle finds, the largest part is that call's largest"""
    fg = annotation(ANNOTATIONS[1][0])
    one = [rle.encode(np.asfortranarray(fg))]
    for conn in (1, 2):
        rles, _, areas, _ = analyze.label_image_to_rle(fg, "binary", conn, device=device)
        topo = analyze.mask_topology(one, conn, device=device)
        assert topo["n_parts"].tolist() == [len(rles)] == [ANNOTATIONS[1][2 if conn == 1 else 1]]
        assert topo["area"].tolist() == [int(fg.sum())] and topo["largest_part_area"].tolist() == [int(areas.max())]
        lab, n = ndimage.label(~fg, structure=cs.STRUCTURE[3 - conn])
        inner = np.setdiff1d(np.arange(1, n + 1), np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        assert topo["n_holes"].tolist() == [len(inner)] and topo["filled_area"].tolist() == [int(fg.sum() + np.isin(lab, inner).sum())]
        best = min(range(len(rles)), key=lambda i: (-int(areas[i]), int(np.flatnonzero(rle.decode(rles[i]).ravel(order="F"))[0])))
        (kept,), stats = analyze.clean_masks(one, keep_largest=True, connectivity=conn, device=device, return_stats=True)
        assert kept["counts"] == rles[best]["counts"] and kept["size"] == rles[best]["size"]
        assert stats["parts_removed"].tolist() == [len(rles) - 1] and stats["pixels_removed"].tolist() == [int(fg.sum() - areas.max())]


def test_spheroidite_annotation_as_one_mask():
    check_annotation_as_one_mask("cpu")
