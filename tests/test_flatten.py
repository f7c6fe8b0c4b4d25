"""amp_flatten_instances on the host (no GPU needed): the NULL-context path against the dense-loop reference of tests/flatten_cases.py on every
hand-made and seeded case -- the label image, every visible list byte for byte, statistics, boxes, pixel classes, the inverse through
label_image_to_rle and the area of the union --, the capacity protocol and every refusal through the raw C call with sentinel words behind
the buffers, and the Python surface: rle.flatten_instances, analyze.resolve_overlaps, analyze.instances_to_label_image; one spheroidite
annotation from label image to instances and back."""
import ctypes as C

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import AmpError, lib
from ampis_amd.structures import Instances, InstanceSet, PolygonMasks, RLEMasks

import flatten_cases as cs
from test_label_runs import ANNOTATIONS, annotation


@pytest.mark.parametrize("name", cs.HAND)
def test_host_equals_the_reference(name):
    cs.check_case(name)


@pytest.mark.parametrize("chunk", range(8))
def test_host_equals_the_reference_on_seeded_cases(chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        cs.check_case(f"seed_{i}")


@pytest.mark.parametrize("name", cs.LARGEST)
def test_the_largest_sides(name):
    cs.check_case(name)


def test_the_cases_are_what_their_names_say():
    e = cs.expected
    assert e("full_under")["stats"][3].tolist() == [99, 99 - int(cs.get("full_under")["masks"][:3].any(axis=0).sum())]
    assert e("full_over")["stats"][:, 1].tolist() == [99, 0, 0, 0] and [c.tolist() for c in e("full_over")["counts"]] == [[0, 99], [99], [99], [99]]
    assert e("full_over_by_rank")["stats"][:, 1].tolist() == [0, 0, 0, 99]
    assert e("two_identical")["stats"].tolist() == [[20, 20], [20, 0]] and e("two_identical")["boxes"].tolist() == [[1, 1, 5, 6], [0, 0, 0, 0]]
    assert e("two_identical_second_wins")["stats"].tolist() == [[20, 0], [20, 20]]
    outer, inner = e("ring_in_ring_outer_on_top")["stats"], e("ring_in_ring_inner_on_top")["stats"]
    assert outer[0, 0] == outer[0, 1] and outer[1, 1] < outer[1, 0] and inner[1, 0] == inner[1, 1] and inner[0, 1] < inner[0, 0]
    assert e("join_across_column_ends")["counts"][0].tolist() == [0, 5, 5, 10]           # [10, 20) is one run across two column ends
    assert e("join_across_column_ends_partial")["counts"][0].tolist() == [0, 5, 4, 11]
    assert e("empty_first_middle_last")["stats"][[0, 3, 5]].tolist() == [[0, 0]] * 3 and e("only_empty")["pixels"].tolist() == [99, 0, 0]
    assert e("no_mask")["pixels"].tolist() == [42, 0, 0] and not e("no_mask")["labels"].any() and e("no_mask")["counts"] == []
    assert e("ranks_all_equal")["labels"].tobytes() == e("full_under")["labels"].tobytes()            # equal ranks: index order
    assert e("ranks_descending")["stats"][:, 1].tolist() == [0, 0, 0, 99]
    z = e("ranks_zero_and_top")["stats"]
    assert z[1, 1] == z[1, 0] and z[3, 1] == z[3, 0] and z[0, 1] == 99 - z[1, 0] - z[3, 0] and z[2, 1] == 0
    many = e("300_on_one_block")
    assert many["pixels"].tolist() == [4900 - 64 - 300, 300, 64] and sorted(many["stats"][:, 1].tolist())[-2:] == [1, 65]
    dots = e("5041_single_pixels")
    assert dots["pixels"].tolist() == [0, 5041, 0] and dots["stats"].tolist() == [[1, 1]] * 5041
    assert sum(len(c) for c in e("checkerboard_66x3")["counts"]) == 393
    seeded = [cs.get(f"seed_{i}") for i in range(cs.N_SEEDED)]
    assert {len(c["masks"]) for c in seeded} == set(range(1, 13)) and any(c["rank"] is None for c in seeded)
    assert any(c["rank"] is not None and len(set(c["rank"].tolist())) < len(c["rank"]) for c in seeded)             # ties
    assert max(max(c["masks"].shape[1:]) for c in seeded) > 128 and sum(int(cs.expected(f"seed_{i}")["pixels"][2]) for i in range(cs.N_SEEDED)) > 10000


SENTINEL = 0x5EA1ED
GUARD = 8


def raw_call(counts_list, h, w, rank=None, counts_cap=64, ctx=None, null=(), n=None, labels=True):
    """The C call with marked buffers and GUARD sentinel words behind each: (status, dict of buffers)."""
    pool, off, ln = rle._pool([np.asarray(c, np.uint32) for c in counts_list])
    nn = len(counts_list) if n is None else n
    k = max(nn, 0)
    pixels = max(h, 0) * max(w, 0) if labels and 0 < h <= 32768 and 0 < w <= 32768 else 0
    buf = {"labels": np.full(pixels + GUARD, SENTINEL, np.int32), "counts": np.full(counts_cap + GUARD, SENTINEL, np.uint32),
           "counts_off": np.full(k + GUARD, SENTINEL, np.uint64), "counts_len": np.full(k + GUARD, SENTINEL, np.int32),
           "stats": np.full(2 * k + GUARD, SENTINEL, np.uint64), "boxes": np.full(4 * k + GUARD, SENTINEL, np.int32),
           "pixels": np.full(3 + GUARD, SENTINEL, np.uint64), "need": np.full(1 + GUARD, SENTINEL, np.uint64), "pool": pool, "off": off, "len": ln,
           "rank": None if rank is None else np.ascontiguousarray(rank, dtype=np.uint32)}
    a = {key: (None if key in null or v is None else v.ctypes.data_as(C.c_void_p)) for key, v in buf.items()}
    if not labels:
        a["labels"] = None
    st = lib().amp_flatten_instances(ctx.handle if ctx is not None else None, a["pool"], a["off"], a["len"], nn, h, w, a["rank"], a["labels"],
                                     a["counts"], counts_cap, a["counts_off"], a["counts_len"], a["stats"], a["boxes"], a["pixels"], a["need"])
    return st, buf


def untouched(buf, but=()):
    return all(set(v.tolist()) == {SENTINEL} for k, v in buf.items() if k not in ("pool", "off", "len", "rank") and k not in but)


def check_capacity_protocol(ctx=None, name="seed_7"):
    lists, rank, (h, w) = [r["counts"] for r in cs.rles(name)], cs.get(name)["rank"], cs.size(name)
    want = cs.expected(name)
    n, total = len(lists), sum(len(c) for c in want["counts"])
    st, buf = raw_call(lists, h, w, rank, counts_cap=0, ctx=ctx)
    assert st == -3 and f"counts_cap = 0; {total} counts are needed" in lib().amp_last_error().decode() and untouched(buf, but=("need",))
    assert int(buf["need"][0]) == total and set(buf["need"][1:].tolist()) == {SENTINEL}          # the exact need
    st, ok = raw_call(lists, h, w, rank, counts_cap=total, ctx=ctx)                              # exactly the need
    assert st == 0, lib().amp_last_error()
    assert ok["need"][0] == total and ok["counts"][:total].tobytes() == np.concatenate(want["counts"]).astype(np.uint32).tobytes()
    lens = [len(c) for c in want["counts"]]
    assert ok["counts_len"][:n].tolist() == lens and ok["counts_off"][:n].tolist() == np.cumsum([0] + lens[:-1]).tolist()
    assert ok["stats"][:2 * n].reshape(n, 2).tolist() == want["stats"].tolist() and ok["boxes"][:4 * n].reshape(n, 4).tolist() == want["boxes"].tolist()
    assert ok["pixels"][:3].tolist() == want["pixels"].tolist() and ok["labels"][:h * w].tobytes() == want["labels"].tobytes()
    for k, used in (("labels", h * w), ("counts", total), ("counts_off", n), ("counts_len", n), ("stats", 2 * n), ("boxes", 4 * n), ("pixels", 3), ("need", 1)):
        assert set(ok[k][used:].tolist()) == {SENTINEL}, k          # nothing behind the result
    st, buf = raw_call(lists, h, w, rank, counts_cap=total - 1, ctx=ctx)                         # one short: refused, nothing written
    assert st == -3 and f"counts_cap = {total - 1}; {total} counts are needed" in lib().amp_last_error().decode()
    assert buf["need"][0] == total and untouched(buf, but=("need",))
    st, only = raw_call(lists, h, w, rank, counts_cap=0, ctx=ctx, null=("counts", "counts_off", "counts_len", "need"))         # no lists
    assert st == 0 and untouched(only, but=("labels", "stats", "boxes", "pixels"))
    assert all(only[k].tobytes() == ok[k].tobytes() for k in ("labels", "stats", "boxes", "pixels"))
    st, bare = raw_call(lists, h, w, rank, counts_cap=0, ctx=ctx, null=("counts", "counts_off", "counts_len", "need"), labels=False)
    assert st == 0 and untouched(bare, but=("stats", "boxes", "pixels")) and bare["stats"].tobytes() == ok["stats"].tobytes()
    return ok


def test_capacity_protocol_on_the_host():
    check_capacity_protocol()
    check_capacity_protocol(name="checkerboard_66x3")


def test_the_stated_capacity_always_suffices():
    """2 x the sum of the input lengths.  check_case asserts it on every case; here the cases that come closest, and a call with a
    capacity of exactly the bound."""
    worst = 0.0
    for name in cs.names():
        got = sum(len(c) for c in cs.expected(name)["counts"])
        bound = cs.capacity_bound(name)
        assert got <= bound, name
        worst = max(worst, got / bound) if bound else worst
    assert 0.9 < worst <= 1.0
    name = "checkerboard_66x3_full_under"
    st, buf = raw_call([r["counts"] for r in cs.rles(name)], 66, 3, cs.get(name)["rank"], counts_cap=cs.capacity_bound(name))
    assert st == 0 and int(buf["need"][0]) <= cs.capacity_bound(name)


# (part of the message, arguments): all AMP_ERR_ARG
GOOD = [[2, 3, 1]]                                                   # a 2 x 3 image
REFUSALS = [
    ("n = -1", dict(n=-1)),
    ("image size 0 x 3", dict(h=0, w=3)),
    ("image size 2 x -7", dict(h=2, w=-7)),
    ("image size 32769 x 2", dict(h=32769, w=2)),
    ("image size 1 x 32769", dict(h=1, w=32769)),
    ("image size 32768 x 32769", dict(h=32768, w=32769)),
    ("null argument pixels", dict(null=("pixels",))),
    ("null argument pixels", dict(null=("pixels",), counts_list=[], n=0)),
    ("null argument pool", dict(null=("pool",))),
    ("null argument off", dict(null=("off",))),
    ("null argument len", dict(null=("len",))),
    ("null argument stats", dict(null=("stats",))),
    ("null argument boxes", dict(null=("boxes",))),
    ("null argument counts_off", dict(null=("counts_off",))),
    ("null argument counts_len", dict(null=("counts_len",))),
    ("null argument need", dict(null=("need",))),
    ("counts_cap = 64 with counts NULL", dict(null=("counts",))),
    ("mask 0 has an empty run list", dict(counts_list=[[]])),
    ("the runs of mask 1 cover more than the image's 6 pixels", dict(counts_list=[[6], [2, 3, 2]])),
    ("the runs of mask 1 cover 5 pixels, the image has 6", dict(counts_list=[[0, 6], [2, 3]])),
    ("the runs of mask 2 cover 5 pixels, the image has 6", dict(counts_list=[[0, 6], [6], [2, 3]], rank=[2, 1, 0])),
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


def test_no_mask_is_a_valid_call():
    st, buf = raw_call([], 3, 5, n=0, null=("pool", "off", "len", "stats", "boxes", "counts_off", "counts_len"))
    assert st == 0 and buf["pixels"][:3].tolist() == [15, 0, 0] and buf["need"][0] == 0 and not buf["labels"][:15].any()
    assert untouched(buf, but=("pixels", "need", "labels"))
    stats, boxes, pixels, counts, labels = rle.flatten_instances([], size=(3, 5), return_labels=True)
    assert stats.shape == (0, 2) and boxes.shape == (0, 4) and pixels.tolist() == [15, 0, 0] and counts == [] and labels.shape == (3, 5)
    with pytest.raises(ValueError, match="size="):
        rle.flatten_instances([])


def test_the_wrapper_refuses_what_is_not_one_image_or_not_a_rank():
    a, b = rle.encode(np.ones((3, 4), np.uint8)), rle.encode(np.ones((4, 3), np.uint8))
    with pytest.raises(ValueError, match="different sizes"):
        rle.flatten_instances([a, b])
    with pytest.raises(ValueError, match="different sizes"):
        rle.flatten_instances([a], size=(4, 3))
    for bad in ([1], [1.5, 2.0], [[1, 2]]):
        with pytest.raises(ValueError, match="rank must be 2 integers"):
            rle.flatten_instances([a, a], rank=bad)
    for bad in ([-1, 0], [0, 2 ** 32]):
        with pytest.raises(ValueError, match="do not fit uint32"):
            rle.flatten_instances([a, a], rank=bad)
    for fn in (analyze.resolve_overlaps, analyze.instances_to_label_image):
        with pytest.raises(ValueError, match="different sizes"):
            fn([a, b], "index", device="cpu")


def _dense(rles):
    return [rle.decode(r).astype(bool) for r in rles]


def check_public_functions(names, device):
    """resolve_overlaps and instances_to_label_image at all four priorities against the dense loop"""
    for name in names:
        c, (h, w) = cs.get(name), cs.size(name)
        masks, n = c["masks"], len(c["masks"])
        rng = np.random.default_rng(len(name))
        scores = np.round(rng.random(n), 1)                          # ties
        areas = masks.sum(axis=(1, 2))
        explicit = rng.integers(-3, 3, n)                            # any integers
        for priority, key, kw in (("score", -scores, dict(scores=scores)), ("area", areas, {}), ("index", np.zeros(n), {}), (explicit, explicit, {})):
            order = np.lexsort((np.arange(n), key))
            labels = np.zeros((h, w), np.int32)
            for i in order[::-1]:
                labels[masks[i]] = i + 1
            got, stats = analyze.resolve_overlaps(masks, priority, size=(h, w), device=device, return_stats=True, **kw)
            assert got == [rle.encode(np.asfortranarray(labels == i + 1)) for i in range(n)], (name, priority)
            assert list(stats) == ["area", "visible_area", "bbox", "pixels"] and all(v.dtype == np.int64 for v in stats.values())
            assert stats["area"].tolist() == areas.tolist() and stats["visible_area"].tolist() == [int((labels == i + 1).sum()) for i in range(n)]
            assert stats["bbox"].shape == (n, 4) and stats["pixels"].shape == (3,) and int(stats["pixels"].sum()) == h * w
            dense = _dense(got)
            assert n == 0 or (np.sum(dense, axis=0) <= 1).all() and (np.any(dense, axis=0) == masks.any(axis=0)).all()          # disjoint, same union
            assert got == analyze.resolve_overlaps(cs.rles(name), priority, size=(h, w), device=device, **kw)
            img = analyze.instances_to_label_image(masks, priority, size=(h, w), device=device, **kw)
            assert img.dtype == np.int32 and img.tobytes() == labels.tobytes(), (name, priority)
            back = analyze.label_image_to_rle(img, "label", device=device)[0]
            assert back == [g for g, v in zip(got, stats["visible_area"]) if v > 0]


PUBLIC = ["full_under", "two_identical", "ring_in_ring_inner_on_top", "empty_first_middle_last", "edges_65x65", "no_mask", "seed_3", "seed_8"]


def test_resolve_overlaps_and_instances_to_label_image():
    check_public_functions(PUBLIC, "cpu")


def test_area_priority_keeps_a_satellite_on_its_particle():
    particle, satellite = np.zeros((20, 20), bool), np.zeros((20, 20), bool)
    particle[2:18, 2:18] = True; satellite[5:8, 5:8] = True
    got, stats = analyze.resolve_overlaps(np.stack([particle, satellite]), "area", device="cpu", return_stats=True)
    assert stats["visible_area"].tolist() == [256 - 9, 9] and stats["pixels"].tolist() == [400 - 256, 256 - 9, 9]
    assert rle.decode(got[1]).astype(bool).tolist() == satellite.tolist()
    assert analyze.resolve_overlaps(np.stack([particle, satellite]), "index", device="cpu", return_stats=True)[1]["visible_area"].tolist() == [256, 0]


def test_instances_instance_sets_and_polygons():
    c = cs.get("full_under")
    rles, n = cs.rles("full_under"), 4
    scores = np.array([0.2, 0.9, 0.9, 0.5])
    want = analyze.resolve_overlaps(rles, "score", scores=scores, device="cpu")
    inst = Instances(image_size=(9, 11), masks=RLEMasks(rles), scores=scores)
    assert analyze.resolve_overlaps(inst, device="cpu") == want                       # the scores field is the default
    iset = InstanceSet()
    iset.instances = inst
    assert analyze.resolve_overlaps(iset, device="cpu") == want
    assert analyze.resolve_overlaps(iset, scores=scores[::-1].copy(), device="cpu") == analyze.resolve_overlaps(rles, "score", scores=scores[::-1].copy(), device="cpu")
    assert analyze.instances_to_label_image(iset, device="cpu").tobytes() == analyze.instances_to_label_image(c["masks"], "score", scores, device="cpu").tobytes()
    import torch
    assert analyze.resolve_overlaps(rles, scores=torch.from_numpy(scores), device="cpu") == want
    bare = Instances(image_size=(9, 11), masks=RLEMasks(rles))
    with pytest.raises(ValueError, match="needs scores"):
        analyze.resolve_overlaps(bare, device="cpu")
    assert analyze.resolve_overlaps(bare, "index", device="cpu") == analyze.resolve_overlaps(rles, "index", device="cpu")
    polys = PolygonMasks([[[1.0, 1.0, 8.0, 1.0, 8.0, 7.0, 1.0, 7.0]], [[4.0, 3.0, 10.0, 3.0, 10.0, 8.5, 4.0, 8.5]]])
    as_rle = analyze.masks_to_rle(polys, (9, 11), device="cpu")
    got = analyze.resolve_overlaps(polys, "index", size=(9, 11), device="cpu")
    assert got == analyze.resolve_overlaps(as_rle, "index", device="cpu") and rle.area(got[1]) < rle.area(as_rle[1]) and got[0]["size"] == [9, 11]
    assert analyze.instances_to_label_image([], "index", size=(4, 6), device="cpu").tolist() == np.zeros((4, 6), int).tolist()
    with pytest.raises(ValueError, match="size="):
        analyze.instances_to_label_image([], "index", device="cpu")


def test_python_surface_refusals(monkeypatch):
    r = cs.rles("full_under")
    for fn in (analyze.resolve_overlaps, analyze.instances_to_label_image):
        for kw, match in ((dict(priority="colour"), "priority = 'colour'"), (dict(priority="index", device="gpu"), "device = 'gpu'"),
                          (dict(priority="score"), "needs scores"), (dict(scores=[0.1, 0.2]), "2 scores for 4 masks"),
                          (dict(scores=[0.1, float("nan"), 0.3, 0.2]), r"scores\[1\] is NaN"), (dict(priority=[0, 1]), "4 integer ranks"),
                          (dict(priority=[0.5, 1, 2, 3]), "4 integer ranks")):
            with pytest.raises(ValueError, match=match):
                fn(r, **dict(dict(device="cpu"), **kw))
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for fn in (analyze.resolve_overlaps, analyze.instances_to_label_image):
        with pytest.raises(AmpError, match="no HIP device"):
            fn(r, "index", device="cuda")
        fn(r, "index", device="auto")                                # 'auto' falls to the host


def check_annotation_round_trip(device):
    """label image -> instances -> label image on one spheroidite annotation: exactly the image back, at every priority (the instances are disjoint)"""
    fg = annotation(ANNOTATIONS[1][0])
    rles, _, areas, _, lab = analyze.label_image_to_rle(fg, "binary", 2, device=device, return_labels=True)
    assert len(rles) == ANNOTATIONS[1][1]
    for priority in ("index", "area"):
        back = analyze.instances_to_label_image(rles, priority, device=device)
        assert back.dtype == np.int32 and back.tobytes() == lab.tobytes()
    got, stats = analyze.resolve_overlaps(rles, "index", device=device, return_stats=True)
    assert got == rles and stats["visible_area"].tolist() == areas.tolist() == stats["area"].tolist()
    assert stats["pixels"].tolist() == [int((~fg).sum()), int(fg.sum()), 0]


def test_spheroidite_annotation_round_trip():
    check_annotation_round_trip("cpu")
