"""amp_mask_morphology on the host (no GPU needed): the NULL-context path against scipy on one decoded mask (tests/morphology_ref.py) on every
case of tests/morphology_cases.py -- three shapes, the case's radii, both border values, all six ops --, byte for byte with boxes and areas;
the set identities of the definition through rle.merge / rle.pair_overlap; the capacity protocol and every refusal through the raw C call
with sentinel words behind the buffers; boundary_iou against its dense restatement, near_pairs against brute-force pixel distances; the
Python surface: rle.morphology, analyze.dilate_masks / erode_masks / open_masks / close_masks / boundary_bands / boundary_iou / near_pairs."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

from ampis_amd import analyze, rle
from ampis_amd._lib import lib

import morphology_cases as cs

N_CHUNKS = 20
PER_CHUNK = cs.N_SEEDED // N_CHUNKS


@pytest.mark.parametrize("name", cs.HAND)
def test_host_equals_the_reference(name):
    for shape, r, b in cs.combos(name):
        cs.check_case(name, shape, r, b)


@pytest.mark.parametrize("shape", cs.SHAPES)
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_host_equals_the_reference_on_seeded_cases(chunk, shape):
    for name in cs.SEEDED[chunk * PER_CHUNK: (chunk + 1) * PER_CHUNK]:
        for r in cs.RADII:
            for b in cs.BORDERS:
                cs.check_case(name, shape, r, b)


def check_largest(name, ctx=None):
    """the closed forms: a rectangle dilated by a square, eroded by a disk"""
    ins, sz = cs.largest_inputs(name), cs.LARGEST[name][0]
    out = []
    for r in cs.LARGEST_RADII:
        for b in cs.BORDERS:
            for op, shape in (("dilate", "square"), ("erode", "disk")):
                res = rle.morphology(ins, op, shape, r, b, ctx=ctx, size=sz, return_stats=True)
                cs.equal_to(res, cs.largest_expected(name, op, r, b), (name, op, r, b))
                out.append(cs.result_bytes(res))
    return out


@pytest.mark.parametrize("name", list(cs.LARGEST))
def test_the_largest_sides(name):
    check_largest(name)


def _dense(rles):
    return [rle.decode(r).astype(bool) for r in rles]


def test_the_cases_are_what_their_names_say():
    sizes = [cs.get(s)["masks"].shape for s in cs.SEEDED]
    assert max(s[1] for s in sizes) == 40 and max(s[2] for s in sizes) == 40 and {s[0] for s in sizes} == set(range(1, 7))
    assert len(cs.get("pool_of_0")["masks"]) == 0 and cs.run("pool_of_0", "dilate", "disk", 2, 0)[0] == []
    assert any(0 in rle._counts(r)[1:-1].tolist() for r in cs.rles("zero_length_runs"))
    assert len(rle.string_to_counts(cs.rles("runs_joined_across_column_ends")[0]["counts"])) == 3       # one run over three columns
    # the bridge: an opening cuts it, a closing of the crack fills it
    bridge = cs.rles("bridge")
    assert analyze.mask_topology(list(bridge), device="cpu")["n_parts"].tolist() == [1]
    opened = analyze.open_masks(list(bridge), "square", 1, device="cpu")
    assert analyze.mask_topology(opened, device="cpu")["n_parts"].tolist() == [2]
    want = cs.get("bridge")["masks"][0].copy(); want[4, 6:9] = False
    assert (_dense(opened)[0] == want).all()
    closed = analyze.close_masks(list(cs.rles("crack")), "square", 1, device="cpu")
    full = cs.get("crack")["masks"][0].copy(); full[2:9, 7] = True
    assert (_dense(closed)[0] == full).all() and analyze.mask_topology(list(cs.rles("crack")), device="cpu")["n_parts"].tolist() == [2]
    # two pieces of a column 2 hh rows apart merge under a dilation, 2 hh + 1 apart they do not; a piece of 2 hh rows vanishes under an
    # erosion, one of 2 hh + 1 rows survives as one row
    for name, lo in (("a", (1, 2, 3, 4, 5)), ("b", (6, 7, 14, 15, 16))):
        for hh in (1, 2, 3, 7):
            grown = _dense(cs.run(f"two_pieces_in_a_column_{name}", "dilate", "square", hh, 0)[0])
            assert [int(ndimage.label(g[:, 2])[1]) for g in grown] == [1 if g <= 2 * hh else 2 for g in lo]
            left = cs.run(f"pieces_of_length_{name}", "erode", "square", hh, 0)
            assert [int(d.any(axis=1).sum()) for d in _dense(left[0])] == [max(k - 2 * hh, 0) for k in lo]
    # every pixel of a checkerboard is its own 4-connected part: the diamond joins them, the inner band is the mask
    board = cs.run("checkerboard_7x7", "band_in", "diamond", 1, 0)
    assert [bytes(x["counts"]) for x in board[0]] == [bytes(r["counts"]) for r in cs.rles("checkerboard_7x7")]
    assert all(d.all() for d in _dense(cs.run("checkerboard_7x7", "dilate", "diamond", 1, 0)[0]))


def complement(r):
    c = rle._counts(r)
    c = c[1:] if c[0] == 0 and len(c) > 1 else np.concatenate([np.zeros(1, np.uint32), c])
    return {"size": list(r["size"]), "counts": rle.counts_to_string(c)}


def _strings(rles):
    return [bytes(r["counts"]) for r in rles]


@pytest.mark.parametrize("chunk", range(4))
def test_set_identities_hold_exactly(chunk):
    for name in cs.SEEDED[chunk * 10: chunk * 10 + 10] + (cs.HAND[2:8] if chunk == 0 else ()):
        masks = list(cs.rles(name))
        n, sz = len(masks), cs.size(name)
        same = np.stack([np.arange(n), np.arange(n)], axis=1)
        canon = rle.morphology(masks, "dilate", "square", 0, size=sz)                    # radius 0: the canonical form of the input
        assert _strings(canon) == _strings([rle.encode(np.asfortranarray(m)) for m in cs.get(name)["masks"]])
        for shape in cs.SHAPES:
            for r in (1, 2, 7):
                where = (name, shape, r)
                d = rle.morphology(masks, "dilate", shape, r, size=sz)
                # duality: eroding with the outside as mask is dilating the complement
                e1 = rle.morphology(masks, "erode", shape, r, 1, size=sz)
                assert _strings(e1) == _strings([complement(x) for x in rle.morphology([complement(m) for m in canon], "dilate", shape, r, size=sz)]), where
                for b in cs.BORDERS:
                    e = rle.morphology(masks, "erode", shape, r, b, size=sz)
                    bi = rle.morphology(masks, "band_in", shape, r, b, size=sz)
                    assert rle.pair_overlap(e, canon, same)[1].tolist() == [0] * n and rle.pair_overlap(canon, d, same)[1].tolist() == [0] * n, where    # erode in M in dilate
                    assert rle.pair_overlap(bi, e, same)[0].tolist() == [0] * n, where  # the inner band and the erosion partition M
                    assert _strings([rle.merge([x, y]) for x, y in zip(bi, e)]) == _strings(canon), where
                    for op in ("open", "close"):                                         # idempotent
                        once = rle.morphology(masks, op, shape, r, b, size=sz)
                        assert _strings(rle.morphology(once, op, shape, r, b, size=sz)) == _strings(once), where + (op, b)
                    assert rle.pair_overlap(rle.morphology(masks, "open", shape, r, b, size=sz), canon, same)[1].tolist() == [0] * n, where           # anti-extensive
                bo = rle.morphology(masks, "band_out", shape, r, size=sz)
                assert rle.pair_overlap(bo, canon, same)[0].tolist() == [0] * n, where  # the outer band and M partition the dilation
                assert _strings([rle.merge([x, y]) for x, y in zip(bo, canon)]) == _strings(d), where
                assert rle.pair_overlap(canon, rle.morphology(masks, "close", shape, r, 1, size=sz), same)[1].tolist() == [0] * n, where              # extensive with border_value 1


# ---- the raw C call: capacities and refusals ------------------------------------------------------------------------------------------------------

SENTINEL = 0xA5A5A5A5
TAIL = 8


def raw_call(counts_list, h, w, op=0, shape=2, radius=1, border_value=0, out_cap=64, ctx=None, n=None, null=()):
    """the call on buffers with TAIL sentinel words behind what the call may write; (status, buffers)"""
    k = len(counts_list)
    n = k if n is None else n
    pool, off, ln = rle._pool([np.asarray(c, np.uint32) for c in counts_list])
    m = max(k, 1)
    buf = {"out_pool": np.full(out_cap + TAIL, SENTINEL, np.uint32), "out_off": np.full(m + TAIL, SENTINEL, np.uint64),
           "out_len": np.full(m + TAIL, 0x5A5A5A5A, np.int32), "boxes": np.full(4 * m + TAIL, SENTINEL, np.int64),
           "areas": np.full(m + TAIL, SENTINEL, np.uint64), "need": np.full(1 + TAIL, SENTINEL, np.uint64)}
    ins = {"pool": pool, "off": off, "len": ln}
    p = lambda name: None if name in null else (ins[name] if name in ins else buf[name]).ctypes.data_as(C.c_void_p)
    st = lib().amp_mask_morphology(ctx.handle if ctx is not None else None, p("pool"), p("off"), p("len"), n, h, w, op, shape, radius, border_value,
                                   p("out_pool"), out_cap, p("out_off"), p("out_len"), p("boxes"), p("areas"), p("need"))
    return st, buf


def untouched(buf, but=()):
    return all(set(a.tolist()) <= {SENTINEL, 0x5A5A5A5A} for name, a in buf.items() if name not in but)


def check_capacity_protocol(ctx=None, name="seed_7", op="open", shape="disk", radius=2):
    counts = [rle._counts(r) for r in cs.rles(name)]
    (h, w), n = cs.size(name), len(counts)
    args = dict(op=rle.MORPH_OPS[op], shape=rle.MORPH_SHAPES[shape], radius=radius, border_value=0, ctx=ctx)
    st, buf = raw_call(counts, h, w, out_cap=0, **args)
    need = int(buf["need"][0])
    assert st == -3 and need >= n and "counts are needed" in lib().amp_last_error().decode() and untouched(buf, but=("need",))
    st, short = raw_call(counts, h, w, out_cap=need - 1, **args)     # one word short: refused, the need again, nothing else written
    assert st == -3 and int(short["need"][0]) == need and untouched(short, but=("need",))
    st, buf = raw_call(counts, h, w, out_cap=need, **args)           # exactly the need
    assert st == 0 and int(buf["need"][0]) == need
    assert set(buf["out_pool"][need:].tolist()) == {SENTINEL} and set(buf["out_off"][n:].tolist()) == {SENTINEL}      # the words behind the result
    assert set(buf["out_len"][n:].tolist()) == {0x5A5A5A5A} and set(buf["boxes"][4 * n:].tolist()) == {SENTINEL}
    assert set(buf["areas"][n:].tolist()) == {SENTINEL} and set(buf["need"][1:].tolist()) == {SENTINEL}
    assert int(buf["out_len"][:n].sum()) == need and buf["out_off"][:n].tolist() == np.concatenate([[0], np.cumsum(buf["out_len"][:n - 1])]).tolist()
    want = cs.expected(name, shape, radius, 0)[op]
    got = rle.counts_to_strings(buf["out_pool"][:need], buf["out_off"][:n], buf["out_len"][:n])
    assert got == [bytes(c) for c in want[0]] and buf["boxes"][:4 * n].reshape(n, 4).tolist() == want[1].tolist()
    assert buf["areas"][:n].tolist() == want[2].tolist()
    return buf


def test_capacity_protocol_on_the_host():
    check_capacity_protocol()
    check_capacity_protocol(name="checkerboard_7x7", op="band_out", shape="diamond", radius=1)


GOOD = [[2, 3, 1]]                                                   # a 2 x 3 image
REFUSALS = [
    ("n = -1", dict(n=-1)),
    ("image size 0 x 3", dict(h=0, w=3)),
    ("image size 2 x -7", dict(h=2, w=-7)),
    ("image size 32769 x 2", dict(h=32769, w=2)),
    ("image size 1 x 32769", dict(h=1, w=32769)),
    ("image size 32768 x 32769", dict(h=32768, w=32769)),
    ("op = -1", dict(op=-1)),
    ("op = 6", dict(op=6)),
    ("shape = -1", dict(shape=-1)),
    ("shape = 3", dict(shape=3)),
    ("border_value = 2", dict(border_value=2)),
    ("border_value = -1", dict(border_value=-1)),
    ("radius = -1", dict(radius=-1)),
    ("radius = 1025", dict(radius=1025)),
    ("null argument pool", dict(null=("pool",))),
    ("null argument off", dict(null=("off",))),
    ("null argument len", dict(null=("len",))),
    ("null argument out_pool", dict(null=("out_pool",))),
    ("null argument out_off", dict(null=("out_off",))),
    ("null argument out_len", dict(null=("out_len",))),
    ("null argument boxes", dict(null=("boxes",))),
    ("null argument areas", dict(null=("areas",))),
    ("null argument need", dict(null=("need",))),
    ("null argument need", dict(null=("need",), counts_list=[], n=0)),
    ("mask 0 has an empty run list", dict(counts_list=[[]])),
    ("the runs of mask 1 cover more than the image's 6 pixels", dict(counts_list=[[6], [2, 3, 2]])),
    ("the runs of mask 1 cover 5 pixels, the image has 6", dict(counts_list=[[0, 6], [2, 3]])),
    ("the runs of mask 0 cover 6 pixels, the image has 8", dict(h=2, w=4)),      # a run list of another image size
    # 2^31 events: 512 x 4096 pixels as 2^20 pieces of one pixel, up to 2049 offsets each, two events an offset
    ("2^31 events or more by mask 0 (2 x the output columns inside the image of every piece, at most 2^31 - 1)",
     dict(counts_list=[[1] * (1 << 21)], h=512, w=4096, radius=1024)),
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


def test_no_mask_empty_and_full_masks_are_valid_calls():
    st, buf = raw_call([], 3, 5, n=0, null=("pool", "off", "len", "out_pool", "out_off", "out_len", "boxes", "areas"), out_cap=0)
    assert st == 0 and int(buf["need"][0]) == 0 and untouched(buf, but=("need",))
    for op in range(6):
        st, buf = raw_call([[15], [0, 15]], 3, 5, op=op, radius=2, border_value=1, out_cap=4)
        full = op in (0, 1, 2, 3)                                    # a full mask stays full when the outside counts as mask; its bands are empty
        assert st == 0 and buf["out_pool"][:int(buf["need"][0])].tolist() == ([15, 0, 15] if full else [15, 15]), op
        assert buf["areas"][:2].tolist() == [0, 15 if full else 0] and buf["boxes"][:8].tolist() == [0, 0, 0, 0] + ([0, 0, 3, 5] if full else [0, 0, 0, 0])
    assert rle.morphology([], "erode", size=(3, 5)) == [] and rle.morphology([], "erode") == []
    out, boxes, areas = rle.morphology([], "erode", return_stats=True)
    assert out == [] and boxes.shape == (0, 4) and areas.shape == (0,)
    with pytest.raises(ValueError, match="masks of different sizes"):
        rle.morphology([{"size": [2, 3], "counts": np.array([6], np.uint32)}, {"size": [3, 2], "counts": np.array([6], np.uint32)}], "dilate")
    for kw in (dict(op="grow"), dict(op="dilate", shape="ball"), dict(op="dilate", radius=-1), dict(op="dilate", radius=1025), dict(op="dilate", radius=1.5),
               dict(op="dilate", border_value=2), dict(op="dilate", radius=True)):
        with pytest.raises(ValueError, match="morphology: "):
            rle.morphology(list(cs.rles("full")), **kw)


# ---- Boundary IoU and the near pairs --------------------------------------------------------------------------------------------------------------

def dense_boundary_iou(g, p, d):
    """the published computation on two decoded masks: cv2.erode with the 3 x 3 element, iterations = d, on a mask padded with a ring of zeros"""
    ones = np.ones((3, 3), bool)
    bg = g & ~ndimage.binary_erosion(g, structure=ones, iterations=d, border_value=0)
    bp = p & ~ndimage.binary_erosion(p, structure=ones, iterations=d, border_value=0)
    return int((bg & bp).sum()), int((bg | bp).sum())


def _pair_pool(seed, n=5):
    """n ground-truth blobs and a prediction for each: the blob shifted, grown or shrunk a little"""
    rng = np.random.RandomState(4200 + seed)
    h, w = int(rng.randint(12, 41)), int(rng.randint(12, 41))
    gt, pred = np.zeros((n, h, w), bool), np.zeros((n, h, w), bool)
    yy, xx = np.mgrid[:h, :w]
    for i in range(n):
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, h / 2), rng.uniform(2, w / 2)
        gt[i] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        dy, dx, s = rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.8, 1.2)
        pred[i] = ((yy - cy - dy) / (ry * s)) ** 2 + ((xx - cx - dx) / (rx * s)) ** 2 <= 1
    return gt, pred


def check_boundary_iou(device):
    pools = [(_pair_pool(s), None) for s in range(10)]                                   # 50 seeded pairs
    hand = np.stack([np.zeros((9, 11), bool), np.ones((9, 11), bool), cs.get("touching_all_four_borders")["masks"][0], cs.get("touching_all_four_borders")["masks"][1]])
    pools.append(((hand, hand[[1, 1, 3, 2]]), 1))                                        # empty against full: 0; full against full; the frame and the cross
    pools.append(((np.zeros((2, 6, 7), bool), np.zeros((2, 6, 7), bool)), 2))           # both bands empty: NaN
    for (gt, pred), dist in pools:
        n = len(gt)
        pairs = np.stack([np.arange(n), np.arange(n)], axis=1)
        for d in ((dist,) if dist else (None, 1, 2, 5)):
            res = analyze.boundary_iou(gt, pred, matches=pairs, distance=d, device=device)
            dd = d if d else max(1, int(round(0.02 * np.sqrt(gt.shape[1] ** 2 + gt.shape[2] ** 2))))
            want = [dense_boundary_iou(g, p, dd) for g, p in zip(gt, pred)]
            assert res["distance"] == dd and res["inter"].dtype == np.int64 and res["union"].dtype == np.int64 and res["boundary_iou"].dtype == np.float64
            assert res["inter"].tolist() == [x[0] for x in want] and res["union"].tolist() == [x[1] for x in want]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.asarray([x[0] for x in want], np.float64) / np.asarray([x[1] for x in want], np.float64)
            assert res["boundary_iou"].tobytes() == ratio.tobytes() and np.isnan(res["boundary_iou"]).tolist() == [x[1] == 0 for x in want]
    gt, pred = _pair_pool(3)
    auto = analyze.boundary_iou(gt, pred, device=device)             # matches=None: the true positives at 0.5
    m = analyze.rle_instance_matcher(gt, pred, device=device)
    given = analyze.boundary_iou(list(analyze.masks_to_rle(gt)), list(analyze.masks_to_rle(pred)), matches=m, dilation_ratio=0.02, device=device)
    assert len(m["tp"]) > 0 and auto["boundary_iou"].tobytes() == given["boundary_iou"].tobytes() and len(auto["inter"]) == len(m["tp"])
    none = analyze.boundary_iou(gt, pred, matches=np.zeros((0, 2), int), device=device)
    assert len(none["boundary_iou"]) == 0 and none["distance"] == 1


def test_boundary_iou_equals_its_dense_restatement():
    check_boundary_iou("cpu")
    gt, pred = _pair_pool(1)
    for kw, what in ((dict(distance=0), "distance"), (dict(distance=1025), "distance"), (dict(distance=1.5), "distance"), (dict(dilation_ratio=-1), "dilation_ratio"),
                     (dict(device="gpu"), "device"), (dict(matches=[[0, 9]]), "pair 0"), (dict(dilation_ratio=40.0), "exceeds 1024")):
        with pytest.raises(ValueError, match=what):
            analyze.boundary_iou(gt, pred, **kw)
    with pytest.raises(ValueError, match="masks of different sizes"):
        analyze.boundary_iou(gt, pred[:, :-1], device="cpu")


def brute_near_pairs(masks, gap, shape):
    pts = [np.argwhere(m) for m in masks]
    out = []
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            if len(pts[i]) == 0 or len(pts[j]) == 0:
                continue
            d = np.abs(pts[i][:, None, :] - pts[j][None, :, :])
            dist = d.max(axis=2) if shape == "square" else d.sum(axis=2) if shape == "diamond" else (d ** 2).sum(axis=2)
            if dist.min() <= (gap * gap if shape == "disk" else gap):
                out.append([i, j])
    return np.asarray(out, np.int64).reshape(-1, 2)


def check_near_pairs(device):
    found = 0
    for seed in range(6):
        rng = np.random.RandomState(7700 + seed)
        h, w, n = int(rng.randint(10, 31)), int(rng.randint(10, 31)), 7
        masks = np.zeros((n, h, w), bool)
        for i in range(n - 1):                                       # small rectangles scattered over the image; the last mask stays empty
            r0, c0 = int(rng.randint(0, h - 3)), int(rng.randint(0, w - 3))
            masks[i, r0: r0 + int(rng.randint(1, 5)), c0: c0 + int(rng.randint(1, 5))] = True
        for shape in cs.SHAPES:
            for gap in (0, 1, 2, 5):
                got = analyze.near_pairs(masks, gap, shape, device=device)
                want = brute_near_pairs(masks, gap, shape)
                assert got.dtype == np.int64 and got.tolist() == want.tolist(), (seed, shape, gap)
                found += len(want)
                grown = analyze.dilate_masks(masks, shape, gap, device=device)
                meets = analyze.overlap_matrix(grown, masks, device=device) > 0
                assert (meets == meets.T).all(), (seed, shape, gap)                      # symmetric by the distance, not by construction of the result
    assert found > 50
    assert analyze.near_pairs(masks[:1], 3, device=device).shape == (0, 2) and analyze.near_pairs([], 3, size=(4, 4), device=device).shape == (0, 2)


def test_near_pairs_equal_the_brute_force_pixel_distances():
    check_near_pairs("cpu")
    touching = np.zeros((2, 4, 4), bool); touching[0, 0, 0] = True; touching[1, 1, 1] = True          # diagonal neighbours: 8-touching, not 4-touching
    assert analyze.near_pairs(touching, 1, "square", device="cpu").tolist() == [[0, 1]] and len(analyze.near_pairs(touching, 1, "diamond", device="cpu")) == 0
    assert len(analyze.near_pairs(touching, 1, "disk", device="cpu")) == 0 and analyze.near_pairs(touching, 2, "disk", device="cpu").tolist() == [[0, 1]]


# ---- the public functions -------------------------------------------------------------------------------------------------------------------------

PUBLIC = ["touching_all_four_borders", "bridge", "empty", "pool_of_0", "zero_length_runs", "seed_3", "seed_10", "seed_11"]


def public_results(name, device, shape="disk", radius=2):
    masks = list(cs.rles(name))
    kw = dict(shape=shape, radius=radius, size=cs.size(name), device=device, return_stats=True)
    return {"dilate": analyze.dilate_masks(masks, **kw), "erode": analyze.erode_masks(masks, **kw), "open": analyze.open_masks(masks, **kw),
            "close": analyze.close_masks(masks, **kw), "erode1": analyze.erode_masks(masks, border_value=1, **kw),
            "band_in": analyze.boundary_bands(masks, radius, "inner", shape, size=cs.size(name), device=device, return_stats=True),
            "band_out": analyze.boundary_bands(masks, radius, "outer", shape, size=cs.size(name), device=device, return_stats=True)}


def public_bytes(res):
    return {k: ([bytes(x["counts"]) for x in out], st["area"].tobytes(), st["bbox"].tobytes()) for k, (out, st) in res.items()}


def check_public_functions(names, device):
    for name in names:
        for shape, radius in (("disk", 2), ("square", 1), ("diamond", 3)):
            res = public_results(name, device, shape, radius)
            for key, (out, st) in res.items():
                op, b = ("erode", 1) if key == "erode1" else (key, 1 if key == "close" else 0)      # close_masks defaults to border_value 1
                want = cs.expected(name, shape, radius, b)[op]
                cs.equal_to((out, st["bbox"], st["area"]), want, (name, key, shape, radius))


def test_the_public_functions_on_the_host():
    check_public_functions(PUBLIC, "cpu")
    masks = cs.get("seed_3")["masks"]
    plain = analyze.dilate_masks(masks, "square", 2, device="cpu")   # without return_stats: the list alone; a bool array is accepted
    assert [bytes(x["counts"]) for x in plain] == [bytes(c) for c in cs.expected("seed_3", "square", 2, 0)["dilate"][0]]
    edge = np.zeros((1, 6, 6), bool); edge[0, 0:3, 0:3] = True       # a closing is extensive at the image's border by default, not with border_value 0
    assert (_dense(analyze.close_masks(edge, "square", 2, device="cpu"))[0] >= edge[0]).all()
    assert not (_dense(analyze.close_masks(edge, "square", 2, border_value=0, device="cpu"))[0] >= edge[0]).all()
    for fn in (analyze.dilate_masks, analyze.erode_masks, analyze.open_masks, analyze.close_masks):
        for kw, what in ((dict(shape="ball"), "shape"), (dict(radius=-1), "radius"), (dict(radius=1025), "radius"), (dict(radius=2.0), "radius"),
                         (dict(border_value=2), "border_value"), (dict(device="gpu"), "device")):
            with pytest.raises(ValueError, match=f"{fn.__name__}: {what}"):
                fn(masks, **kw)
        with pytest.raises(ValueError, match="masks of different sizes"):
            fn([cs.rles("seed_3")[0], cs.rles("seed_10")[0]], device="cpu")
    with pytest.raises(ValueError, match="side"):
        analyze.boundary_bands(masks, 1, side="both")
    with pytest.raises(ValueError, match="boundary_bands: radius"):
        analyze.boundary_bands(masks, -2)
    with pytest.raises(ValueError, match="near_pairs: radius"):
        analyze.near_pairs(masks, gap=-1)
