"""amp_render_instances on the host (no GPU needed): the NULL-context path against the dense reference -- the untouched
Visualizer.draw_binary_mask / draw_box, instance by instance (tests/render_cases.py) -- byte for byte on every case, every refusal on a raw call
with the output untouched, analyze.render_instances against Visualizer.overlay_instances, and the Visualizer against the hashes of its output
before it drew through amp_render_instances (tests/golden/render_vectors.json)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import lib
from ampis_amd.utils.visualizer import Visualizer, _palette

import render_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_vectors.json")


@pytest.mark.parametrize("name", rc.HAND)
def test_host_equals_the_dense_reference(name):
    rc.check_case(name)


@pytest.mark.parametrize("chunk", range(8))
def test_host_equals_the_dense_reference_on_seeded_cases(chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        rc.check_case(f"seed_{i}")


def test_the_cases_cover_what_they_should():
    for k in (3, 4):                                                 # order is honoured, not merely tolerated: two orders, two images
        assert rc.expected(f"order_{k}_forward").tobytes() != rc.expected(f"order_{k}_reverse").tobytes()
    assert rc.expected("edge_off").tobytes() != rc.expected("masks_without_boxes").tobytes()
    assert len({rc.expected(f"alpha_{a}").tobytes() for a in (0, 0.3, 0.5, 1)}) == 4
    assert len({rc.expected(f"boxes_lw{lw}").tobytes() for lw in (1, 2, 3)}) == 3
    assert rc.expected("no_instances").tobytes() == rc.get("no_instances")["image"].tobytes()
    h1 = rc.get("size_1x65")
    want = rc.expected("size_1x65")                                  # h == 1: no blended pixel, every mask pixel shows an edge colour
    edges = {tuple(np.clip(c * 255.0 * 0.7, 0, 255).astype(np.uint8).tolist()) for c in h1["colors"]}
    boxes = {tuple(np.clip(c * 255.0, 0, 255).astype(np.uint8).tolist()) for c in h1["colors"]}
    covered = np.logical_or.reduce(h1["masks"])
    assert covered.any() and all(tuple(p.tolist()) in edges | boxes for p in want[covered])
    sizes = [rc.seeded_case(i)["image"].shape[:2] for i in range(rc.N_SEEDED)]
    assert max(max(s) for s in sizes) <= 140 and any(h > 128 for h, _ in sizes) and any(w > 128 for _, w in sizes)
    kinds = {(rc.seeded_case(i)["masks"] is None, rc.seeded_case(i)["boxes"] is None) for i in range(rc.N_SEEDED)}
    assert kinds >= {(False, False), (True, False), (False, True)}
    assert max(len(rc.seeded_case(i)["colors"]) for i in range(rc.N_SEEDED)) == 12


def test_in_place_call_and_repeat():
    c = rc.get("box_crossed_by_next_mask")
    raw = raw_call(c["image"], [rle._counts(rc.enc(m)) for m in c["masks"]], colors=c["colors"], boxes=c["boxes"], lw=c["lw"], in_place=True)
    assert raw[0] == 0 and raw[1].tobytes() == rc.expected("box_crossed_by_next_mask").tobytes()
    assert rc.call("seam_edges").tobytes() == rc.call("seam_edges").tobytes()


def raw_call(image, runs, colors=None, boxes=None, alpha=0.5, edge=True, lw=1, ctx=None, in_place=False, h=None, w=None, n=None, null=()):
    """The C call on uint32 run lists (None: no masks); returns (status, out) with out pre-filled with a mark (the image when in place)."""
    ih, iw = image.shape[:2]
    cnt = len(runs) if runs is not None else (len(boxes) if boxes is not None else 0)
    colors = rc.PALETTE[np.arange(cnt) % len(rc.PALETTE)] if colors is None else colors
    tables, edge_rgb, ibox, box_rgb = analyze.render_inputs(colors, alpha, boxes, ih, iw)
    pool, off, ln = rle._pool([np.asarray(x, np.uint32) for x in runs]) if runs is not None else (None, None, None)
    img = np.ascontiguousarray(image).copy()
    out = img if in_place else np.full(image.shape, 0xAB, np.uint8)
    args = {"image": img, "pool": pool, "off": off, "len": ln, "tab": tables if runs is not None else None,
            "edge": edge_rgb if edge and runs is not None else None, "boxes": ibox, "box_rgb": box_rgb if boxes is not None else None, "out": out}
    a = {k: (None if k in null or v is None else v.ctypes.data_as(C.c_void_p)) for k, v in args.items()}
    st = lib().amp_render_instances(ctx.handle if ctx is not None else None, a["image"], ih if h is None else h, iw if w is None else w, a["pool"],
                                    a["off"], a["len"], cnt if n is None else n, a["tab"], a["edge"], a["boxes"], a["box_rgb"], lw, a["out"])
    return st, out


# (part of the message, arguments) on a 2 x 3 image: every one is AMP_ERR_ARG
HOSTILE = [
    ("the runs of mask 1 cover 5 pixels, the image has 6", dict(runs=[[6], [2, 3]])),                          # a short run list
    ("the runs of mask 0 cover more than the image's 6 pixels", dict(runs=[[1, 6]])),                          # an over-long run list
    ("the runs of mask 0 cover more than the image's 6 pixels", dict(runs=[[0xFFFFFFFF, 7]])),
    ("mask 1 has an empty run list", dict(runs=[[6], []])),
    ("lw = 0", dict(runs=[[0, 6]], lw=0)),
    ("lw = -3", dict(runs=None, boxes=[(0, 0, 1, 1)], lw=-3)),
    ("null image", dict(runs=[[0, 6]], null=("image",))),
    ("null image", dict(runs=[[0, 6]], null=("out",))),
    ("n = -1", dict(runs=[[0, 6]], n=-1)),
    ("null argument", dict(runs=[[0, 6]], null=("len",))),
    ("null argument", dict(runs=[[0, 6]], null=("tab",))),
    ("null argument", dict(runs=None, boxes=[(0, 0, 1, 1)], null=("box_rgb",))),
    ("image size 0 x 3", dict(runs=[[0, 6]], h=0)),
    ("image size 32769 x 32769", dict(runs=[[0, 6]], h=32769, w=32769)),                                         # beyond 2^30 pixels: nothing that large exists
    ("image size 1073741825 x 1", dict(runs=[[0, 6]], h=(1 << 30) + 1, w=1)),
]


def check_hostile(what, kw, ctx=None):
    img = rc.image(2, 3)
    st, out = raw_call(img, kw["runs"], boxes=kw.get("boxes"), lw=kw.get("lw", 1), ctx=ctx, h=kw.get("h"), w=kw.get("w"), n=kw.get("n"),
                       null=kw.get("null", ()))
    assert st == -1 and what in lib().amp_last_error().decode(), (st, lib().amp_last_error())
    assert set(out.reshape(-1).tolist()) == {0xAB}                   # a refused call leaves the output untouched


@pytest.mark.parametrize("what, kw", HOSTILE, ids=[f"{i}-{h[0][:24]}" for i, h in enumerate(HOSTILE)])
def test_hostile_arguments_are_refused_with_their_message(what, kw):
    check_hostile(what, kw)


def check_box_outside_the_image_is_refused(ctx=None):
    """the binding's callers round and clip as draw_box does; the raw call refuses what they would never pass"""
    img = rc.image(2, 3)
    pool, off, ln = rle._pool([np.array([0, 6], np.uint32)])
    tab, rgb, out = np.zeros((1, 256, 3), np.uint8), np.zeros((1, 3), np.uint8), np.full(img.shape, 0xAB, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for box in ((0, 0, 3, 1), (-1, 0, 1, 1), (0, 2, 1, 1), (0, 0, 1, -1)):
        b = np.array([box], np.int32)
        st = lib().amp_render_instances(ctx.handle if ctx is not None else None, vp(img), 2, 3, vp(pool), vp(off), vp(ln), 1, vp(tab), vp(rgb),
                                        vp(b), vp(rgb), 1, vp(out))
        assert st == -1 and "outside the 2 x 3 image" in lib().amp_last_error().decode() and set(out.reshape(-1).tolist()) == {0xAB}


def test_box_outside_the_image_is_refused():
    check_box_outside_the_image_is_refused()


def test_the_limit_is_two_to_the_thirty_pixels():
    """32768 x 32768 = 2^30 pixels is inside the limit: the call gets as far as the runs, which cover 6 pixels"""
    st, out = raw_call(rc.image(2, 3), [[0, 6]], h=32768, w=32768)
    assert st == -1 and "cover 6 pixels, the image has 1073741824" in lib().amp_last_error().decode()
    assert set(out.reshape(-1).tolist()) == {0xAB}


def test_layout_of_the_raw_call():
    """2 x 3 image, pixels 0 .. 5 column-major.  Mask = pixels 1 .. 3: (1, 0), (0, 1), (1, 1); every pixel of a 2-row image is an edge pixel"""
    img = rc.image(2, 3)
    col = np.array([[0.2, 0.4, 1.0]])
    st, out = raw_call(img, [[1, 3, 2]], colors=col, edge=False)
    assert st == 0, lib().amp_last_error()
    m = np.array([[0, 1, 0], [1, 1, 0]], bool)
    want = img.copy()
    want[m] = (img[m].astype(np.float64) * 0.5 + col[0] * 255.0 * 0.5 + 0.5).astype(np.uint8)
    assert out.tobytes() == want.tobytes()
    st, out = raw_call(img, [[1, 3, 2]], colors=col)
    want[m] = np.array([35, 71, 178], np.uint8)                      # uint8(255 * colour * 0.7)
    assert st == 0 and out.tobytes() == want.tobytes()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------------

def overlay_inputs():
    h, w = 70, 90
    masks = [rc.disc(h, w, 30, 30, 18), rc.disc(h, w, 36, 48, 22, 15), rc.rect(h, w, 5, 40, 50, 85), np.zeros((h, w), bool)]
    polys = [[[10.0, 10.0, 60.5, 12.0, 55.0, 60.0, 12.5, 50.0]], [[40.0, 5.0, 88.0, 8.0, 70.0, 66.0], [5.0, 40.0, 30.0, 42.0, 20.0, 68.0]]]
    boxes = np.array([[12, 12, 48, 48], [33, 14, 63, 58], [50, 5, 84, 39], [-4.5, 20.5, 30.5, 90.0]])
    return rc.image(h, w, 3), masks, polys, boxes


def overlay(img, scale=1, **kw):
    return Visualizer(img, None, scale=scale).overlay_instances(**kw).get_image()


def dense_overlay(img, masks, boxes, colors, alpha=0.5):
    """overlay_instances restated on the primitives: what it was before the one call"""
    vis = Visualizer(img)
    order = np.argsort(-np.prod(boxes[:, 2:] - boxes[:, :2], axis=1)) if boxes is not None else np.arange(len(masks))
    for i in order:
        if masks is not None:
            vis.draw_binary_mask(masks[i], colors[i], alpha=alpha)
        if boxes is not None:
            vis.draw_box(boxes[i], colors[i])
    return vis.output.img


@pytest.mark.parametrize("form", ["rle", "bool", "polygons"])
@pytest.mark.parametrize("with_boxes", [True, False])
def test_render_instances_equals_overlay_instances(form, with_boxes):
    img, masks, polys, boxes = overlay_inputs()
    if form == "polygons":
        given = polys
        dense = [rle.decode(rle.merge(rle.frPyObjects(p, 70, 90))).astype(bool) for p in polys]
        from ampis_amd.structures import PolygonMasks
        for_analyze = PolygonMasks(polys)
    else:
        given = [rc.enc(m) for m in masks] if form == "rle" else np.stack(masks)
        dense, for_analyze = masks, given
    n = len(dense)
    bx = boxes[:n] if with_boxes else None
    cols = rc.PALETTE[2:2 + n]
    want = dense_overlay(img, dense, bx, cols, alpha=0.3)
    got = overlay(img, masks=given, boxes=bx, assigned_colors=cols, alpha=0.3)
    assert got.tobytes() == want.tobytes()
    drawn = analyze.render_instances(img, for_analyze, bx, cols, alpha=0.3, device="cpu")
    assert drawn.dtype == np.uint8 and drawn.tobytes() == want.tobytes()
    assert (want != img).any()


def test_render_instances_arguments():
    img, masks, _, boxes = overlay_inputs()
    rles = [rc.enc(m) for m in masks]
    base = analyze.render_instances(img, rles, boxes, device="cpu")                                  # the palette, the Visualizer's order
    assert base.tobytes() == overlay(img, masks=rles, boxes=boxes).tobytes()
    rev = analyze.render_instances(img, rles, boxes, order=[3, 2, 1, 0], device="cpu")
    assert rev.tobytes() != base.tobytes()
    thick = analyze.render_instances(img, None, boxes, line_width=4, device="cpu")
    vis = Visualizer(img)
    for i in analyze.render_order(boxes, 4):
        vis.draw_box(boxes[i], _palette(4)[i], line_width=4)
    assert thick.tobytes() == vis.output.img.tobytes()
    assert analyze.render_instances(img, [], device="cpu").tobytes() == img.tobytes()
    grey = analyze.render_instances(img[:, :, 0], rles, device="cpu")
    assert grey.tobytes() == overlay(img[:, :, 0], masks=rles).tobytes()
    with pytest.raises(ValueError, match="alpha"):
        analyze.render_instances(img, rles, alpha=1.5, device="cpu")
    with pytest.raises(ValueError, match="colours"):
        analyze.render_instances(img, rles, colors=np.full((4, 3), 1.5), device="cpu")
    with pytest.raises(ValueError, match="size"):
        analyze.render_instances(img, [rc.enc(np.ones((5, 5), bool))], device="cpu")
    with pytest.raises(ValueError, match="device"):
        analyze.render_instances(img, rles, device="tpu")


def test_the_visualizer_falls_back_to_the_primitives():
    img, masks, _, boxes = overlay_inputs()
    rles = [rc.enc(m) for m in masks]
    cols = rc.PALETTE[:4]
    # scale = 2: the masks are resampled, the primitives draw
    vis = Visualizer(img, scale=2)
    want = Visualizer(img, scale=2)
    for i in analyze.render_order(boxes, 4):
        want.draw_binary_mask(masks[i], cols[i], alpha=0.5)
        want.draw_box(boxes[i], cols[i])
    assert vis.overlay_instances(masks=rles, boxes=boxes, assigned_colors=cols).get_image().tobytes() == want.output.img.tobytes()
    assert want.output.img.shape == (140, 180, 3)
    # a colour of 1.5: the blend leaves the table's range, the primitives draw (uint8 wrap-around and all)
    hot = cols.copy()
    hot[1] = (1.5, 0.2, 0.2)
    with np.errstate(invalid="ignore"):
        got = overlay(img, masks=rles, boxes=boxes, assigned_colors=hot)
        assert got.tobytes() == dense_overlay(img, masks, boxes, hot).tobytes()
    # alpha beyond 1 likewise
    with np.errstate(invalid="ignore"):
        assert overlay(img, masks=rles, assigned_colors=cols, alpha=1.25).tobytes() == dense_overlay(img, masks, None, cols, alpha=1.25).tobytes()
    # uint8 masks are not bool arrays: drawn by the primitives, the same picture
    assert overlay(img, masks=np.stack(masks).astype(np.uint8), assigned_colors=cols).tobytes() == dense_overlay(img, masks, None, cols).tobytes()
    # an RLE of another size: the primitives resample it to the image (Visualizer._to_out), as before; a bool array of another size likewise
    small = np.zeros((35, 45), bool)
    small[5:30, 10:40] = True
    want = Visualizer(img)
    want.draw_binary_mask(small, cols[0])
    assert overlay(img, masks=[rc.enc(small)], assigned_colors=cols[:1]).tobytes() == want.output.img.tobytes()
    assert overlay(img, masks=small[None], assigned_colors=cols[:1]).tobytes() == want.output.img.tobytes()
    assert (want.output.img != img).any()
    # a mask the primitives cannot draw raises what it raised: a 3-D array per instance
    for bad in (np.ones((1, 2, 70, 90), bool),):
        with pytest.raises(IndexError) as a:
            overlay(img, masks=bad)
        with pytest.raises(IndexError) as b:
            Visualizer(img).draw_binary_mask(bad[0], (1.0, 0.0, 0.0))
        assert str(a.value) == str(b.value)


def test_the_visualizer_draws_what_it_drew_before():
    """every image of golden_renders against the hashes made before overlay_instances went through amp_render_instances: the one call, the
    fallbacks and the labels of one PIL session change no byte"""
    with open(GOLDEN) as f:
        want = json.load(f)["images"]
    got = rc.golden_renders()
    assert sorted(got) == sorted(want)
    for name, img in got.items():
        assert list(img.shape) == want[name]["shape"], name
        assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == want[name]["sha256"], name
    assert any("labels" in k for k in want)
