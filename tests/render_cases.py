"""The case set of amp_render_instances, shared by tests/test_render.py (host path), tests/test_render_gpu.py (device path) and, as shapes, by
the sanitizer run.  A case is {image: uint8 [h, w, 3], masks: list of bool [h, w] in draw order or None, boxes: list of XYXY floats as a caller
of draw_box passes them or None, colors: [n, 3] in [0, 1], alpha, edge, lw}.  The expected image is the DENSE REFERENCE: a loop over the
decoded masks calling the untouched Visualizer.draw_binary_mask / draw_box on a Visualizer of the case's image, computed once per process.
The smallest shapes at which the word building, the edge rule or the replay can go wrong: see the comment of each case."""
import functools

import numpy as np

from ampis_amd import analyze, rle
from ampis_amd.utils.visualizer import Visualizer

SIZES = (1, 2, 63, 64, 65, 130)                   # word and tile seams; 1: every mask pixel is an edge pixel


def enc(m):
    return rle.encode(np.asfortranarray(np.asarray(m).astype(np.uint8)))


def image(h, w, seed=0):
    """a reproducible image in which neighbouring pixels and channels differ"""
    yy, xx = np.mgrid[:h, :w]
    return np.stack([(yy * 7 + xx * 13 + seed * 31) % 256, (yy * 11 + xx * 3 + 97 + seed) % 256, (yy * yy + xx * 5 + seed * 7) % 256], axis=2).astype(np.uint8)


def rect(h, w, r0, r1, c0, c1):
    m = np.zeros((h, w), bool)
    m[max(r0, 0):r1, max(c0, 0):c1] = True
    return m


def disc(h, w, cy, cx, ry, rx=None):
    yy, xx = np.ogrid[:h, :w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / (rx or ry)) ** 2 <= 1.0


def pixels(h, w, pts):
    m = np.zeros((h, w), bool)
    for r, c in pts:
        m[r, c] = True
    return m


PALETTE = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.2, 0.4, 1.0], [1.0, 0.85, 0.1], [0.6, 0.0, 0.9], [0.0, 0.75, 0.75], [0.33, 0.33, 0.33],
                    [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.9, 0.5, 0.25], [0.123, 0.456, 0.789], [0.5, 0.5, 0.0]])


def case(h, w, masks=None, boxes=None, alpha=0.5, edge=True, lw=1, colors=None, seed=0):
    n = len(masks) if masks is not None else (len(boxes) if boxes is not None else 0)
    assert masks is None or boxes is None or len(masks) == len(boxes)
    assert masks is None or all(np.asarray(m).shape == (h, w) for m in masks)
    return {"image": image(h, w, seed), "masks": None if masks is None else [np.asarray(m, bool) for m in masks],
            "boxes": None if boxes is None else [tuple(float(v) for v in b) for b in boxes], "alpha": alpha, "edge": edge, "lw": lw,
            "colors": PALETTE[np.arange(n) % len(PALETTE)] if colors is None else np.asarray(colors, np.float64).reshape(n, 3)}


def overlap_masks(h, w, k):
    """k masks that all cover the centre of the image: shifted discs and a box"""
    out = [disc(h, w, h / 2 + 2 * i - k, w / 2 - 3 * i + k, h / 3, w / 4) for i in range(k - 1)]
    return out + [rect(h, w, h // 3, 2 * h // 3, w // 5, 4 * w // 5)]


@functools.lru_cache(maxsize=None)
def hand_cases():
    c = {}
    # every image size against every other: a disc over the centre, a box along the borders, one frame.  Heights / widths 1: all edge
    for h in SIZES:
        for w in SIZES:
            c[f"size_{h}x{w}"] = case(h, w, [disc(h, w, h / 2, w / 2, h / 2.5 + 1, w / 2.5 + 1), rect(h, w, 0, max(h // 2, 1), 0, w)],
                                      [(0, 0, w - 1, h - 1), (w / 4, h / 4, 3 * w / 4, 3 * h / 4)], lw=1 + (h + w) % 3, seed=h + w)
    H, W = 70, 75
    # one run of the list crosses a column end: the last rows of column 9 and the first rows of column 10
    c["run_crosses_column_end"] = case(H, W, [rect(H, W, H - 3, H, 9, 10) | rect(H, W, 0, 4, 10, 11)])
    c["full_image"] = case(H, W, [np.ones((H, W), bool)])
    c["full_image_130"] = case(130, 130, [np.ones((130, 130), bool)], [(0, 0, 129, 129)], lw=2)
    # single pixels: the four corners, each border, both sides of the tile corner (63 | 64, 63 | 64)
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 30), (H - 1, 30), (30, 0), (30, W - 1), (63, 63), (63, 64), (64, 63), (64, 64), (20, 20)]
    c["single_pixels"] = case(H, W, [pixels(H, W, [p]) for p in pts])
    c["single_pixels_one_mask"] = case(H, W, [pixels(H, W, pts)])
    # 4-neighbourhood against 8-neighbourhood: stairs two pixels thick, the pixels diagonal to the outside are inner pixels
    stairs = np.zeros((H, W), bool)
    for i in range(5, 60):
        stairs[i:i + 9, i:i + 9] = True
    c["diagonal_stairs"] = case(H, W, [stairs, np.eye(H, W, dtype=bool)])
    hole = rect(H, W, 10, 68, 10, 70)
    hole[30, 40] = hole[63, 63] = hole[64, 64] = False               # one-pixel holes: their four neighbours become edge pixels
    c["one_pixel_holes"] = case(H, W, [hole])
    c["empty_mask_with_box"] = case(H, W, [np.zeros((H, W), bool), disc(H, W, 30, 30, 12)], [(5, 6, 40, 50), (18, 18, 42, 42)])
    # words and outer columns at the tile seams: a mask whose edge runs along rows 63 | 64 and columns 63 | 64 of a 130 x 130 image
    c["seam_edges"] = case(130, 130, [rect(130, 130, 10, 64, 10, 64), rect(130, 130, 64, 120, 64, 120), rect(130, 130, 63, 66, 0, 130),
                                      rect(130, 130, 0, 130, 62, 65), disc(130, 130, 64, 64, 40)])
    # draw order: the same masks in two orders
    for k in (3, 4):
        ms = overlap_masks(H, W, k)
        bx = [(5 + 4 * i, 8 + 3 * i, 60 - 2 * i, 55 + i) for i in range(k)]
        c[f"order_{k}_forward"] = case(H, W, ms, bx, alpha=0.3)
        c[f"order_{k}_reverse"] = case(H, W, ms[::-1], bx[::-1], alpha=0.3, colors=PALETTE[np.arange(k)][::-1])
    # boxes: on and beyond the border, inverted, degenerate, wider lines than the box, a frame crossed by the next instance's mask
    c["boxes_border"] = case(H, W, None, [(0, 0, W - 1, H - 1), (-20, -5, 30.4, 20.5), (50.5, 40.5, 500, 400), (W - 1, H - 1, W - 1, H - 1), (0.49, 0.5, 1.5, 2.5)])
    c["boxes_inverted"] = case(H, W, None, [(40, 10, 20, 30), (10, 50, 30, 35), (60, 60, 45, 42), (25, 25, 25, 40), (30, 12, 44, 12)], lw=2)
    for lw in (1, 2, 3):
        c[f"boxes_lw{lw}"] = case(H, W, None, [(3, 4, 60, 66), (62, 62, 66, 66), (0, 0, 1, 1), (70, 20, 74, 69)], lw=lw)
    c["boxes_lw_larger_than_box"] = case(H, W, None, [(10, 10, 13, 12), (72, 66, 74, 69), (0, 0, 2, 2), (40, 40, 20, 30)], lw=9)
    c["box_crossed_by_next_mask"] = case(H, W, [disc(H, W, 20, 20, 9), disc(H, W, 30, 34, 14), rect(H, W, 0, 70, 40, 44)],
                                         [(8, 8, 34, 34), (20, 16, 48, 44), (40, 0, 43, 69)], lw=2)
    # arguments
    for a in (0, 0.3, 0.5, 1):
        c[f"alpha_{a}"] = case(H, W, overlap_masks(H, W, 3), [(5, 5, 50, 50)] * 3, alpha=a)
    c["edge_off"] = case(H, W, overlap_masks(H, W, 3) + [hole], None, edge=False)
    c["masks_without_boxes"] = case(H, W, overlap_masks(H, W, 4))
    c["boxes_without_masks"] = case(H, W, None, [(5, 5, 50, 50), (30, 30, 74, 69)])
    c["no_instances"] = case(H, W, [], [])
    c["more_than_64_instances"] = case(H, W, [disc(H, W, 5 + (7 * i) % 60, 5 + (11 * i) % 65, 3 + i % 6) for i in range(70)],
                                       [(i % 50, (3 * i) % 40, i % 50 + 20, (3 * i) % 40 + 25) for i in range(70)])
    return c


HAND = tuple(hand_cases().keys())
N_SEEDED = 200


@functools.lru_cache(maxsize=None)
def seeded_case(i):
    """images of at most 140 x 140, up to 12 instances: discs, boxes, noise, now and then an empty or a full mask; with and without boxes"""
    r = np.random.default_rng(20261018 + i)
    h, w = (int(v) for v in r.integers(1, 141, size=2))
    if i % 10 == 0:
        h, w = int(r.choice([63, 64, 65, 128, 129])), int(r.choice([63, 64, 65, 128, 129]))

    def blob():
        kind = int(r.integers(0, 12))
        if kind == 0:
            return np.zeros((h, w), bool)
        if kind == 1:
            return np.ones((h, w), bool)
        if kind < 5:
            r0, c0 = int(r.integers(0, h)), int(r.integers(0, w))
            return rect(h, w, r0, r0 + 1 + int(r.integers(0, h)), c0, c0 + 1 + int(r.integers(0, w)))
        if kind == 5:
            return r.random((h, w)) < 0.5
        return disc(h, w, r.integers(0, h), r.integers(0, w), r.integers(1, 50), r.integers(1, 50))

    n = int(r.integers(0, 13))
    what = int(r.integers(0, 4))                                     # 0: masks only, 1: boxes only, else both
    masks = [blob() for _ in range(n)] if what != 1 else None
    boxes = [tuple(r.uniform(-10, max(h, w) + 10, size=4).tolist()) for _ in range(n)] if what != 0 else None
    return case(h, w, masks, boxes, alpha=float(r.choice([0.0, 0.3, 0.5, 0.77, 1.0])), edge=bool(r.integers(0, 4)), lw=int(r.integers(1, 5)),
                colors=r.random((n, 3)), seed=i)


def get(name):
    return seeded_case(int(name[5:])) if name.startswith("seed_") else hand_cases()[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the dense reference: the untouched primitives of the Visualizer, instance by instance"""
    c = get(name)
    vis = Visualizer(c["image"])
    n = len(c["colors"])
    for i in range(n):
        if c["masks"] is not None:
            vis.draw_binary_mask(c["masks"][i], c["colors"][i], alpha=c["alpha"], edge=c["edge"])
        if c["boxes"] is not None:
            vis.draw_box(c["boxes"][i], c["colors"][i], line_width=c["lw"])
    out = vis.output.img
    out.setflags(write=False)
    return out


def call(name, ctx=None):
    """amp_render_instances on the case through the thin binding (ctx None: the host path)"""
    c = get(name)
    h, w = c["image"].shape[:2]
    tables, edge_rgb, ibox, box_rgb = analyze.render_inputs(c["colors"], c["alpha"], c["boxes"], h, w)
    masks = None if c["masks"] is None else [enc(m) for m in c["masks"]]
    return rle.render_instances(c["image"], masks, tables, edge_rgb if c["edge"] else None, ibox, box_rgb, c["lw"], ctx=ctx)


def check_case(name, ctx=None):
    """the call against the dense reference, byte for byte; returns the drawn image"""
    got, want = call(name, ctx), expected(name)
    assert got.dtype == np.uint8 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError(f"{name}: {len(bad)} pixels differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])].tolist()} != {want[tuple(bad[0])].tolist()}")
    return got


# ---- the micrograph: 48 of the 351 ground-truth instances of one 1024 x 1536 image, overlapping ones first ------------------------------------

MICROGRAPH = "Sc1Tile_001-002-000_0-000.png"
N_SUBSET = 48


@functools.lru_cache(maxsize=None)
def micrograph_subset():
    """indices of N_SUBSET instances: those whose XYXY box meets another instance's box, in index order, filled up with the first others"""
    import seg_perf_data as data
    _, boxes, _ = data.gt_polygons(MICROGRAPH)
    x0, y0, x1, y1 = boxes.T
    meet = (x0[:, None] <= x1[None]) & (x0[None] <= x1[:, None]) & (y0[:, None] <= y1[None]) & (y0[None] <= y1[:, None])
    np.fill_diagonal(meet, False)
    first = np.flatnonzero(meet.any(axis=1)).tolist()
    rest = [i for i in range(len(boxes)) if i not in set(first)]
    return (first + rest)[:N_SUBSET]


def micrograph_image():
    import seg_perf_data as data
    return image(*data.SIZE, seed=5)


def micrograph_colors(n):
    return PALETTE[(np.arange(n) * 5) % len(PALETTE)]


def golden_renders():
    """name -> image of every Visualizer call pinned by tests/golden/render_vectors.json (made by tests/golden/make_render_vectors.py with the
    Visualizer as it was before overlay_instances went through amp_render_instances): the inputs of tests/test_facade.py and the micrograph
    subset with and without labels and boxes, from RLE dicts, polygons and bool arrays"""
    import seg_perf_data as data
    from ampis_amd.structures import Boxes, BoxMode, Instances
    out = {}
    img = np.full((60, 80, 3), 100, np.uint8)
    m0, m1 = rect(60, 80, 10, 30, 10, 40), rect(60, 80, 35, 55, 50, 75)
    boxes = np.array([[10, 10, 39, 29], [50, 35, 74, 54]], np.float32)
    two = np.array([[1, 0, 0], [0, 1, 0]])
    out["facade_rle_boxes_empty_labels"] = Visualizer(img, {"thing_classes": ["a"]}, scale=1).overlay_instances(
        boxes=boxes, masks=[rle.encode(m0), rle.encode(m1)], labels=["", ""], assigned_colors=two).get_image()
    out["facade_bool_arrays"] = Visualizer(img, None).overlay_instances(masks=np.stack([m0, m1]), assigned_colors=two).get_image()
    dd = {"annotations": [{"bbox": [10, 10, 30, 20], "bbox_mode": BoxMode.XYWH_ABS, "segmentation": [[10, 10, 40, 10, 40, 30, 10, 30]], "category_id": 0}]}
    out["facade_dataset_dict"] = Visualizer(img, {"thing_classes": [""]}).draw_dataset_dict(dd).get_image()
    inst = Instances((60, 80), pred_boxes=Boxes(boxes), scores=np.array([0.9, 0.8], np.float32), pred_classes=np.array([0, 0]),
                     pred_masks=[rle.encode(m0), rle.encode(m1)])
    out["facade_predictions_scale2"] = Visualizer(img, {"thing_classes": ["p"]}, scale=2).draw_instance_predictions(inst).get_image()
    out["facade_predictions_labels"] = Visualizer(img, {"thing_classes": ["p"]}).draw_instance_predictions(inst).get_image()
    sub = micrograph_subset()
    polys, gt_boxes, size = data.gt_polygons(MICROGRAPH)
    rles = [data.gt_rles(MICROGRAPH)[i] for i in sub]
    bx, big = gt_boxes[sub], micrograph_image()
    labels = [("" if k % 7 == 3 else f"particle {k}") for k in range(len(sub))]
    cols = micrograph_colors(len(sub))
    for name, kw in (("labels_boxes", dict(boxes=bx, labels=labels)), ("boxes", dict(boxes=bx)), ("labels", dict(labels=labels)), ("plain", {})):
        out[f"micrograph_rle_{name}"] = Visualizer(big).overlay_instances(masks=rles, assigned_colors=cols, alpha=0.4, **kw).get_image()
    dd = {"annotations": [{"bbox": gt_boxes[i].tolist(), "bbox_mode": BoxMode.XYXY_ABS, "segmentation": [np.asarray(p).tolist() for p in polys[i]],
                           "category_id": k % 2} for k, i in enumerate(sub)]}
    out["micrograph_dataset_dict_polygons"] = Visualizer(big, {"thing_classes": ["particle", "satellite"]}).draw_dataset_dict(dd).get_image()
    dense = np.stack([rle.decode(r).astype(bool) for r in rles[:6]])
    out["micrograph_bool_arrays_default_colors"] = Visualizer(big).overlay_instances(masks=dense, boxes=bx[:6], labels=labels[:6]).get_image()
    return out
