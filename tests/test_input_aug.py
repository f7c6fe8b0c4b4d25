"""Host side of the train-time input augmentations (no GPU; the built library's host functions): INPUT.CROP, INPUT.RANDOM_FLIP
"horizontal" | "vertical" | "none" and INPUT.MIN_SIZE_TRAIN_SAMPLING "choice" | "range" as detectron2's DatasetMapper.from_config reads them
for a Mask R-CNN config -- the statistics of the draws, the run-length and polygon forms of a cropped mask against dense restatements, the
three annotation transforms against each other, and the refusals."""
import json
import os

import numpy as np
import pytest

CROP_TYPES = {"relative_range": [0.9, 0.9], "relative": [0.75, 0.5], "absolute": [30, 70], "absolute_range": [20, 30]}


def _cfg(**inp):
    from ampis_amd.config import get_cfg
    cfg = get_cfg()
    for k, v in inp.items():
        node, parts = cfg.INPUT, k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg


def _crop_cfg(kind, **inp):
    return _cfg(**{"CROP.ENABLED": True, "CROP.TYPE": kind, "CROP.SIZE": CROP_TYPES[kind]}, **inp)


# ---- 1. the draws ---------------------------------------------------------------------------------------------------------------------

def test_default_cfg_draws_the_sequence_it_always_drew():
    """draw() under a cfg that sets none of the new keys: (min_size, bool), consumed from the generator in the order recorded on the commit
    before INPUT.CROP existed (tests/golden/input_aug_default_draws.json: DatasetMapper(cfg, True, seed=1), 64 draws)."""
    from ampis_amd import model_zoo
    from ampis_amd.config import get_cfg
    from ampis_amd.data import DatasetMapper
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "input_aug_default_draws.json")))
    cfg = get_cfg()
    assert cfg.INPUT.CROP.ENABLED is False and cfg.INPUT.CROP.TYPE == "relative_range" and list(cfg.INPUT.CROP.SIZE) == [0.9, 0.9]
    assert cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING == "choice" and cfg.INPUT.RANDOM_FLIP == "horizontal"
    for name in ("get_cfg", "mask_rcnn_R_50_FPN_3x"):
        cfg = get_cfg()
        if name != "get_cfg":
            cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/" + name + ".yaml"))
        m = DatasetMapper(cfg, True, seed=1)
        got = [m.draw() for _ in range(64)]
        assert all(type(a) is int and type(b) is bool for a, b in got)
        assert [[a, b] for a, b in got] == gold[name]


@pytest.mark.parametrize("kind", sorted(CROP_TYPES))
def test_crop_draws_stay_inside_their_ranges_and_reach_both_ends(kind):
    from ampis_amd.data import DatasetMapper, unpack_aug
    from ampis_amd.engine.defaults import crop_window, input_kwargs
    cfg = _crop_cfg(kind)
    h, w = 40, 25
    s0, s1 = CROP_TYPES[kind]
    want_h, want_w = {"relative_range": ((36, 40), (23, 25)),                 # int(40 * 0.9 + 0.5) .. 40, int(25 * 0.9 + 0.5) .. 25
                      "relative": ((30, 30), (13, 13)),                       # int(40 * 0.75 + 0.5), int(25 * 0.5 + 0.5)
                      "absolute": ((30, 30), (25, 25)),                       # min(30, 40), min(70, 25)
                      "absolute_range": ((20, 30), (20, 25))}[kind]           # [min(40, 20), min(40, 30)], [min(25, 20), min(25, 30)]
    m = DatasetMapper(cfg, True, seed=11)
    wins = []
    for _ in range(4000):
        size, aug = m.draw()
        hf, vf, u = unpack_aug(aug)
        assert not vf and len(u) == 4 and all(0.0 <= v < 1.0 for v in u)
        wins.append(crop_window(input_kwargs(cfg)["crop"], h, w, u))
    wins = np.asarray(wins)
    y0, x0, ch, cw = wins.T
    assert (ch.min(), ch.max()) == want_h and (cw.min(), cw.max()) == want_w
    assert y0.min() == 0 and x0.min() == 0 and (y0 + ch <= h).all() and (x0 + cw <= w).all()
    assert (y0 + ch == h).any() and (x0 + cw == w).any() and ((y0 > 0) & (y0 + ch == h)).any() == bool((ch < h).any())
    if kind.endswith("range"):      # every integer extent in between occurs too
        assert set(ch.tolist()) == set(range(want_h[0], want_h[1] + 1)) and set(cw.tolist()) == set(range(want_w[0], want_w[1] + 1))
    # the origin is uniform over [0, h - ch]: for the most frequent extent every origin occurs
    top = np.bincount(ch).argmax()
    assert set(y0[ch == top].tolist()) == set(range(0, h - top + 1))


def test_flip_axes_and_range_scale_sampling():
    from ampis_amd.data import DatasetMapper, unpack_aug
    n = 4000
    for axis in ("horizontal", "vertical", "none"):
        m = DatasetMapper(_cfg(RANDOM_FLIP=axis), True, seed=2)
        flips = np.asarray([unpack_aug(m.draw()[1])[:2] for _ in range(n)])
        on, off = (0, 1) if axis == "horizontal" else (1, 0)
        assert not flips[:, off].any()
        if axis == "none":
            assert not flips.any()
        else:
            assert abs(flips[:, on].mean() - 0.5) < 0.05         # five standard deviations of 4000 fair coins: 0.04
    # a crop rides along with either axis
    m = DatasetMapper(_crop_cfg("relative_range", RANDOM_FLIP="vertical"), True, seed=3)
    flips = np.asarray([unpack_aug(m.draw()[1])[:2] for _ in range(n)])
    assert not flips[:, 0].any() and abs(flips[:, 1].mean() - 0.5) < 0.05
    m = DatasetMapper(_cfg(MIN_SIZE_TRAIN=(30, 37), MIN_SIZE_TRAIN_SAMPLING="range"), True, seed=4)
    sizes = [m.draw()[0] for _ in range(n)]
    assert set(sizes) == set(range(30, 38)) and all(type(s) is int for s in sizes)
    m = DatasetMapper(_cfg(MIN_SIZE_TRAIN=(30, 37)), True, seed=4)
    assert {m.draw()[0] for _ in range(200)} == {30, 37}          # "choice": the two values, nothing between


# ---- 2. a cropped bitmask in the run-length domain -----------------------------------------------------------------------------------------

def _dense_crop(mask, win, nh, nw, flips):
    from PIL import Image
    y0, x0, ch, cw = win
    m = np.asarray(Image.fromarray(np.ascontiguousarray(mask[y0:y0 + ch, x0:x0 + cw]).astype(np.uint8)).resize((nw, nh), Image.NEAREST))
    if flips & 1:
        m = m[:, ::-1]
    if flips & 2:
        m = m[::-1]
    return m.astype(bool)


def test_rle_domain_crop_resize_is_slice_then_pil_nearest_then_numpy_flips():
    """amp_rle_crop_resize_nearest against decode -> slice -> PIL NEAREST -> [:, ::-1] / [::-1] -> encode, run for run."""
    from ampis_amd import rle
    rng = np.random.default_rng(0)
    h, w = 23, 31
    masks = [rng.random((h, w)) > 0.5, rng.random((h, w)) > 0.9, np.zeros((h, w), bool), np.ones((h, w), bool)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):             # one pixel in each corner
        m = np.zeros((h, w), bool); m[y, x] = True
        masks.append(m)
    blocky = np.zeros((h, w), bool); blocky[5:17, 8:22] = True; blocky[9:12, 12:15] = False
    masks.append(blocky)
    windows = [(0, 0, h, w),                                                    # everything
               (0, 4, 9, 11), (h - 9, 4, 9, 11), (6, 0, 9, 11), (6, w - 11, 9, 11),   # touching the top, bottom, left, right border
               (0, 0, 1, 1), (h - 1, w - 1, 1, 1), (11, 13, 1, 1), (0, 7, 1, 9), (3, w - 1, 12, 1),   # 1-pixel windows and 1-pixel-wide strips
               (4, 5, 15, 20)]
    sizes = lambda ch, cw: [(ch, cw), (2 * ch + 3, 3 * cw + 1), (max(1, ch // 2), max(1, (2 * cw) // 3)), (ch + 5, max(1, cw - 3)), (1, 1)]
    n = 0
    for m in masks:
        r = rle.encode(np.asfortranarray(m))
        for win in windows:
            for nh, nw in sizes(win[2], win[3]):
                for flips in range(4):
                    ref = _dense_crop(m, win, nh, nw, flips)
                    got = rle.crop_resize_nearest(r, win, nh, nw, flips & 1, flips & 2)
                    want = rle.encode(np.asfortranarray(ref))
                    assert got["size"] == [nh, nw] and got["counts"] == want["counts"], (win, nh, nw, flips)
                    assert np.array_equal(rle.string_to_counts(got["counts"]), rle.string_to_counts(want["counts"]))
                    ys, xs = np.nonzero(ref)
                    assert rle.bbox(got) == (None if len(ys) == 0 else (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1))
                    n += 1
    assert n == len(masks) * len(windows) * 5 * 4
    # a micrograph-sized mask, down-scaled from a window, both mirrors
    m = np.zeros((1024, 1536), bool); m[300:700, 200:900] = True; m[::97, ::89] = True
    win = (51, 77, 922, 1382)
    got = rle.crop_resize_nearest(rle.encode(np.asfortranarray(m)), win, 800, 1199, True, True)
    assert np.array_equal(rle.decode(got).astype(bool), _dense_crop(m, win, 800, 1199, 3))
    with pytest.raises(RuntimeError, match="amp_rle_crop_resize_nearest"):
        rle.crop_resize_nearest(rle.encode(np.asfortranarray(masks[0])), (0, 0, h + 1, w), 10, 10)


# ---- 3. the polygon clipper, by region ---------------------------------------------------------------------------------------------------------

def _even_odd(poly, px, py):
    """Even-odd point-in-polygon of the points (px, py) + their distance to the nearest edge."""
    x, y = poly[0::2], poly[1::2]
    inside = np.zeros(px.shape, bool)
    dist = np.full(px.shape, np.inf)
    for i in range(len(x)):
        ax, ay, bx, by = x[i], y[i], x[(i + 1) % len(x)], y[(i + 1) % len(x)]
        if (ay > py).any() or (by > py).any():
            cross = ((ay > py) != (by > py))
            with np.errstate(divide="ignore", invalid="ignore"):
                xi = ax + (py - ay) * (bx - ax) / (by - ay)
            inside ^= cross & (px < xi)
        dx, dy = bx - ax, by - ay
        L2 = dx * dx + dy * dy
        t = np.clip(((px - ax) * dx + (py - ay) * dy) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(px.shape)
        dist = np.minimum(dist, np.hypot(px - (ax + t * dx), py - (ay + t * dy)))
    return inside, dist


def _clip(polys, win):
    from ampis_amd import rle
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
    out, oo = rle.clip_polygons(np.concatenate(polys), off, np.arange(len(polys)), *win)
    return [out[oo[j]: oo[j + 1]] for j in range(len(polys))]


def test_polygon_clipper_keeps_exactly_the_region_inside_the_window():
    from ampis_amd import synth
    win = (40.5, 30.25, 150.0, 120.75)            # x0, y0, x1, y1
    _, gt = synth.micrograph(3, 160, 200, seed=5)
    polys = [np.asarray(p, np.float64) for p in gt["polygons"]]
    # non-convex ones that leave and re-enter the window: a comb through the right border, a U around the top-left corner, a spiral arm
    polys.append(np.array([100, 40, 170, 40, 170, 50, 120, 50, 120, 60, 170, 60, 170, 70, 120, 70, 120, 80, 170, 80, 170, 90, 100, 90], np.float64))
    polys.append(np.array([20, 20, 90, 20, 90, 50, 80, 50, 80, 28, 30, 28, 30, 100, 60, 100, 60, 110, 20, 110], np.float64))
    polys.append(np.array([60, 100, 160, 100, 160, 140, 50, 140, 50, 60, 70, 60, 70, 130, 145, 130, 145, 110, 60, 110], np.float64))
    polys.append(np.array([45.0, 35.0, 60.0, 35.0, 52.5, 47.0]))              # inside
    polys.append(np.array([160.0, 10.0, 190.0, 10.0, 175.0, 25.0]))            # outside
    polys.append(np.array([150.0, 40.0, 150.0, 60.0, 180.0, 50.0]))            # touches the right border along an edge only: no area inside
    got = _clip(polys, win)
    gx, gy = np.meshgrid(np.linspace(win[0], win[2], 150), np.linspace(win[1], win[3], 150))
    gx, gy = gx.ravel(), gy.ravel()
    straddling = 0
    for p, q in zip(polys, got):
        x, y = p[0::2], p[1::2]
        inside = x.min() >= win[0] and x.max() <= win[2] and y.min() >= win[1] and y.max() <= win[3]
        outside = x.max() <= win[0] or x.min() >= win[2] or y.max() <= win[1] or y.min() >= win[3]
        if inside:
            assert q.tobytes() == p.tobytes()                                  # bit-identical, vertex order included
        if outside:
            assert len(q) == 0
        if len(q):
            assert len(q) >= 6 and q[0::2].min() >= win[0] and q[0::2].max() <= win[2] and q[1::2].min() >= win[1] and q[1::2].max() <= win[3]
        a, da = _even_odd(p, gx, gy)
        b, db = _even_odd(q, gx, gy) if len(q) else (np.zeros(gx.shape, bool), np.full(gx.shape, np.inf))
        ok = (da > 1e-9) & (db > 1e-9)
        assert ok.sum() > 0.9 * len(gx) and np.array_equal(a[ok], b[ok])
        straddling += int(not inside and not outside and len(q) > 0)
    assert len(got[-1]) == 0 and len(got[-2]) == 0 and straddling >= 8


# ---- 4. the three annotation transforms ---------------------------------------------------------------------------------------------------------

def _annos(h, w):
    """Synthetic micrograph instances, category_id = the instance's index (so the survivors of a crop can be named)."""
    from ampis_amd import synth
    _, gt = synth.micrograph(1, h, w, seed=5)
    return [{"bbox": [float(v) for v in b], "bbox_mode": 0, "segmentation": [[float(v) for v in p]], "category_id": i}
            for i, (b, p) in enumerate(zip(gt["boxes"], gt["polygons"]))]


@pytest.mark.parametrize("recompute", [True, False])
def test_vectorised_per_instance_and_bitmask_transforms_agree_under_crop_and_flips(recompute):
    from ampis_amd import data, rle
    h, w = 200, 280
    annos = _annos(h, w)
    parsed = data.parse_annotations(annos)
    assert parsed is not None and parsed["n"] == len(annos) > 40
    cases = 0
    for win in ((0, 0, h, w), (17, 33, 150, 190), (60, 100, 90, 61), (0, 150, 200, 130)):
        y0, x0, ch, cw = win
        ext = parsed["extent"]
        gone = {i for i in range(len(annos)) if ext[i, 2] <= x0 or ext[i, 0] >= x0 + cw or ext[i, 3] <= y0 or ext[i, 1] >= y0 + ch}
        whole = {i for i in range(len(annos)) if ext[i, 0] >= x0 and ext[i, 2] <= x0 + cw and ext[i, 1] >= y0 and ext[i, 3] <= y0 + ch}
        for nh, nw in ((ch, cw), (int(ch * 1.37), int(cw * 0.81))):           # no resize; anisotropic
            for hf in (False, True):
                for vf in (False, True):
                    kw = dict(crop=win, vflip=vf, recompute_boxes=recompute)
                    vec = data.transform_parsed(parsed, nw / cw, nh / ch, hf, nw, nh, **kw)
                    loop = data._transform_annotations_loop(annos, nw / cw, nh / ch, hf, nw, nh, **kw)
                    assert data.transform_annotations(annos, nw / cw, nh / ch, hf, nw, nh, **kw)["boxes"].tobytes() == vec["boxes"].tobytes()
                    assert vec["boxes"].dtype == np.float32 and vec["boxes"].tobytes() == loop["boxes"].tobytes()
                    assert vec["classes"].tolist() == loop["classes"].tolist() and len(vec["polygons"]) == len(loop["polygons"]) == len(vec["boxes"])
                    assert vec["poly_len"].tolist() == [len(p) for p in vec["polygons"]] and len(vec["poly_flat"]) == vec["poly_len"].sum()
                    for p, q in zip(vec["polygons"], loop["polygons"]):
                        assert p.tobytes() == q.tobytes()
                    kept = set(vec["classes"].tolist())
                    assert whole <= kept and not (gone & kept)
                    if recompute:
                        assert kept == set(range(len(annos))) - gone or len(kept) < len(annos) - len(gone)      # a sliver may clip to nothing
                        for b, p in zip(vec["boxes"], vec["polygons"]):
                            want = np.array([p[0::2].min(), p[1::2].min(), max(p[0::2].max(), 0.0), max(p[1::2].max(), 0.0)]).astype(np.float32)
                            assert b.tobytes() == want.tobytes()
                            assert 0 <= b[0] < b[2] <= nw and 0 <= b[1] < b[3] <= nh
                    # the bitmask form of the same polygon annotations: the raster of the polygons the other forms hand on
                    bm = data.transform_annotations_bitmask(annos, h, w, nh, nw, hf, **kw)
                    exp = {}
                    for c, b, p in zip(loop["classes"].tolist(), loop["boxes"], loop["polygons"]):
                        r = rle.frPyObjects([p.tolist()], nh, nw)[0]
                        m = rle.decode(r)
                        ys, xs = np.nonzero(m)
                        if len(ys):
                            exp[c] = (r["counts"], np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32) if recompute else b)
                    assert bm["classes"].tolist() == sorted(exp) and not (gone & set(bm["classes"].tolist()))
                    for c, b, r in zip(bm["classes"].tolist(), bm["boxes"], bm["masks_rle"]):
                        assert r["size"] == [nh, nw] and r["counts"] == exp[c][0] and b.tobytes() == exp[c][1].tobytes()
                    cases += 1
    assert cases == 32


def test_bitmask_transform_of_rle_annotations_under_a_crop_matches_the_dense_pipeline():
    from ampis_amd import data, rle
    h, w = 120, 170
    polys = _annos(h, w)[:60]
    annos = []
    for a in polys:
        r = rle.frPyObjects(a["segmentation"], h, w)[0]
        annos.append(dict(a, segmentation=r))
    for win in ((10, 20, 100, 130), (40, 0, 55, 170)):
        for nh, nw, hf, vf in ((win[2], win[3], False, True), (150, 111, True, True), (61, 200, True, False)):
            got = data.transform_annotations_bitmask(annos, h, w, nh, nw, hf, crop=win, vflip=vf, recompute_boxes=True)
            exp = []
            for a in annos:
                m = _dense_crop(rle.decode(a["segmentation"]).astype(bool), win, nh, nw, int(hf) | 2 * int(vf))
                ys, xs = np.nonzero(m)
                if len(ys):
                    exp.append((a["category_id"], m, np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32)))
            assert 0 < len(exp) < len(annos) and got["classes"].tolist() == [e[0] for e in exp]
            for r, b, (_, m, eb) in zip(got["masks_rle"], got["boxes"], exp):
                assert np.array_equal(rle.decode(r).astype(bool), m) and b.tobytes() == eb.tobytes()
            # without recompute_boxes: the annotation's box, translated, scaled, mirrored and clipped
            plain = data.transform_annotations_bitmask(annos, h, w, nh, nw, hf, crop=win, vflip=vf)
            for c, b in zip(plain["classes"].tolist(), plain["boxes"]):
                e = np.asarray(annos[c]["bbox"], np.float64) - [win[1], win[0], win[1], win[0]]
                e[0::2] *= nw / win[3]; e[1::2] *= nh / win[2]
                if hf:
                    e[0], e[2] = nw - e[2], nw - e[0]
                if vf:
                    e[1], e[3] = nh - e[3], nh - e[1]
                assert b.tobytes() == np.clip(e, 0, [nw, nh, nw, nh]).astype(np.float32).tobytes()


def test_mapper_on_its_own_crops_and_flips_pixels_and_ground_truth_together():
    """DatasetMapper(cfg, True)(dataset_dict), the way a validation-loss hook calls it: the pixels are the window, resized and mirrored, the
    deferred form plans exactly that, and the ground truth moved with them (a marked instance stays under its mask)."""
    from PIL import Image
    from ampis_amd import rle, synth
    from ampis_amd.data import DatasetMapper, mapped_hw, unpack_aug
    from ampis_amd.engine.defaults import crop_window, input_kwargs, shortest_edge_size
    h, w = 120, 170
    img, _ = synth.micrograph(2, h, w, seed=5)
    img = img.copy()
    img[30:70, 40:100] = 255                                                     # a bright block with its annotation
    dd = {"file_name": "x.png", "image_bgr": img, "height": h, "width": w, "image_id": 0,
          "annotations": [{"bbox": [40, 30, 100, 70], "bbox_mode": 0, "segmentation": [[40, 30, 100, 30, 100, 70, 40, 70]], "category_id": 0}]}
    cfg = _cfg(**{"CROP.ENABLED": True, "CROP.TYPE": "relative_range", "CROP.SIZE": [0.8, 0.7], "RANDOM_FLIP": "vertical",
                  "MIN_SIZE_TRAIN": (96, 140), "MIN_SIZE_TRAIN_SAMPLING": "range", "MAX_SIZE_TRAIN": 220})
    m = DatasetMapper(cfg, True, seed=9)
    flips = 0
    for _ in range(30):
        size, aug = m.draw()
        hf, vf, u = unpack_aug(aug)
        y0, x0, ch, cw = crop_window(input_kwargs(cfg)["crop"], h, w, u)
        nh, nw = shortest_edge_size(ch, cw, size, 220)
        ref = np.asarray(Image.fromarray(np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])).resize((nw, nh), Image.BILINEAR)) if (nh, nw) != (ch, cw) else img[y0:y0 + ch, x0:x0 + cw]
        ref = ref[::-1] if vf else ref
        host, dev = m.apply(dd, size, aug), m.apply(dd, size, aug, True)
        assert np.array_equal(host["image_bgr"], ref) and host["image_bgr"].flags.c_contiguous and (host["height"], host["width"]) == (h, w)
        assert dev["image_bgr"] is img and dev["device_plan"] == (nh, nw, 2 * int(vf), y0, x0, ch, cw) and mapped_hw(dev) == (nh, nw)
        assert host["gt"]["boxes"].tobytes() == dev["gt"]["boxes"].tobytes() and len(host["gt"]["boxes"]) == 1
        x_a, y_a, x_b, y_b = host["gt"]["boxes"][0]
        inner = host["image_bgr"][int(np.ceil(y_a)) + 2:int(y_b) - 2, int(np.ceil(x_a)) + 2:int(x_b) - 2, 0]
        assert inner.size and (inner > 200).all()                               # the box still frames the bright block
        mask = rle.decode(rle.frPyObjects([host["gt"]["polygons"][0].tolist()], nh, nw)[0]).astype(bool)
        assert (host["image_bgr"][:, :, 0][mask] > 128).mean() > 0.9
        flips += int(vf)
    assert 5 < flips < 25
    # a second call of the mapper object draws afresh
    a, b = m(dd), m(dd)
    assert "gt" in a and "gt" in b


# ---- 5. refusals, defaults, capacity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inp, key", [
    ({"RANDOM_FLIP": "vertcal"}, r"INPUT\.RANDOM_FLIP"),
    ({"RANDOM_FLIP": True}, r"INPUT\.RANDOM_FLIP"),
    ({"CROP.ENABLED": True, "CROP.TYPE": "relative_rnge"}, r"INPUT\.CROP\.TYPE"),
    ({"CROP.ENABLED": "yes"}, r"INPUT\.CROP\.ENABLED"),
    ({"CROP.ENABLED": True, "CROP.SIZE": [0.9]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.SIZE": [0.9, 0.0]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.SIZE": [0.9, -0.5]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.SIZE": [0.9, "0.9"]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.SIZE": [1.2, 0.9]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.TYPE": "relative", "CROP.SIZE": [0.5, 1.5]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.TYPE": "absolute_range", "CROP.SIZE": [300, 200]}, r"INPUT\.CROP\.SIZE"),
    ({"CROP.ENABLED": True, "CROP.TYPE": "absolute", "CROP.SIZE": [300, float("nan")]}, r"INPUT\.CROP\.SIZE"),
    ({"MIN_SIZE_TRAIN_SAMPLING": "uniform"}, r"INPUT\.MIN_SIZE_TRAIN_SAMPLING"),
    ({"MIN_SIZE_TRAIN_SAMPLING": "range", "MIN_SIZE_TRAIN": (640, 672, 704)}, r"INPUT\.MIN_SIZE_TRAIN\b"),
    ({"MIN_SIZE_TRAIN_SAMPLING": "range", "MIN_SIZE_TRAIN": (640,)}, r"INPUT\.MIN_SIZE_TRAIN\b"),
])
def test_what_cannot_be_honoured_is_refused_by_name(inp, key):
    from ampis_amd.data import DatasetMapper
    from ampis_amd.engine.defaults import input_kwargs
    cfg = _cfg(**inp)
    with pytest.raises(ValueError, match=key):
        input_kwargs(cfg)
    with pytest.raises(ValueError, match=key):                                   # the mapper on its own refuses too: nothing trains silently without it
        DatasetMapper(cfg, True).draw()


def test_accepted_settings_and_the_keys_of_a_hand_built_cfg():
    from ampis_amd.config import CfgNode, get_cfg
    from ampis_amd.engine.defaults import input_kwargs
    assert get_cfg().INPUT.CROP.ENABLED is False
    assert input_kwargs(get_cfg()) == dict(sizes=(800,), sampling="choice", flip="horizontal", crop=None, recompute_boxes=False)
    bare = CfgNode({"INPUT": {"MIN_SIZE_TRAIN": 512}})                          # detectron2's defaults for what a hand-built node leaves out
    assert input_kwargs(bare) == dict(sizes=(512,), sampling="choice", flip="horizontal", crop=None, recompute_boxes=False)
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "absolute_range", "INPUT.CROP.SIZE", (384, 600), "INPUT.RANDOM_FLIP", "none"])
    assert input_kwargs(cfg) == dict(sizes=(800,), sampling="choice", flip="none", crop=("absolute_range", (384, 600)), recompute_boxes=True)
    cfg.INPUT.CROP.ENABLED = False                                               # a disabled crop's TYPE / SIZE are not looked at
    cfg.INPUT.CROP.TYPE = "nonsense"
    assert input_kwargs(cfg)["crop"] is None


@pytest.mark.parametrize("kind", sorted(CROP_TYPES))
def test_capacity_from_cfg_bounds_every_frame_a_crop_can_produce(kind):
    from ampis_amd.data import DatasetCatalog, DatasetMapper, unpack_aug
    from ampis_amd.engine.defaults import DefaultTrainer, crop_window, input_kwargs, shortest_edge_size
    shapes = [(200, 280), (280, 200), (192, 192)]
    dicts = [{"file_name": f"s{i}.png", "height": h, "width": w, "image_id": i, "annotations": []} for i, (h, w) in enumerate(shapes)]
    DatasetCatalog.clear()
    DatasetCatalog.register("cap_Train", lambda: dicts)
    try:
        sizes = {"relative_range": [0.6, 0.8], "relative": [0.75, 0.5], "absolute": [150, 260], "absolute_range": [100, 250]}[kind]
        for max_size in (260, 1000):                                             # with and without the MAX_SIZE_TRAIN clamp at work
            cfg = _cfg(**{"CROP.ENABLED": True, "CROP.TYPE": kind, "CROP.SIZE": sizes, "MIN_SIZE_TRAIN": (160, 224), "MIN_SIZE_TRAIN_SAMPLING": "range",
                          "MAX_SIZE_TRAIN": max_size})
            cfg.DATASETS.TRAIN, cfg.DATASETS.TEST = ("cap_Train",), ()
            tr = object.__new__(DefaultTrainer)                                  # the bound is a function of cfg alone: no device
            tr.cfg = cfg
            cap = tr._capacity_from_cfg()
            m = DatasetMapper(cfg, True, seed=6)
            for k in range(200):
                size, aug = m.draw()
                h0, w0 = shapes[k % len(shapes)]
                _, _, ch, cw = crop_window(input_kwargs(cfg)["crop"], h0, w0, unpack_aug(aug)[2])
                nh, nw = shortest_edge_size(ch, cw, size, max_size)
                assert (nh + 31) // 32 * 32 <= cap[0] and (nw + 31) // 32 * 32 <= cap[1], (kind, (h0, w0), (ch, cw), size, (nh, nw), cap)
            # a bound from the crop's geometry, not the MAX_SIZE_TRAIN square: no window of these settings is more than 2.5 times as long as it is
            # wide (absolute_range: 250 / 100; relative_range: 280 / (0.6 * 200) = 2.34), so no frame edge passes 224 * 2.5 = 560 -> 576 padded
            lim = min(576, (max_size + 31) // 32 * 32)
            assert cap[0] <= lim and cap[1] <= lim, (cap, lim)
    finally:
        DatasetCatalog.clear()
