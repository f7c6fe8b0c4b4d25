"""analyze.seg_perf_iset / seg_class_map / det_perf_iset / align_instance_sets / masks_to_bitmask_array (no GPU needed): the reference's return
shapes, keys, colour tables and labels; every kind of input; consistency with det_seg_scores; the fixture the reference itself made
(tests/golden/seg_perf_vectors.json.gz, generator beside it) byte for byte; and, where the reference tree exists, notebook cells 46 and 50 with
this module in place of the reference's, through the reference's own display_iset on the façade."""
import base64
import gzip
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd.structures import Instances, InstanceSet, PolygonMasks, RLEBitMasks, RLEMasks

import seg_class_cases as cs
import seg_class_ref as ref
import seg_perf_data as data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def gold():
    with gzip.open(os.path.join(data.GOLDEN, "seg_perf_vectors.json.gz"), "rt") as f:
        return json.load(f)


def _inputs(rec):
    gt = [data.gt_rles(rec["file_name"])[i] for i in rec["gt_indices"]]
    pred, boxes = data.pred_rles(rec["file_name"])
    return gt, [pred[i] for i in rec["pred_indices"]], data.gt_polygons(rec["file_name"])[1][rec["gt_indices"]], boxes[rec["pred_indices"]]


def _counts(masks):
    return [m["counts"] for m in masks]


# ---- the reference-made fixture -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(2))
def test_seg_perf_iset_equals_the_reference_byte_for_byte(gold, k):
    rec = gold["images"][k]
    gt, pred, _, _ = _inputs(rec)
    assert gold["n_instances"] == 100 and len(gt) == len(pred) == 100
    m = analyze.rle_instance_matcher(gt, pred)
    for key in ("tp", "fn", "fp", "iou"):
        assert np.array_equal(np.asarray(m[key]).reshape(-1), np.asarray(rec["match_results"][key]).reshape(-1)), key
    for mode in ("reduced", "all"):
        want = rec[mode]
        for match in (None, {k2: np.asarray(v) for k2, v in rec["match_results"].items()}):
            iset, (colors, labels) = analyze.seg_perf_iset(gt, pred, match_results=match, mode=mode, device="cpu")
            assert _counts(iset.instances.masks.rle) == [base64.b64decode(c) for c in want["counts_b64"]]
            assert all(r["size"] == [1024, 1536] for r in iset.instances.masks.rle) and list(iset.instances.image_size) == [1024, 1536]
            assert colors.tolist() == want["colors"] and labels == want["labels"]                      # value for value
            assert np.array_equal(iset.instances.colors, np.asarray(want["colors"])) and iset.instances.boxes.tolist() == want["boxes"]
            assert iset.instances.boxes.shape == (len(want["counts_b64"]), 4) and iset.instances.boxes.dtype == np.float64


@pytest.mark.parametrize("k", range(2))
def test_det_perf_iset_equals_the_reference(gold, k):
    rec = gold["images"][k]
    gt, pred, gt_boxes, pred_boxes = _inputs(rec)
    gi = InstanceSet(instances=Instances(data.SIZE, masks=RLEMasks(gt), boxes=gt_boxes))
    pi = InstanceSet(instances=Instances(data.SIZE, masks=RLEMasks(pred), boxes=pred_boxes))
    for key, tp_gt in (("det", False), ("det_tp_gt", True)):
        want = rec[key]
        iset, colormap = analyze.det_perf_iset(gi, pi, tp_gt=tp_gt)
        assert _counts(iset.instances.masks.rle) == [base64.b64decode(c) for c in want["counts_b64"]]
        assert iset.instances.boxes.tolist() == want["boxes"] and iset.instances.colors.tolist() == want["colors"]
        assert {k2: v.tolist() for k2, v in colormap.items()} == want["colormap"] and list(colormap) == list(want["colormap"])
    n_tp, n_fp, n_fn = (len(rec["match_results"][k2]) for k2 in ("tp", "fp", "fn"))
    assert len(rec["det"]["counts_b64"]) == n_tp + n_fp + n_fn and n_tp and n_fp and n_fn


# ---- return shapes, order, conventions --------------------------------------------------------------------------------------------------------------

def _toy():
    """3 ground truths, 3 predictions on 20 x 30: gt 0 matches pred 1, gt 1 is missed, gt 2 matches pred 2, pred 0 is spurious"""
    g = [cs.rect(20, 30, 1, 8, 1, 9), cs.rect(20, 30, 10, 18, 1, 6), cs.rect(20, 30, 2, 12, 15, 28)]
    p = [cs.rect(20, 30, 14, 19, 20, 29), cs.rect(20, 30, 1, 8, 2, 10), cs.rect(20, 30, 3, 12, 15, 27)]
    return [cs.enc(m) for m in g], [cs.enc(m) for m in p], g, p


def test_det_perf_iset_order_and_conventions():
    g, p, _, _ = _toy()
    m = analyze.rle_instance_matcher(g, p)
    assert m["tp"].tolist() == [[0, 1], [2, 2]] and m["fn"].tolist() == [1] and m["fp"].tolist() == [0]
    gb, pb = np.arange(12, dtype=np.float32).reshape(3, 4), 100 + np.arange(12, dtype=np.float32).reshape(3, 4)
    gi, pi = Instances((20, 30), masks=RLEMasks(g), boxes=gb), Instances((20, 30), masks=RLEMasks(p), boxes=pb)
    out = analyze.det_perf_iset(InstanceSet(instances=gi), InstanceSet(instances=pi))
    assert isinstance(out, tuple) and len(out) == 2                                       # colormap not given: (iset, colormap)
    iset, colormap = out
    assert isinstance(iset, InstanceSet) and isinstance(iset.instances, Instances) and isinstance(iset.instances.masks, RLEMasks)
    assert set(iset.instances.get_fields()) == {"masks", "boxes", "colors"} and list(colormap) == ["TP", "FP", "FN"]
    assert _counts(iset.instances.masks.rle) == _counts([p[1], p[2], p[0], g[1]])           # TP (predictions), FP, FN
    assert np.array_equal(iset.instances.boxes, np.concatenate([pb[[1, 2]], pb[[0]], gb[[1]]]))
    assert iset.instances.colors.tolist() == [[0.5, 0., 1.]] * 2 + [[0., 1., 1.]] + [[1., 0., 0.]]
    mine = {"TP": np.array([0.1, 0.2, 0.3, 1.0]), "FP": np.array([0.4, 0.5, 0.6, 1.0]), "FN": np.array([0.7, 0.8, 0.9, 0.5])}
    iset = analyze.det_perf_iset(InstanceSet(instances=gi), InstanceSet(instances=pi), colormap=mine, tp_gt=True)
    assert isinstance(iset, InstanceSet)                                                     # colormap given: the iset alone
    assert _counts(iset.instances.masks.rle) == _counts([g[0], g[2], p[0], g[1]])           # tp_gt: TP from the ground truth
    assert np.array_equal(iset.instances.boxes, np.concatenate([gb[[0, 2]], pb[[0]], gb[[1]]]))
    assert iset.instances.colors.tolist() == [mine["TP"].tolist()] * 2 + [mine["FP"].tolist()] + [mine["FN"].tolist()]
    # the caller's match_results are used as they are; plain mask lists get the tight boxes of their masks
    swapped = {"tp": np.array([[1, 0]]), "fn": np.array([0, 2]), "fp": np.array([1, 2]), "iou": np.array([0.0])}
    iset, _ = analyze.det_perf_iset(g, p, match_results=swapped)
    assert _counts(iset.instances.masks.rle) == _counts([p[0], p[1], p[2], g[0], g[2]])
    assert iset.instances.boxes.tolist()[0] == [20, 14, 29, 19] and iset.instances.boxes.tolist()[3] == [1, 1, 9, 8]


def test_seg_perf_iset_shapes_and_keys():
    g, p, _, _ = _toy()
    for mode, K, labels in (("reduced", 4, ["TP", "FN", "FP", "other"]),
                            ("all", 7, ["Other", "TP", "FN", "TP+FN", "FP", "TP+FP", "FN+FP", "TP+FN+FP"])):
        iset, colors = analyze.seg_perf_iset(g, p, mode=mode, device="cpu")
        assert isinstance(colors, list) and len(colors) == 2 and colors[1] == labels and colors[0].shape == (K, 3)
        inst = iset.instances
        assert isinstance(iset, InstanceSet) and set(inst.get_fields()) == {"masks", "colors", "boxes"} and len(inst) == K
        assert isinstance(inst.masks, RLEMasks) and len(inst.masks.rle) == K and list(inst.image_size) == [20, 30]
        assert np.array_equal(inst.boxes, np.zeros((K, 4))) and inst.colors is colors[0]
        r = analyze.seg_class_map(g, p, mode=mode, device="cpu")
        assert set(r) == {"masks", "labels", "colors", "pixel_counts", "match_results"} and r["pixel_counts"].shape == (8,)
        assert _counts(r["masks"]) == _counts(inst.masks.rle) and all(isinstance(c, bytes) for c in _counts(r["masks"]))
        want, want_px, _ = ref.dense(g, p, r["match_results"]["tp"], mode, (20, 30))
        assert [rle.string_to_counts(c).tolist() for c in _counts(r["masks"])] == [w.tolist() for w in want]
        assert r["pixel_counts"].tolist() == want_px.tolist()
    assert analyze.SEG_COLORS["reduced"] == [[0.5, 0., 1.], [1., 0., 0.], [0., 1., 1.], [1., 1., 0.]]
    with pytest.raises(ValueError, match="mode = 'some'"):
        analyze.seg_perf_iset(g, p, mode="some")
    with pytest.raises(ValueError, match="device = 'tpu'"):
        analyze.seg_perf_iset(g, p, device="tpu")
    with pytest.raises(ValueError, match="masks of different sizes"):
        analyze.seg_perf_iset(g, [cs.enc(np.ones((5, 5), bool))], device="cpu")
    with pytest.raises(ValueError, match=r"match_results\['tp'\]\[0\] = \(3, 0\)"):
        analyze.seg_perf_iset(g, p, match_results={"tp": np.array([[3, 0]])}, device="cpu")


def test_every_kind_of_input_gives_the_same_bytes():
    g, p, gd, pd = _toy()
    want = _counts(analyze.seg_perf_iset(g, p, mode="all", device="cpu")[0].instances.masks.rle)
    box = lambda m: [np.array([c0, r0, c1, r0, c1, r1, c0, r1], np.float64) for (r0, r1), (c0, c1) in
                     [((np.flatnonzero(m.any(1))[0], np.flatnonzero(m.any(1))[-1] + 1), (np.flatnonzero(m.any(0))[0], np.flatnonzero(m.any(0))[-1] + 1))]]
    polys = PolygonMasks([box(m) for m in gd])                          # axis-aligned boxes on pixel corners rasterise to themselves
    assert _counts(analyze.masks_to_rle(polys, (20, 30))) == _counts(g)
    kinds = {"rle list": (g, p, None), ".rle object": (RLEMasks(g), RLEBitMasks(p, (20, 30)), None), "polygons": (polys, p, (20, 30)),
             "bool array": (np.stack(gd), np.stack(pd), None),
             "instance sets": (InstanceSet(instances=Instances((20, 30), masks=polys)), InstanceSet(instances=Instances((20, 30), masks=RLEMasks(p))), None),
             "instances": (Instances((20, 30), masks=RLEMasks(g)), Instances((20, 30), masks=np.stack(pd)), None)}
    for name, (a, b, size) in kinds.items():
        got = analyze.seg_perf_iset(a, b, mode="all", size=size, device="cpu")[0].instances.masks.rle
        assert _counts(got) == want, name
    with pytest.raises(AssertionError, match="size="):
        analyze.seg_perf_iset(polys, p, device="cpu")


def test_an_empty_side_gives_all_background_classes():
    g, p, _, _ = _toy()
    for a, b in (([], p), (g, []), ([], [])):
        r = analyze.seg_class_map(a, b, mode="all", size=(20, 30), device="cpu")
        assert [rle.string_to_counts(m["counts"]).tolist() for m in r["masks"]] == [[600]] * 7 and r["pixel_counts"].tolist() == [600] + [0] * 7
        iset, _ = analyze.seg_perf_iset(a, b, size=(20, 30), device="cpu")
        assert len(iset.instances) == 4 and list(iset.instances.image_size) == [20, 30]
    with pytest.raises(ValueError, match="size="):
        analyze.seg_class_map([], [], device="cpu")


def test_masks_to_bitmask_array_and_the_containers():
    g, p, gd, _ = _toy()
    arr = analyze.masks_to_bitmask_array(g)
    assert arr.dtype == bool and arr.shape == (3, 20, 30) and np.array_equal(arr, np.stack(gd))
    assert analyze.masks_to_bitmask_array(arr) is arr
    iset = InstanceSet(instances=Instances((20, 30), masks=RLEMasks(g)), filepath="a/b.png", HFW=3.0, HFW_units="um", randomstate=5)
    assert np.array_equal(analyze.masks_to_bitmask_array(iset), arr) and np.array_equal(analyze.masks_to_bitmask_array(iset.instances), arr)
    assert analyze.masks_to_bitmask_array([], size=(4, 5)).shape == (0, 4, 5)
    for f in ("mask_format", "bbox_mode", "filepath", "annotations", "instances", "img", "dataset_class", "pred_or_gt", "HFW", "HFW_units",
              "randomstate", "rprops", "colors"):
        assert hasattr(iset, f), f
    dup = iset.copy()
    assert dup is not iset and dup.instances is not iset.instances and dup.filepath == "a/b.png" and dup.randomstate == 5
    assert _counts(dup.instances.masks.rle) == _counts(g) and isinstance(InstanceSet().randomstate, int)
    m = RLEMasks(g)
    assert len(m) == 3 and _counts(m[1].rle) == _counts(g[1:2]) and _counts(m[1:].rle) == _counts(g[1:])
    assert _counts(m[np.array([True, False, True])].rle) == _counts([g[0], g[2]]) and _counts(m[[2, 0]].rle) == _counts([g[2], g[0]])
    assert _counts(iset.instances[np.array([2, 0])].masks.rle) == _counts([g[2], g[0]])


# ---- align_instance_sets -------------------------------------------------------------------------------------------------------------------------

class _Item:
    def __init__(self, filepath, tag):
        self.filepath, self.tag = filepath, tag


def test_align_instance_sets():
    """The reference (ampis/analyze.py:42-51) matches by file name, keeps the order of `a`, and LEAVES OUT what has no partner on either side --
    it has no assert; notebook cell 61 relies on the dropping to remove images labelled in one dataset only.  This is held to the reference's
    own function where its tree exists (test_notebook_cells_46_and_50...)."""
    names = [f"img_{i}.png" for i in range(7)]
    order = np.random.default_rng(3).permutation(7)
    a = [_Item(f"gt/dir/{n}", ("a", n)) for n in names]
    b = [_Item(f"pred/other/{names[i]}", ("b", names[i])) for i in order]
    x, y = analyze.align_instance_sets(a, b)
    assert [i.tag for i in x] == [("a", n) for n in names] and [i.tag for i in y] == [("b", n) for n in names] and x[0] is a[0]
    # a name missing on either side: the item is left out, on both sides, and nothing else moves
    x, y = analyze.align_instance_sets(a[:5] + [_Item("only_in_a.png", "lone")], b)
    assert [i.tag for i in x] == [("a", n) for n in names[:5]] and [i.tag for i in y] == [("b", n) for n in names[:5]]
    assert analyze.align_instance_sets(a, []) == ([], []) and analyze.align_instance_sets([], b) == ([], [])
    from pathlib import Path
    x, y = analyze.align_instance_sets([_Item(Path("p") / names[2], 1)], b)
    assert len(x) == 1 and y[0].tag == ("b", names[2])


# ---- consistency with det_seg_scores ----------------------------------------------------------------------------------------------------------------

def test_true_positive_pixels_equal_det_seg_scores_on_disjoint_masks():
    """ground truths mutually disjoint and predictions mutually disjoint (one cell of a 6 x 6 grid each): a pixel is TP of at most one pair, so
    the pixels with the TP bit are exactly the sum of the pairs' intersections"""
    r = np.random.default_rng(11)
    h, w, cell = 96, 90, 15
    g, p = [], []
    for i, (y, x) in enumerate((y, x) for y in range(0, 90, cell) for x in range(0, 90, cell)):
        dy, dx = (int(v) for v in r.integers(-1, 2, size=2))
        g.append(cs.rect(h, w, y + 3, y + 12, x + 3, x + 12))
        if i % 5:
            p.append(cs.rect(h, w, max(y + 3 + dy, y), min(y + 12 + dy, y + cell), max(x + 3 + dx, x), min(x + 12 + dx, x + cell)))
    assert (np.sum(g, axis=0) <= 1).all() and (np.sum(p, axis=0) <= 1).all()
    ge, pe = [cs.enc(m) for m in g], [cs.enc(m) for m in p]
    scores = analyze.det_seg_scores(ge, pe)
    assert len(scores["det_tp"]) > 15 and len(scores["det_fn"]) > 3
    for mode in ("reduced", "all"):
        px = analyze.seg_class_map(ge, pe, mode=mode, device="cpu")["pixel_counts"]
        assert int(px[1] + px[3] + px[5] + px[7]) == int(np.sum(scores["seg_tp"])) and int(px.sum()) == h * w
        assert int(px[2] + px[3] + px[6] + px[7]) == int(np.sum(scores["seg_fn"])) and int(px[4] + px[5] + px[6] + px[7]) == int(np.sum(scores["seg_fp"]))


def test_device_cuda_without_a_device_is_an_error(monkeypatch):
    import torch
    from ampis_amd._lib import AmpError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g, p, _, _ = _toy()
    with pytest.raises(AmpError, match="no HIP device"):
        analyze.seg_perf_iset(g, p, device="cuda")
    assert len(analyze.seg_perf_iset(g, p, device="auto")[0].instances) == 4                       # 'auto' falls to the host


# ---- notebook cells 46 and 50 on the façade ---------------------------------------------------------------------------------------------------------

NOTEBOOK_CELLS = textwrap.dedent('''
    import json
    import numpy as np
    for _alias, _t in (("int", int), ("float", float), ("bool", bool)):
        if not hasattr(np, _alias):
            setattr(np, _alias, _t)
    from PIL import Image
    sys.modules["skimage.io"].imread = lambda p, as_gray=False: np.asarray(Image.open(str(p)).convert("L"))
    sys.modules["skimage"].color = types.ModuleType("skimage.color")
    sys.modules["skimage"].color.gray2rgb = lambda a: np.stack([a] * 3, -1) if a.ndim == 2 else a
    sys.modules["skimage.color"] = sys.modules["skimage"].color
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    sys.path.insert(0, REFERENCE)
    os.chdir(WORK)                                     # the notebook addresses the checkout as ./AMPIS
    nb = json.load(open(os.path.join(REFERENCE, "colab", "AMPIS Tutorial.ipynb")))
    ns = {}
    def run(i):
        src = "".join(l for l in nb["cells"][i]["source"] if not l.lstrip().startswith(("%", "!")))
        exec(compile(src, f"cell{i}", "exec"), ns)
    for i in (33, 35, 36, 38):
        run(i)
    reference_analyze = ns["analyze"]
    import ampis_amd.analyze as product
    # alignment: the product against the reference's own function, on the notebook's lists and on lists with names missing on either side
    for a, b in ((ns["iset_particles_gt"], ns["iset_particles_pred"]), (ns["iset_particles_gt"], ns["iset_satellites_gt"]),
                 (ns["iset_satellites_pred"][::-1], ns["iset_particles_gt"][1:])):
        want, got = reference_analyze.align_instance_sets(a, b), product.align_instance_sets(a, b)
        assert len(want[0]) == len(got[0]) > 0 and all(x is y for w_, g_ in zip(want, got) for x, y in zip(w_, g_))
    assert len(product.align_instance_sets(ns["iset_satellites_pred"], ns["iset_particles_gt"])[0]) < len(ns["iset_satellites_pred"])
    run(40)
    ns["analyze"] = product                            # cells 46 and 50 as they are, `analyze` being ampis_amd.analyze
    shown = []
    import ampis.visualize
    real = ampis.visualize.display_iset
    def display_iset(img, iset, **kw):                 # the reference's display_iset, its result kept for the checks below
        out = real(img, iset, get_img=True, **kw)
        shown.append((iset, out))
        return real(img, iset, **kw)
    ns["display_iset"] = display_iset
    run(46)
    run(50)
    gt, pred, img = ns["gt"], ns["pred"], ns["img"]
    assert type(gt.instances.masks).__name__ == "PolygonMasks" and len(shown) == 2
    for iset, out in shown:
        assert out.shape == img.shape and (out != img).any()
    # cell 46: the product's overlay instances equal the reference's own on the same polygon ground truth
    want, _ = reference_analyze.det_perf_iset(gt, pred)
    got = ns["iset_det"]
    assert [m["counts"] for m in got.instances.masks.rle] == [m["counts"] for m in want.instances.masks.rle]
    assert np.array_equal(got.instances.boxes, want.instances.boxes) and np.array_equal(got.instances.colors, want.instances.colors)
    # cell 50: four class masks of the image's size; apply_correction left the pixels outside every class untouched
    seg = ns["iset_seg"]
    assert len(seg.instances) == 4 and ns["color_labels"] == ["TP", "FN", "FP", "other"] and ns["colors"].shape == (4, 3)
    import ampis_amd.rle as prle
    keep = np.logical_or.reduce([prle.decode(m).astype(bool) for m in seg.instances.masks.rle])
    assert keep.any() and not keep.all() and np.array_equal(shown[1][1][~keep], img[~keep])
    print("CELLS 46 50 OK", len(got.instances), int(keep.sum()))
''')


def test_notebook_cells_46_and_50_run_on_this_module_through_the_references_display_iset(tmp_path):
    """Where the reference tree exists (skipped elsewhere, as in test_zero_edit.py): the source of notebook cells 33 - 40 (the reference's own
    loading of ground truth and predictions), then cells 46 and 50 unmodified with `analyze` = ampis_amd.analyze on the notebook's own polygon
    ground truth, drawn by the reference's visualize.display_iset on the façade (cell 50: apply_correction=True)."""
    if not os.path.isfile(os.path.join(REFERENCE, "colab", "AMPIS Tutorial.ipynb")):
        pytest.skip("the reference tree is not on this machine")
    from test_zero_edit import PREAMBLE
    os.symlink(REFERENCE, tmp_path / "AMPIS")
    script = f"ROOT = {ROOT!r}\nREFERENCE = {REFERENCE!r}\nWORK = {str(tmp_path)!r}\n" + PREAMBLE + NOTEBOOK_CELLS
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0 and "CELLS 46 50 OK" in r.stdout, (r.stdout[-1500:] + r.stderr[-4000:])
