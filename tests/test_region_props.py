"""Region properties on the host (no GPU needed): amp_mask_region_props with a NULL context against tests/region_props_ref.py -- the 13 integers
and the box exactly, on hand-known shapes, degenerate masks, boxes that end before / on / after a 64-row word and 200 seeded blobs; the derived
floats of ampis_amd.analyze.region_properties against their exact-rational value within 8 ulp; the public functions and every refusal."""
import math
import types

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd._lib import AmpError, lib

import region_props_ref as ref


def _rles(masks):
    return [rle.encode(np.asfortranarray(m.astype(np.uint8))) for m in masks]


def check_integers(names, ctx=None):
    """amp_mask_region_props of the named cases in ONE call (ctx None: the host path) against the reference: box and 13 integers, exactly."""
    c = ref.cases()
    bbox, vals = rle.region_props(_rles([c[k][0] for k in names]), ctx=ctx)
    for k, b, v in zip(names, bbox.tolist(), vals.tolist()):
        assert tuple(b) == tuple(c[k][1]) and v == c[k][2], (k, b, c[k][1], v, c[k][2])


@pytest.mark.parametrize("name", ref.NAMED)
def test_host_integers_equal_the_reference(name):
    check_integers([name])


def test_host_integers_equal_the_reference_on_the_blob_batch():
    check_integers([k for k in ref.cases() if k.startswith("blob/")])


LIMITS = [(32768, 32768), (2, 32768), (32768, 3)]


def check_full_image_at_the_limits(h, w, ctx=None):
    """One run covering an h x w image: every sum in closed form (sum r c and sum r^2 reach 2^58 at 32768 x 32768), the frame as border --
    all of it class 1 -- and the image as its own hull.  The widest box there is: 65537 points per hull chain."""
    bbox, vals = rle.region_props([{"size": [h, w], "counts": np.array([0, h * w], np.uint32)}], ctx=ctx)
    sq = lambda k: k * (k + 1) * (2 * k + 1) // 6
    assert bbox.tolist() == [[0, 0, h, w]]
    assert vals[0].tolist() == [h * w, w * h * (h - 1) // 2, h * w * (w - 1) // 2, w * sq(h - 1), (h * (h - 1) // 2) * (w * (w - 1) // 2), h * sq(w - 1),
                                2 * h + 2 * w - 4, 0, 0, h * w, 0, 0, 0]


@pytest.mark.parametrize("h, w", LIMITS)
def test_host_full_image_at_the_size_limits(h, w):
    check_full_image_at_the_limits(h, w)


def test_hand_known_answers():
    t = analyze.region_properties(np.stack([ref.cases()[k][0] for k in ref.HAND]), keys=list(analyze.RPROPS_KEYS), device="cpu")
    assert t["area"].tolist() == [1, 23, 20, 9]
    assert t["perimeter"].tolist() == [0.0, 21.0, 18 * math.sqrt(2.0), 8.0]
    assert t["convex_area"].tolist()[:3] == [1, 23, 20]
    assert t["major_axis_length"][0] == 0.0 and t["minor_axis_length"][0] == 0.0 and t["orientation"][0] == math.pi / 4
    assert t["major_axis_length"][1] == 4 * math.sqrt(44.0) and t["minor_axis_length"][1] == 0.0
    c = ref.cases()
    assert c["row_1x23"][2][6:9] == [21, 0, 0] and c["diagonal_20"][2][6:9] == [0, 18, 0]        # the reference agrees with the literals


def test_integer_hull_rule_equals_the_qhull_formulation():
    differ = [k for k, (m, _, v) in ref.cases().items() if ref.convex_area_qhull(m) != v[9]]
    assert not differ, differ


def test_empty_mask_columns():
    t = analyze.region_properties(np.zeros((1, 12, 9), bool), keys=list(analyze.RPROPS_KEYS), device="cpu")
    for k in ("area", "perimeter", "convex_area", "equivalent_diameter", "bbox-0", "bbox-1", "bbox-2", "bbox-3"):
        assert t[k][0] == 0, k
    for k in ("centroid-0", "centroid-1", "eccentricity", "extent", "major_axis_length", "minor_axis_length", "orientation", "solidity"):
        assert np.isnan(t[k][0]), k


def test_derived_floats_are_within_8_ulp_of_the_exact_value():
    worst = {}
    for name, (_, bbox, vals) in ref.cases().items():
        got, exact = analyze.region_floats(bbox, vals), ref.exact_floats(bbox, vals)
        for k in ref.FLOAT_KEYS:
            if exact[k] is None:
                assert math.isnan(got[k]), (name, k)
                continue
            err, bound = ref.float_error(k, got[k], exact[k])
            assert err <= bound, (name, k, got[k], exact[k])
            if bound:
                worst[k] = max(worst.get(k, 0.0), float(err / bound) * 8)
    print("worst error in ulp (orientation: in units of 2^-52):", {k: round(v, 2) for k, v in worst.items()})


def test_public_table_columns_types_and_default_keys():
    masks = np.stack([ref.cases()[k][0] for k in ("hole", "two_parts")])
    t = analyze.region_properties(masks, device="cpu")
    assert list(t) == ["area", "equivalent_diameter", "major_axis_length", "perimeter", "solidity", "orientation"]
    t = analyze.region_properties(_rles(masks), keys=["bbox", "centroid", "area", "extent", "bbox_area"], device="cpu")
    assert list(t) == ["bbox-0", "bbox-1", "bbox-2", "bbox-3", "centroid-0", "centroid-1", "area", "extent", "bbox_area"]
    assert all(v.shape == (2,) for v in t.values()) and t["area"].dtype == np.int64 and t["extent"].dtype == np.float64
    assert [t[f"bbox-{i}"][0] for i in range(4)] == [5, 8, 30, 40] and t["bbox_area"][0] == 25 * 32
    assert t["area"][0] == 25 * 32 - 8 * 13 - 1 and t["extent"][0] == t["area"][0] / (25 * 32)
    assert analyze.region_properties([], device="cpu")["area"].shape == (0,)


def test_refusals():
    m = np.ones((1, 6, 7), bool)
    with pytest.raises(ValueError, match="'feret_diameter_max'"):
        analyze.region_properties(m, keys=["area", "feret_diameter_max"], device="no such device")      # the key is looked at first
    with pytest.raises(ValueError, match="device"):
        analyze.region_properties(m, device="tpu")
    with pytest.raises(ValueError, match="different sizes"):
        analyze.region_properties(_rles([np.ones((6, 7), bool), np.ones((7, 6), bool)]), device="cpu")
    with pytest.raises(ValueError, match="2-D integer"):
        analyze.regionprops_table(np.zeros((4, 4)), ["area"])


@pytest.mark.parametrize("counts, size, what", [([5, 10, 20], (6, 7), "cover 35 pixels"), ([40, 10], (6, 7), "more than"), ([], (6, 7), "empty run list"),
                                                ([0, 42], (6, 70000), "image size"), ([0], (0, 5), "image size")])
def test_malformed_run_lists_are_argument_errors(counts, size, what):
    with pytest.raises(AmpError, match=what):
        rle.region_props([{"size": list(size), "counts": np.array(counts, dtype=np.uint32)}])
    assert what in lib().amp_last_error().decode()


def test_compute_rprops_on_a_stand_in_instance_set():
    masks = np.stack([ref.cases()[k][0] for k in ("square_3x3", "hole", "row_1x23")])
    iset = types.SimpleNamespace(instances=types.SimpleNamespace(masks=_rles(masks), image_size=masks.shape[1:], class_idx=np.array([0, 1, 0])), rprops=None)
    assert analyze.compute_rprops(iset, device="cpu") is None
    df = iset.rprops
    assert list(df.columns) == analyze.RPROPS_DEFAULT_KEYS + ["class_idx"] and len(df) == 3
    assert df["area"].tolist() == [9, 25 * 32 - 8 * 13 - 1, 23] and df["class_idx"].tolist() == [0, 1, 0] and df["perimeter"][0] == 8.0
    back = analyze.compute_rprops(iset, keys=["area", "centroid"], return_df=True, device="cpu")
    assert back is iset.rprops and list(back.columns) == ["area", "centroid-0", "centroid-1", "class_idx"] and back["centroid-0"][0] == 21.0


def test_regionprops_table_on_a_three_label_image():
    c = ref.cases()
    lab = np.zeros((40, 50), np.int32)
    lab[c["two_parts"][0]] = 7
    lab[c["square_3x3"][0]] = 2
    lab[c["row_1x23"][0]] = 4
    t = analyze.regionprops_table(lab, ["area", "bbox", "perimeter", "convex_area"])
    masks = [lab == v for v in (2, 4, 7)]            # ascending labels
    want = [ref.ref_integers(m) for m in masks]
    assert t["area"].tolist() == [w[1][0] for w in want] and t["convex_area"].tolist() == [w[1][9] for w in want]
    assert [[int(t[f"bbox-{i}"][k]) for i in range(4)] for k in range(3)] == [list(w[0]) for w in want]
    assert t["perimeter"].tolist() == [analyze.region_floats(*w)["perimeter"] for w in want]
    assert analyze.regionprops_table(np.zeros((5, 5), int), ["area"])["area"].shape == (0,)
