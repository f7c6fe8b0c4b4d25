"""Region properties on the device: amp_mask_region_props with a context (csrc/region_props.hip) against tests/region_props_ref.py on every case
of tests/test_region_props.py (integers exact), against the host path byte for byte on the 200-mask batch and on the 351 polygons of a
1024 x 1536 micrograph, twice for identical bytes, through ampis_amd.analyze.region_properties(device='cuda'), and with nothing to do."""
import json
import os

import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd.structures import PolygonMasks

import region_props_ref as ref
from test_region_props import LIMITS, _rles, check_full_image_at_the_limits, check_integers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ref.NAMED)
def test_device_integers_equal_the_reference(gpu_ctx, name):
    check_integers([name], ctx=gpu_ctx)


def test_device_equals_reference_and_host_on_the_blob_batch_and_repeats_its_bytes(gpu_ctx):
    names = [k for k in ref.cases() if k.startswith("blob/")]
    check_integers(names, ctx=gpu_ctx)
    rles = _rles([ref.cases()[k][0] for k in names])
    host, dev, again = rle.region_props(rles), rle.region_props(rles, ctx=gpu_ctx), rle.region_props(rles, ctx=gpu_ctx)
    for a, b, c in zip(host, dev, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_all_named_cases_in_one_call_with_mixed_sizes_of_box(gpu_ctx):
    # one image size per call: the 40 x 50 cases together -- empty, full-image and one-pixel masks share the launches
    names = [k for k in ref.NAMED if ref.cases()[k][0].shape == (40, 50)]
    check_integers(names, ctx=gpu_ctx)


@pytest.mark.parametrize("h, w", LIMITS)
def test_device_full_image_at_the_size_limits(gpu_ctx, h, w):
    check_full_image_at_the_limits(h, w, ctx=gpu_ctx)


def _via_polygons():
    root = os.path.dirname(os.path.abspath(__file__))
    via = json.load(open(os.path.join(root, "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    return PolygonMasks(polys), (h, w)


def test_micrograph_polygons_device_equals_host(gpu_ctx):
    polys, size = _via_polygons()
    rles = analyze.masks_to_rle(polys, size)
    assert size == (1024, 1536) and len(rles) == 351
    host, dev = rle.region_props(rles), rle.region_props(rles, ctx=gpu_ctx)
    assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes()
    assert (host[1][:, 0] > 0).sum() > 300 and int(host[1][:, 9].min()) >= 0 and (host[1][:, 9] >= host[1][:, 0]).all()     # hull >= area
    keys = list(analyze.RPROPS_KEYS)
    cpu, gpu = analyze.region_properties(polys, keys, size=size, device="cpu"), analyze.region_properties(polys, keys, size=size, device="cuda")
    assert list(cpu) == list(gpu) and all(cpu[k].tobytes() == gpu[k].tobytes() for k in cpu)


def test_public_function_on_the_device_is_bit_identical_to_the_host(gpu_ctx):
    masks = np.stack(ref.blob_batch()[:40])
    keys = list(analyze.RPROPS_KEYS)
    cpu, gpu, auto = (analyze.region_properties(masks, keys, device=d) for d in ("cpu", "cuda", "auto"))
    for k in cpu:
        assert cpu[k].dtype == gpu[k].dtype and cpu[k].tobytes() == gpu[k].tobytes() == auto[k].tobytes(), k


def test_nothing_to_do(gpu_ctx):
    bbox, vals = rle.region_props([], ctx=gpu_ctx)
    assert bbox.shape == (0, 4) and vals.shape == (0, 13)
    bbox, vals = rle.region_props(_rles([np.zeros((33, 17), bool)] * 5), ctx=gpu_ctx)
    assert not bbox.any() and not vals.any() and vals.shape == (5, 13)
    t = analyze.region_properties(np.zeros((2, 33, 17), bool), ["area", "solidity"], device="cuda")
    assert t["area"].tolist() == [0, 0] and np.isnan(t["solidity"]).all()
