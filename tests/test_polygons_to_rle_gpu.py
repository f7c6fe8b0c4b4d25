"""amp_polygons_to_rle on the device (csrc/polygon_runs.hip): the bytes of the host path (which tests/test_polygons_to_rle.py holds to the oracle and to
the per-polygon composition) and of the device's own second call, on every hand case, the seeded cases and both micrographs of
tests/polygon_cases.py; the refusals and the capacity protocol with a context; analyze.masks_to_rle / det_seg_scores on the device path.  No
tolerance anywhere."""
import numpy as np
import pytest

from ampis_amd import analyze, rle
from ampis_amd.structures import PolygonMasks

import polygon_cases as pc
import seg_perf_data as D
import test_polygons_to_rle as host

pytestmark = pytest.mark.gpu

CHUNK = 50


def same(a, b):
    return ([bytes(r["counts"]) for r in a[0]] == [bytes(r["counts"]) for r in b[0]] and [r["size"] for r in a[0]] == [r["size"] for r in b[0]]
            and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())


def device_equals_host(insts, h, w, ctx):
    want = rle.polygons_to_rle(insts, h, w, ctx=None, return_boxes=True)
    got = rle.polygons_to_rle(insts, h, w, ctx=ctx, return_boxes=True)
    again = rle.polygons_to_rle(insts, h, w, ctx=ctx, return_boxes=True)
    bad = [i for i in range(len(insts)) if bytes(got[0][i]["counts"]) != bytes(want[0][i]["counts"])]
    assert not bad, f"instances {bad[:8]} differ from the host"
    assert same(got, want) and same(again, got)
    return got


@pytest.mark.parametrize("name", host.HAND)
def test_hand_case_on_the_device_equals_the_host(gpu_ctx, name):
    h, w, insts = pc.all_cases()[name]
    got = device_equals_host(insts, h, w, gpu_ctx)
    assert [bytes(r["counts"]) for r in got[0]] == pc.references(name)[1]


@pytest.mark.parametrize("start", range(0, pc.SEEDS, CHUNK))
def test_seeded_cases_on_the_device_equal_the_host(gpu_ctx, start):
    for i in range(start, start + CHUNK):                                        # one call per seed: every image size, masks empty and not
        h, w, insts = pc.all_cases()[f"seed_{i}"]
        device_equals_host(insts, h, w, gpu_ctx)
    for size in pc.SEED_SIZES:                                                   # and the chunk's seeds of one size as the instances of one call
        insts = [pc.all_cases()[f"seed_{i}"][2][0] for i in range(start, start + CHUNK) if pc.SEED_SIZES[i % len(pc.SEED_SIZES)] == size]
        device_equals_host(insts, size[0], size[1], gpu_ctx)


@pytest.mark.parametrize("name", host.MICRO)
def test_micrograph_on_the_device_equals_the_host(gpu_ctx, name):
    h, w, insts = pc.all_cases()[name]
    got = device_equals_host(insts, h, w, gpu_ctx)
    assert [bytes(r["counts"]) for r in got[0]] == pc.references(name)[1]


@pytest.mark.parametrize("what,kw", host.REFUSALS, ids=[r[0] for r in host.REFUSALS])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    host.refusal(what, kw, gpu_ctx)


def test_capacity_protocol_on_the_device(gpu_ctx):
    host.capacity_protocol(gpu_ctx)


def test_only_empty_masks_on_the_device(gpu_ctx):
    insts = [[np.array([100.0, 100, 120, 100, 120, 120])], [np.array([3.0, 4])], [np.array([-9.0, -9, -5, -9, -5, -5]), np.array([70.0, 2, 75, 2, 75, 9])]]
    got = device_equals_host(insts, 37, 53, gpu_ctx)                             # not one crossing inside the image
    assert [rle.string_to_counts(r["counts"]).tolist() for r in got[0]] == [[37 * 53]] * 3 and not got[1].any() and not got[2].any()


def test_masks_to_rle_and_det_seg_scores_on_the_device_equal_the_host(gpu_ctx):
    fn = D.file_names()[1]
    polys, _, size = D.gt_polygons(fn)
    pred, _ = D.pred_rles(fn)
    on_dev, on_host = analyze.masks_to_rle(PolygonMasks(polys), size, device="cuda"), analyze.masks_to_rle(PolygonMasks(polys), size, device="cpu")
    assert [bytes(r["counts"]) for r in on_dev] == [bytes(r["counts"]) for r in on_host] == pc.references(fn)[1]
    s1 = analyze.det_seg_scores(PolygonMasks(polys), pred, size=size, device="cuda")
    s2 = analyze.det_seg_scores(PolygonMasks(polys), pred, size=size, device="cpu")
    assert s1.keys() == s2.keys()
    for k in s1:
        assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k])), k
