"""amp_render_instances on the device (csrc/render.hip): every case of tests/render_cases.py against the dense reference -- the untouched
Visualizer.draw_binary_mask / draw_box -- and against the host path, byte for byte; the device's bytes against its own second call; the refusals
(made before any device work); one 1024 x 1536 micrograph with 48 instances against the dense reference and with all 351 against the host."""
import numpy as np
import pytest

from ampis_amd import analyze, rle

import render_cases as rc
import seg_perf_data as data
from test_render import HOSTILE, check_box_outside_the_image_is_refused, check_hostile, raw_call

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", rc.HAND)
def test_device_equals_the_dense_reference_and_the_host(gpu_ctx, name):
    dev = rc.check_case(name, ctx=gpu_ctx)
    assert dev.tobytes() == rc.call(name).tobytes()


@pytest.mark.parametrize("chunk", range(8))
def test_device_equals_the_dense_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        dev = rc.check_case(f"seed_{i}", ctx=gpu_ctx)
        assert dev.tobytes() == rc.call(f"seed_{i}").tobytes(), i


@pytest.mark.parametrize("name", ["seam_edges", "more_than_64_instances", "order_4_forward"])
def test_device_equals_its_own_second_call(gpu_ctx, name):
    assert rc.call(name, gpu_ctx).tobytes() == rc.call(name, gpu_ctx).tobytes()


def test_in_place_call_on_the_device(gpu_ctx):
    c = rc.get("box_crossed_by_next_mask")
    st, out = raw_call(c["image"], [rle._counts(rc.enc(m)) for m in c["masks"]], colors=c["colors"], boxes=c["boxes"], lw=c["lw"], ctx=gpu_ctx,
                       in_place=True)
    assert st == 0 and out.tobytes() == rc.expected("box_crossed_by_next_mask").tobytes()


@pytest.mark.parametrize("what, kw", HOSTILE, ids=[f"{i}-{h[0][:24]}" for i, h in enumerate(HOSTILE)])
def test_hostile_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_hostile(what, kw, ctx=gpu_ctx)


def test_box_outside_the_image_is_refused_on_the_device_path(gpu_ctx):
    check_box_outside_the_image_is_refused(ctx=gpu_ctx)


def _micrograph(idx):
    _, boxes, size = data.gt_polygons(rc.MICROGRAPH)
    rles = data.gt_rles(rc.MICROGRAPH)
    assert size == data.SIZE and len(rles) == 351
    return [rles[i] for i in idx], boxes[idx], rc.micrograph_colors(len(idx))


def test_micrograph_subset_against_the_dense_reference(gpu_ctx):
    """1024 x 1536, the 48 instances of the golden file, boxes and a 3-pixel frame: device == host == the primitives"""
    from ampis_amd.utils.visualizer import Visualizer
    rles, boxes, cols = _micrograph(rc.micrograph_subset())
    img = rc.micrograph_image()
    tables, edge_rgb, ibox, box_rgb = analyze.render_inputs(cols, 0.4, boxes, *data.SIZE)
    dev = rle.render_instances(img, rles, tables, edge_rgb, ibox, box_rgb, 3, ctx=gpu_ctx)
    vis = Visualizer(img)
    for r, b, c in zip(rles, boxes, cols):
        vis.draw_binary_mask(rle.decode(r).astype(bool), c, alpha=0.4)
        vis.draw_box(b, c, line_width=3)
    assert dev.tobytes() == vis.output.img.tobytes()
    assert dev.tobytes() == rle.render_instances(img, rles, tables, edge_rgb, ibox, box_rgb, 3).tobytes()
    assert (dev != img).any(axis=2).sum() > 20000


def test_micrograph_with_all_instances_against_the_host(gpu_ctx):
    """1024 x 1536, all 351 ground-truth run lists with boxes: device against host and against its own second call (the dense reference takes
    seconds per dozen instances at this size)"""
    rles, boxes, cols = _micrograph(list(range(351)))
    img = rc.micrograph_image()
    dev = analyze.render_instances(img, rles, boxes, cols, device="cuda")
    assert dev.tobytes() == analyze.render_instances(img, rles, boxes, cols, device="cpu").tobytes()
    assert dev.tobytes() == analyze.render_instances(img, rles, boxes, cols, device="cuda").tobytes()
    assert (dev != img).any(axis=2).sum() > 100000
