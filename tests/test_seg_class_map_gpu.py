"""amp_seg_class_map on the device (csrc/seg_class_map.hip): every case of tests/seg_class_cases.py in both modes against the dense reference
and against the host path, byte for byte; one micrograph with all its matched pairs; the device's bytes against its own second call; the
refusals (made before any device work)."""
import numpy as np
import pytest

from ampis_amd import analyze, rle

import seg_class_cases as cs
import seg_class_ref as ref
import seg_perf_data as data
from test_seg_class_map import HOSTILE, check_full_image_at_the_size_limit, check_hostile, raw_call

pytestmark = pytest.mark.gpu


def _bytes(res):
    return [c.tobytes() for c in res[0]] + [res[1].tobytes()]


@pytest.mark.parametrize("mode", cs.MODES)
@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_dense_reference_and_the_host(gpu_ctx, name, mode):
    dev = cs.check_case(name, mode, ctx=gpu_ctx)
    assert _bytes(dev) == _bytes(cs.check_case(name, mode))


@pytest.mark.parametrize("chunk", range(8))
def test_device_equals_the_dense_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        for mode in cs.MODES:
            dev = cs.check_case(f"seed_{i}", mode, ctx=gpu_ctx)
            assert _bytes(dev) == _bytes(cs.check_case(f"seed_{i}", mode)), (i, mode)


def test_raw_bytes_of_the_device_equal_the_host(gpu_ctx):
    host = raw_call([[0, 4, 2]], [[2, 3, 1]], [(0, 0)], 2, 3, mode=1)
    dev = raw_call([[0, 4, 2]], [[2, 3, 1]], [(0, 0)], 2, 3, mode=1, ctx=gpu_ctx)
    assert host[0] == dev[0] == 0 and dev[2].tolist() == [0, 3, 6, 7, 10, 11, 12, 13]
    assert all(h.tobytes() == d.tobytes() for h, d in zip(host[1:], dev[1:]))         # the words behind the result are untouched on both paths


@pytest.mark.parametrize("mode", cs.MODES)
def test_micrograph_with_all_matched_pairs(gpu_ctx, mode):
    """1024 x 1536, the 351 VIA polygons against the 257 committed predictions, every matched pair: the device against the dense reference
    (three planes built pair by pair), against the host and against its own second call"""
    name = "Sc1Tile_001-002-000_0-000.png"
    gt, (pred, _) = data.gt_rles(name), data.pred_rles(name)
    pairs = analyze.rle_instance_matcher(gt, pred)["tp"]
    assert len(gt) == 351 and len(pred) == 257 and len(pairs) > 150
    dev = rle.seg_class_map(gt, pred, pairs, mode, ctx=gpu_ctx)
    want, want_px, _ = ref.dense(gt, pred, pairs, mode, data.SIZE)
    assert [c.tobytes() for c in dev[0]] == [c.astype(np.uint32).tobytes() for c in want] and dev[1].tolist() == want_px.tolist()
    assert _bytes(dev) == _bytes(rle.seg_class_map(gt, pred, pairs, mode)) == _bytes(rle.seg_class_map(gt, pred, pairs, mode, ctx=gpu_ctx))
    assert dev[1][1] > 100000 and dev[1][2] > 0 and dev[1][4] > 0


def test_device_full_image_at_the_size_limit(gpu_ctx):
    check_full_image_at_the_size_limit(ctx=gpu_ctx)


@pytest.mark.parametrize("status, what, kw", HOSTILE, ids=[f"{i}-{h[1][:24]}" for i, h in enumerate(HOSTILE)])
def test_hostile_arguments_are_refused_before_any_device_work(gpu_ctx, status, what, kw):
    check_hostile(status, what, kw, ctx=gpu_ctx)
