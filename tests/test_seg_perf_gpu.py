"""analyze.seg_perf_iset / seg_class_map on the device: device='cuda' and 'auto' against device='cpu' -- the same bytes -- on the reference-made
fixture inputs, on the micrograph with its polygon ground truth, on every kind of input and with nothing to do."""
import numpy as np
import pytest

from ampis_amd import analyze
from ampis_amd.structures import PolygonMasks

import seg_perf_data as data
from test_seg_perf import _counts, _toy

pytestmark = pytest.mark.gpu


def _same(a, b):
    return (_counts(a["masks"]) == _counts(b["masks"]) and a["pixel_counts"].tobytes() == b["pixel_counts"].tobytes()
            and a["labels"] == b["labels"] and np.array_equal(a["colors"], b["colors"]))


@pytest.mark.parametrize("mode", ("reduced", "all"))
def test_cuda_and_auto_equal_cpu_on_the_micrograph(gpu_ctx, mode):
    name = data.file_names()[0]
    polys, _, size = data.gt_polygons(name)
    pred, _ = data.pred_rles(name)
    gt = PolygonMasks(polys)
    match = analyze.rle_instance_matcher(gt, pred, size=size)
    cpu, cuda, auto = (analyze.seg_class_map(gt, pred, match, mode, size=size, device=d) for d in ("cpu", "cuda", "auto"))
    assert _same(cpu, cuda) and _same(cpu, auto) and len(match["tp"]) > 100 and int(cpu["pixel_counts"].sum()) == 1024 * 1536
    iset_c, (col_c, lab_c) = analyze.seg_perf_iset(gt, pred, mode=mode, size=size, device="cpu")
    iset_g, (col_g, lab_g) = analyze.seg_perf_iset(gt, pred, mode=mode, size=size, device="cuda")
    assert _counts(iset_c.instances.masks.rle) == _counts(iset_g.instances.masks.rle) == _counts(cpu["masks"])
    assert lab_c == lab_g and np.array_equal(col_c, col_g) and np.array_equal(iset_c.instances.boxes, iset_g.instances.boxes)


def test_small_inputs_and_nothing_to_do(gpu_ctx):
    g, p, gd, pd = _toy()
    for mode in ("reduced", "all"):
        cpu = analyze.seg_class_map(g, p, mode=mode, device="cpu")
        assert _same(cpu, analyze.seg_class_map(g, p, mode=mode, device="cuda"))
        assert _same(cpu, analyze.seg_class_map(np.stack(gd), np.stack(pd), mode=mode, device="auto"))
        for a, b in (([], p), (g, []), ([], [])):                                       # no pair: every class is background, on either path
            assert _same(analyze.seg_class_map(a, b, mode=mode, size=(20, 30), device="cpu"),
                         analyze.seg_class_map(a, b, mode=mode, size=(20, 30), device="cuda"))
