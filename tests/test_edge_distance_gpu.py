"""mask_edge_distance on the device: amp_mask_edge_distance with a context (csrc/edge_distance.hip) against the reference's own vectors under
the exact rule of tests/test_edge_distance.py (every squared distance equal to rint(v^2) of the reference's value), against the host path on a
batch the fixture does not hold, twice for identical bytes, and through ampis_amd.analyze.mask_edge_distance(device='cuda')."""
import numpy as np
import pytest
import torch

from ampis_amd import analyze, rle
from ampis_amd._lib import lib

from edge_distance_cases import call_c, cases, check_case, untouched
from test_edge_distance import NAMES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES)
def test_device_path_gives_the_reference_squared_distances(gpu_ctx, name):
    check_case(name, ctx=gpu_ctx)


def _batch():
    """300 seeded pairs on 96 x 130 (not in the fixture): run lists and boxes from one pixel to beyond the image, some crops empty, some
    without any target pixel (the sentinel)."""
    r = np.random.default_rng(20240607)
    h, w = 96, 130
    yy, xx = np.ogrid[:h, :w]

    def blob(k):
        m = np.zeros((h, w), bool)
        for _ in range(k):
            m |= ((yy - r.integers(0, h)) / r.integers(2, 40)) ** 2 + ((xx - r.integers(0, w)) / r.integers(2, 50)) ** 2 <= 1.0
        return m
    gt = [blob(int(r.integers(1, 4))) for _ in range(40)]
    pred = [np.roll(g, (int(r.integers(-4, 5)), int(r.integers(-4, 5))), (0, 1)) ^ blob(1) for g in gt] + [blob(2) for _ in range(10)]
    pairs = np.stack([r.integers(0, len(gt), 300), r.integers(0, len(pred), 300)], axis=1)
    pairs[:40, 0] = pairs[:40, 1] = np.arange(40)
    boxes = np.zeros((300, 4), np.int64)
    for i in range(300):
        kind = i % 6
        if kind == 0:
            boxes[i] = (0, h, 0, w)
        elif kind == 1:
            boxes[i] = (0, 400, 0, 400)
        else:
            r1, c1 = int(r.integers(0, h)), int(r.integers(0, w))
            boxes[i] = (r1, r1 + int(r.choice([0, 1, 2, 31, 33, 63, 64, 65, 96])), c1, c1 + int(r.choice([0, 1, 5, 32, 63, 64, 65, 127, 130])))
    counts = lambda ms: [rle._counts(rle.encode(np.asfortranarray(m.astype(np.uint8)))) for m in ms]
    return counts(gt), counts(pred), pairs, boxes, h, w


def test_device_equals_host_element_for_element_and_repeats_its_bytes(gpu_ctx):
    gc, pc, pairs, boxes, h, w = _batch()
    cap = 300 * h * w
    host = call_c(None, gc, pc, pairs, boxes, h, w, cap, cap)
    dev = call_c(gpu_ctx, gc, pc, pairs, boxes, h, w, cap, cap)
    again = call_c(gpu_ctx, gc, pc, pairs, boxes, h, w, cap, cap)
    assert host[0] == 0 and dev[0] == 0 and again[0] == 0, lib().amp_last_error().decode()
    nfp, nfn = int(host[2][-1]), int(host[4][-1])
    assert nfp > 20000 and nfn > 20000                                            # the batch is not trivial ...
    assert (host[1][:nfp] == 0xFFFFFFFF).any() and (np.diff(host[2].astype(np.int64)) == 0).any()    # ... and holds sentinels and empty lists
    for a, b, c in zip(host[1:], dev[1:], again[1:]):
        assert np.array_equal(a, b)                                               # offsets, values and the untouched tails alike
        assert b.tobytes() == c.tobytes()


def test_device_path_through_the_public_function(gpu_ctx):
    for name in [n for n in NAMES if n.startswith("A/")]:
        c = cases()[name]
        fp, fn = analyze.mask_edge_distance(c["gt"], c["pred"], c["gt_box"], c["pred_box"], c["matches"], device="cuda")
        assert len(fp) == len(fn) == len(c["matches"])
        for got, d2 in zip(fp + fn, c["fp"] + c["fn"]):
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device.type == "cpu"
            assert got.numpy().tobytes() == np.sqrt(d2.astype(np.float64)).tobytes()
    c = cases()["A/indices_reused"]
    auto = analyze.mask_edge_distance(c["gt"], c["pred"], c["gt_box"], c["pred_box"], c["matches"], squared=True)     # 'auto': the device here
    assert all(np.array_equal(x.numpy(), d.astype(np.int64)) for x, d in zip(auto[0] + auto[1], c["fp"] + c["fn"]))


def test_device_path_errors_write_nothing(gpu_ctx):
    c = cases()["A/annulus_vs_disc"]
    gc, pc = [rle._counts(m) for m in c["gt"]], [rle._counts(m) for m in c["pred"]]
    h, w = c["size"]
    nfp, nfn = len(c["fp"][0]), len(c["fn"][0])
    st, fp, fpo, fn, fno = call_c(gpu_ctx, gc, pc, c["matches"], c["boxes"], h, w, nfp, nfn - 1)
    msg = lib().amp_last_error().decode()
    assert st != 0 and str(nfp) in msg and str(nfn) in msg and untouched(fp, fpo, fn, fno), msg
    bad = gc[0].copy()
    bad[0] += 7                                                                   # refused on the host, before any launch
    st, fp, fpo, fn, fno = call_c(gpu_ctx, [bad], pc, c["matches"], c["boxes"], h, w, nfp, nfn)
    assert st != 0 and "pair 0" in lib().amp_last_error().decode() and untouched(fp, fpo, fn, fno)
