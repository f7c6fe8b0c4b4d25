"""The shared case set of the run-list layer (tests/run_list_cases.py) through the host paths of all four mask analyses, against the dense
references the project already has: tests/region_props_ref.py, tests/seg_class_ref.py, the brute forces of tests/test_edge_distance.py and
tests/rle_overlap_cases.py.  Every comparison is exact.  Then the refusals of the shared walk, once per entry point."""
import numpy as np
import pytest

import region_props_ref
import rle_overlap_cases
import seg_class_ref
from ampis_amd._lib import AmpError, lib
from run_list_cases import ENTRY_POINTS, FAULTS, SIZES, dense, masks, pairs_and_boxes, run_all
from test_edge_distance import brute as edge_brute


def edge_reference(g, p, box):
    """test_edge_distance.brute, with the C ABI's 0xffffffff where the target mask has no pixel in the crop"""
    r1, r2, c1, c2 = (int(v) for v in box)
    gc, pc = g[r1:r2, c1:c2], p[r1:r2, c1:c2]
    if gc.any() and pc.any():
        return edge_brute(g, p, box)
    none = lambda q, t: np.full(0 if t.any() else int(q.sum()), 0xFFFFFFFF, np.uint32)      # one side is empty: its pixels are no queries
    return none(pc, gc), none(gc, pc)


@pytest.mark.parametrize("h, w", SIZES)
def test_host_paths_equal_the_dense_references(h, w):
    gt, pred = masks(h, w)
    assert len(gt) <= 6 and len(pred) <= 6
    G, P = [dense(m) for m in gt], [dense(m) for m in pred]
    pairs, boxes = pairs_and_boxes(gt, pred)
    got = run_all(gt, pred)
    # mask_edge_distance
    fpo, fno, fp, fn = got["edge"]
    for k, ((g, q), box) in enumerate(zip(pairs.tolist(), np.minimum(boxes, [h, h, w, w]))):
        wfp, wfn = edge_reference(G[g], P[q], box)
        assert np.array_equal(fp[int(fpo[k]): int(fpo[k + 1])], wfp) and np.array_equal(fn[int(fno[k]): int(fno[k + 1])], wfn), (k, g, q, box)
    # region properties
    bbox, vals = got["props"]
    for i, m in enumerate(G + P):
        wb, wv = region_props_ref.ref_integers(m)
        assert tuple(bbox[i].tolist()) == tuple(wb) and vals[i].tolist() == wv, i
    # group overlap: the group (gt, pred) and the group (pred, gt)
    n = 2
    inter, aa, ab = got["overlap"][:n], got["overlap"][n: 2 * n], got["overlap"][2 * n:]
    for k, (a, b) in enumerate(((G, P), (P, G))):
        assert np.array_equal(inter[k], rle_overlap_cases.brute(a, b))
        assert aa[k].tolist() == [int(m.sum()) for m in a] and ab[k].tolist() == [int(m.sum()) for m in b]
    # segmentation class map
    for mode in ("reduced", "all"):
        want_counts, want_px, _ = seg_class_ref.dense(gt, pred, pairs, mode, (h, w))
        counts, px = got["seg-" + mode][:-1], got["seg-" + mode][-1]
        assert len(counts) == len(want_counts) and all(np.array_equal(a, b) for a, b in zip(counts, want_counts))
        assert np.array_equal(px, want_px)


def test_the_case_set_holds_the_shapes_it_promises():
    gt, pred = masks(129, 5)
    G, P = [dense(m) for m in gt], [dense(m) for m in pred]
    assert len(gt) == 6 and len(pred) == 5
    assert not G[0].any() and G[1].all() and G[2].sum() == 1 and G[2][63, 4] and P[0].sum() == 1 and P[0][64, 0]
    assert G[3][128, 0] and G[3][0, 1] and G[3].sum() == 2                       # a run across a column end
    assert G[4][:, 1].all() and G[4].sum() == 2 * 129 + 1                        # more than one full column
    assert gt[5]["counts"][0] == 0 and 0 in gt[5]["counts"][1:-1].tolist()       # zero-length runs, leading and interior
    assert (G[2] & P[1]).sum() == 1 and P[1].sum() == 2                          # exactly one common pixel


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_every_entry_point_refuses_what_the_shared_walk_refuses(entry, fault):
    bad, what = FAULTS[fault]
    with pytest.raises(AmpError, match=what.replace("(", r"\(")):
        ENTRY_POINTS[entry](bad, None)
    assert what in lib().amp_last_error().decode()
