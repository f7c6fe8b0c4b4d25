"""mask_edge_distance on the host (no GPU needed): amp_mask_edge_distance with a NULL context against the reference's own vectors and against
a numpy brute force over integer coordinates, and the public function ampis_amd.analyze.mask_edge_distance with device='cpu'.
The contract is the exact integer squared distance: the reference (torch.sqrt of exact integers, not always correctly rounded) is held to it
through rint(v^2), every value within 1e-6 of an integer (asserted when the fixture is made and again when it is loaded)."""
import numpy as np
import pytest
import torch

from ampis_amd import analyze, rle
from ampis_amd._lib import lib

from edge_distance_cases import call_c, cases, check_case, untouched

NAMES = ["A/identical", "A/pred_inside_gt", "A/corner_pixels", "A/annulus_vs_disc", "A/two_components", "A/staircase", "A/all_borders_full_box",
         "A/boxes_cut_masks", "A/box_beyond_image", "A/empty_crop", "A/indices_reused", "A/no_matches", "B/word_borders", "C/tall", "C/wide",
         "C/pixel_vs_square", "D/many_pairs", "E/large_offsets"]


def test_the_fixture_holds_the_cases_the_tests_name():
    assert sorted(cases()) == sorted(NAMES)
    c = cases()
    assert len(c["D/many_pairs"]["matches"]) == 320 and len(c["B/word_borders"]["matches"]) == 81 and len(c["A/no_matches"]["matches"]) == 0
    assert len(c["C/pixel_vs_square"]["fp"][0]) == 39999 and c["C/pixel_vs_square"]["fp"][0].max() == 2 * 199 * 199
    assert c["E/large_offsets"]["size"] == [1024, 1536]


@pytest.mark.parametrize("name", NAMES)
def test_host_path_gives_the_reference_squared_distances(name):
    check_case(name, ctx=None)


def brute(g, p, box):
    """Squared distances by exhaustive comparison of integer coordinates: (pred & ~gt) -> gt and (gt & ~pred) -> pred inside the crop."""
    r1, r2, c1, c2 = (int(v) for v in box)
    g, p = g[r1:r2, c1:c2].astype(bool), p[r1:r2, c1:c2].astype(bool)

    def one(q, t):
        qa, ta = np.argwhere(q & ~t).astype(np.int64), np.argwhere(t).astype(np.int64)         # argwhere: row-major, torch.where's order
        out = np.empty(len(qa), np.int64)
        for i in range(0, len(qa), 2048):                                                      # chunks: memory stays small
            d = qa[i:i + 2048, None, :] - ta[None, :, :]
            out[i:i + 2048] = (d * d).sum(axis=2).min(axis=1)
        return out.astype(np.uint32)
    return one(p, g), one(g, p)


@pytest.mark.parametrize("name", [n for n in NAMES if n[0] in "ABC"])
def test_host_path_agrees_with_a_brute_force_over_integer_coordinates(name):
    c = cases()[name]
    fp, fn = rle.edge_distance(c["gt"], c["pred"], c["matches"], c["boxes"])
    gd, pd = [rle.decode(m) for m in c["gt"]], [rle.decode(m) for m in c["pred"]]
    for k, ((g, p), box) in enumerate(zip(c["matches"].tolist(), c["boxes"])):
        bfp, bfn = brute(gd[g], pd[p], box)
        assert np.array_equal(fp[k], bfp) and np.array_equal(fn[k], bfn), (name, k)


def test_public_function_returns_the_reference_types_and_the_correctly_rounded_root():
    for name in ("A/indices_reused", "A/boxes_cut_masks", "A/box_beyond_image", "B/word_borders"):
        c = cases()[name]
        fp, fn = analyze.mask_edge_distance(c["gt"], c["pred"], c["gt_box"], c["pred_box"], c["matches"], device="cpu")
        assert isinstance(fp, list) and isinstance(fn, list) and len(fp) == len(fn) == len(c["matches"])
        for got, d2 in zip(fp + fn, c["fp"] + c["fn"]):
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device.type == "cpu" and got.ndim == 1
            assert got.numpy().tobytes() == np.sqrt(d2.astype(np.float64)).tobytes()                  # bit-equal to numpy's root of the integer
        sq_fp, sq_fn = analyze.mask_edge_distance(c["gt"], c["pred"], c["gt_box"], c["pred_box"], c["matches"], device="cpu", squared=True)
        for got, d2 in zip(sq_fp + sq_fn, c["fp"] + c["fn"]):
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), d2.astype(np.int64))


def test_public_function_with_no_matches_returns_two_empty_lists():
    c = cases()["A/no_matches"]
    assert analyze.mask_edge_distance(c["gt"], c["pred"], c["gt_box"], c["pred_box"], np.zeros((0, 2), int), device="cpu") == ([], [])


def test_boxes_none_means_the_tight_boxes_of_the_runs():
    c = cases()["D/many_pairs"]                                   # the fixture's boxes of this group are the tight ones, computed from the bitmaps
    a = analyze.mask_edge_distance(c["gt"], c["pred"], None, None, c["matches"], device="cpu", squared=True)
    b = analyze.mask_edge_distance(c["gt"], c["pred"], c["gt_box"], c["pred_box"], c["matches"], device="cpu", squared=True)
    assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert all(np.array_equal(x.numpy(), d.astype(np.int64)) for x, d in zip(a[0] + a[1], c["fp"] + c["fn"]))


def test_masks_are_accepted_as_bitmaps_too():
    c = cases()["A/indices_reused"]
    gd, pd = np.stack([rle.decode(m) for m in c["gt"]]).astype(bool), np.stack([rle.decode(m) for m in c["pred"]]).astype(bool)
    a = analyze.mask_edge_distance(gd, pd, c["gt_box"], c["pred_box"], c["matches"], device="cpu", squared=True)
    assert all(np.array_equal(x.numpy(), d.astype(np.int64)) for x, d in zip(a[0] + a[1], c["fp"] + c["fn"]))


def test_merge_boxes_is_the_union_box():
    assert analyze.merge_boxes([3, 9, 10, 12], np.array([5, 8, 2, 40])).tolist() == [3, 9, 2, 40]


@pytest.mark.parametrize("gt_box, pred_box, matches, word", [
    ([[1, 2, 3]], None, [[0, 0]], "gt_box[0]"),                              # not four values
    ([[1.5, 9, 3, 9]], None, [[0, 0]], "gt_box[0]"),                         # not integers
    (None, [[-1, 9, 3, 9]], [[0, 0]], "pred_box[0]"),                        # negative index
    (None, [[9, 8, 3, 9]], [[0, 0]], "pred_box[0]"),                         # r1 > r2
    ([[0, 9, 7, 3]], None, [[0, 0]], "gt_box[0]"),                           # c1 > c2
    (None, None, [[0, 1]], "matches[0]"),                                    # prediction index out of range
    (None, None, [[0, 0], [-1, 0]], "matches[1]"),                           # negative ground-truth index
])
def test_public_function_refuses_bad_arguments_naming_them(gt_box, pred_box, matches, word):
    c = cases()["A/boxes_cut_masks"]
    with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
        analyze.mask_edge_distance(c["gt"], c["pred"], gt_box, pred_box, np.array(matches), device="cpu")


def test_public_function_refuses_masks_of_different_sizes_and_unknown_devices():
    a, b = cases()["A/boxes_cut_masks"], cases()["C/tall"]
    with pytest.raises(ValueError, match="different sizes"):
        analyze.mask_edge_distance(a["gt"], b["pred"], None, None, np.array([[0, 0]]), device="cpu")
    with pytest.raises(ValueError, match="device"):
        analyze.mask_edge_distance(a["gt"], a["pred"], None, None, np.array([[0, 0]]), device="tpu")


def test_a_pair_without_a_target_pixel_in_its_box_raises_and_is_the_sentinel_in_c():
    g, p = np.zeros((20, 30), np.uint8), np.zeros((20, 30), np.uint8)
    g[2:5, 2:5] = 1
    p[10:14, 20:25] = 1
    gr, pr = [rle.encode(np.asfortranarray(g))], [rle.encode(np.asfortranarray(p))]
    box = [[8, 20, 15, 30]]                                        # holds the prediction only: its pixels have no ground truth to look for
    with pytest.raises(ValueError, match="pair 0"):
        analyze.mask_edge_distance(gr, pr, box, box, np.array([[0, 0]]), device="cpu")
    st, fp, fpo, fn, fno = call_c(None, [rle._counts(gr[0])], [rle._counts(pr[0])], [[0, 0]], box, 20, 30, 20, 9)
    assert st == 0 and fpo.tolist() == [0, 20] and fno.tolist() == [0, 0] and (fp[:20] == 0xFFFFFFFF).all()


def test_c_level_errors_write_nothing():
    c = cases()["A/annulus_vs_disc"]
    gc, pc = [rle._counts(m) for m in c["gt"]], [rle._counts(m) for m in c["pred"]]
    h, w = c["size"]
    nfp, nfn = len(c["fp"][0]), len(c["fn"][0])
    st, fp, fpo, fn, fno = call_c(None, gc, pc, c["matches"], c["boxes"], h, w, nfp, nfn)             # exactly enough
    assert st == 0 and np.array_equal(fp[:nfp], c["fp"][0]) and np.array_equal(fn[:nfn], c["fn"][0])
    for caps in ((nfp - 1, nfn), (nfp, nfn - 1)):                                                   # one short: an error that states the need
        st, fp, fpo, fn, fno = call_c(None, gc, pc, c["matches"], c["boxes"], h, w, *caps)
        msg = lib().amp_last_error().decode()
        assert st != 0 and str(nfp) in msg and str(nfn) in msg, msg
        assert untouched(fp, fpo, fn, fno)
    bad = gc[0].copy()
    bad[-1] += 1                                                                                    # runs that do not sum to h * w
    for g_runs in ([bad], [np.zeros(0, np.uint32)]):                                                # ... and an empty run list
        st, fp, fpo, fn, fno = call_c(None, g_runs, pc, c["matches"], c["boxes"], h, w, nfp, nfn)
        assert st != 0 and "pair 0" in lib().amp_last_error().decode()
        assert untouched(fp, fpo, fn, fno)
    st = call_c(None, gc, pc, [[0, 1]], c["boxes"], h, w, nfp, nfn)[0]                              # pair index out of range
    assert st != 0
    st = call_c(None, gc, pc, c["matches"], c["boxes"], 40000, w, nfp, nfn)[0]                      # beyond 32768: refused
    assert st != 0 and "32768" in lib().amp_last_error().decode()
