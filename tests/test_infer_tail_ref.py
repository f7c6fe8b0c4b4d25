"""CPU tests of tests/infer_tail_ref.py, the NumPy references tests/test_infer_tail_gpu.py holds the inference tail's kernels to:
paste_ref against the oracle's detector_postprocess / paste_mask (F.grid_sample) on every paste case of the device tests, paste_path's
report of the data path each case reaches, and box_candidates_ref against the oracle's box inference before NMS."""
import functools

import numpy as np
import pytest
import torch

import infer_tail_ref as R
from oracle import maskrcnn as O, rle as orle

F32 = np.float32
MAX_TIE_PIXELS = 4         # pixels, over the whole case list, where the oracle's sample lies within 1e-6 of the threshold


def _oracle_flips(prob, box, out_hw, in_hw, thr):
    """paste_ref against detector_postprocess for one detection.  Asserts the box and the validity; returns the number of mask pixels
    that differ, every one of them proved to lie within 1e-6 of the threshold in the oracle's own sample (paste_prob)."""
    H, W = int(out_hw[0]), int(out_hw[1])
    ob, valid, mask = R.paste_ref(prob, box, out_hw, in_hw, thr)
    cfg = O.Cfg(mask_threshold=thr)
    b, _, _, masks, _ = O.detector_postprocess(torch.from_numpy(np.asarray(box, F32)[None]), torch.ones(1), torch.zeros(1, dtype=torch.int64),
                                               torch.from_numpy(prob[None]), (int(in_hw[0]), int(in_hw[1])), H, W, cfg)
    assert valid == (len(b) == 1)
    if not valid:
        assert not mask.any()
        return 0
    assert np.array_equal(ob.view(np.uint32), b[0].numpy().view(np.uint32))
    ref = masks[0].numpy()
    ys, xs = np.nonzero(mask != ref)
    if len(ys):
        pm, y0, x0 = O.paste_prob(torch.from_numpy(prob), b[0], H, W)
        margin = np.abs(pm.numpy()[ys - y0, xs - x0] - thr)
        assert margin.max() < 1e-6, float(margin.max())
    # the run lengths of the reference mask are a whole encoding of the image
    runs = orle.encode_counts(mask)
    assert int(runs.sum()) == H * W and np.array_equal(orle.decode_counts(runs, H, W), mask)
    return len(ys)


@functools.lru_cache(maxsize=None)
def _case_flips(i):
    prob, boxes, hw, thr = R.paste_case_inputs(i)
    return sum(_oracle_flips(prob[j], boxes[j], hw, hw, thr) for j in range(2))


@pytest.mark.parametrize("i", range(len(R.PASTE_CASES)), ids=R.PASTE_IDS)
def test_paste_ref_matches_the_oracle(i):
    assert _case_flips(i) <= MAX_TIE_PIXELS


@functools.lru_cache(maxsize=None)
def _multi_flips():
    m = R.multi_image_case()
    total = 0
    for in_hw in (m["in_hw"], np.array([m["in_common"]] * 3)):
        for i in range(len(m["prob"])):
            b = m["batch"][i]
            total += _oracle_flips(m["prob"][i], m["boxes"][i], m["out_hw"][b], in_hw[b], 0.5)
    return total


def test_paste_ref_matches_the_oracle_on_scaled_images():
    assert _multi_flips() <= MAX_TIE_PIXELS
    m = R.multi_image_case()
    _, valid, _ = R.paste_many_ref(m["prob"], m["boxes"], m["batch"], m["out_hw"], m["in_hw"], 0.5)
    assert 0 < valid.sum() < len(valid)           # the launch holds a detection that is empty after the clip
    assert any(h * m["in_hw"][b][1] != w * m["in_hw"][b][0] for b, (h, w) in enumerate(m["out_hw"]))     # sx != sy


def test_tie_pixels_over_the_whole_case_list():
    total = sum(_case_flips(i) for i in range(len(R.PASTE_CASES))) + _multi_flips()
    print("pixels that differ from the oracle's paste over all cases:", total)
    assert total <= MAX_TIE_PIXELS


@pytest.mark.parametrize("i", range(len(R.PASTE_CASES)), ids=R.PASTE_IDS)
def test_paste_path_reports_the_path_each_case_is_named_for(i):
    name, hw, box, thr, nxy, path = R.PASTE_CASES[i]
    _, valid, reg = R.paste_region(np.asarray(box, F32), hw, hw)
    if nxy is None:
        assert not valid
        return
    nx, ny = reg[2] - reg[0], reg[3] - reg[1]
    assert (nx, ny) == nxy
    p = R.paste_path(nx, ny)
    assert p["path"] == path
    assert p["nseg"] * p["SEG"] >= ny > (p["nseg"] - 1) * p["SEG"]
    if path == "a":
        assert p["SEG"] <= 32 and p["keep_bits"]
    elif path == "b":
        assert 32 < p["SEG"] <= 64 and p["keep_bits"] and p["units"] <= R.MAX_UNITS
    elif path == "c":
        assert p["SEG"] > 64 and not p["keep_bits"] and p["units"] <= R.MAX_UNITS
    else:
        assert nx > R.MAX_UNITS and p["nseg"] == 1 and p["units"] == nx and not p["keep_bits"]


def test_paste_path_of_the_table():
    want = {"small": (31, 4), "b": (39, 13), "b_wrap": (39, 13), "c": (75, 7), "c_wrap": (76, 7), "d": (20, 1), "d_wrap": (24, 1),
            "tall": (32, 131)}
    for name, hw, box, thr, nxy, path in R.PASTE_CASES:
        if name in want:
            p = R.paste_path(*nxy)
            assert (p["SEG"], p["nseg"]) == want[name], (name, p)


def test_wrap_and_closing_cases_are_what_they_are_named_for():
    reg = {c[0]: R.paste_region(np.asarray(c[2], F32), c[1], c[1])[2] for c in R.PASTE_CASES if c[4] is not None}
    hw = {c[0]: c[1] for c in R.PASTE_CASES}
    for name in ("b_wrap", "c_wrap", "d_wrap", "thr0_all"):         # full-height columns
        assert reg[name][1] == 0 and reg[name][3] == hw[name][0]
    for name in ("bottom", "bottom_b", "bottom_c"):                  # bottom on H, top > 1, right of the region inside the image
        assert reg[name][1] > 0 and reg[name][3] == hw[name][0] and reg[name][2] < hw[name][1]
    for name in ("right", "corner"):
        assert reg[name][2] == hw[name][1]
    assert reg["corner"][3] == hw["corner"][0] and reg["corner"][1] > 0


def test_threshold_extremes():
    prob, boxes, hw, _ = R.paste_case_inputs(R.PASTE_IDS.index("thr0_all"))
    for j in range(2):
        assert list(orle.encode_counts(R.paste_ref(prob[j], boxes[j], hw, hw, 0.0)[2])) == [0, hw[0] * hw[1]]
        assert list(orle.encode_counts(R.paste_ref(prob[j], boxes[j], hw, hw, 1.5)[2])) == [hw[0] * hw[1]]


# ---- the detection tail ----
def _all_box_cases():
    return [R.box_case(n) for n in R.BOX_CASES] + [R.nonfinite_case()[0], R.overflow_case()]


BOX_IDS = list(R.BOX_CASES) + ["nonfinite", "overflow"]


@pytest.mark.parametrize("ci", range(len(BOX_IDS)), ids=BOX_IDS)
def test_box_candidates_ref_matches_the_oracle_before_nms(ci):
    c = _all_box_cases()[ci]
    K = c["K"]
    ref = R.box_candidates_ref(c["pred"], c["props"], c["counts"], K, c["thr"], c["img_hw"])
    cfg = O.Cfg(num_classes=K, score_thresh=c["thr"], nms_thresh=2.0, detections_per_image=-1)      # IoU <= 1: nothing is suppressed
    for b, r in enumerate(ref):
        n = int(c["counts"][b])
        # membership in the candidate set is no rounding question
        live = r["probs"][r["finite"]]
        assert live.size == 0 or np.abs(live - c["thr"]).min() > 1e-5
        rows = torch.from_numpy(c["pred"][b, :n])
        ob, os_, oc = O.box_inference_single(rows[:, :K + 1], rows[:, K + 1:K + 1 + 4 * K], torch.from_numpy(c["props"][b, :n]),
                                             tuple(int(v) for v in c["img_hw"][b]), cfg)
        assert len(os_) == len(r["cand"])
        if not r["cand"]:
            continue
        idx = np.array([p for p, _ in r["cand"]])
        sc, bx, cl = r["probs"].reshape(-1)[idx], r["boxes"].reshape(-1, 4)[idx], np.array([k for _, k in r["cand"]])
        order = np.argsort(-sc, kind="stable")
        assert np.array_equal(cl[order], oc.numpy())
        assert np.abs(sc[order] - os_.numpy()).max() < 2e-6
        assert np.abs(bx[order] - ob.numpy()).max() < 2e-4


def test_nonfinite_rows_are_no_candidates():
    c, bad = R.nonfinite_case()
    ref = R.box_candidates_ref(c["pred"], c["props"], c["counts"], c["K"], c["thr"], c["img_hw"])
    for b, r in bad:
        assert not ref[b]["finite"][r]
        assert all(p // c["K"] != r for p, _ in ref[b]["cand"])
    # their neighbours are candidates: the filter drops rows, not waves
    for b, r in bad:
        assert any(p // c["K"] in (r - 1, r + 1) for p, _ in ref[b]["cand"])


def test_overflow_case_overflows_one_image_only():
    c = R.overflow_case()
    ref = R.box_candidates_ref(c["pred"], c["props"], c["counts"], c["K"], c["thr"], c["img_hw"])
    assert len(ref[0]["cand"]) > 300 and 0 < len(ref[1]["cand"]) < c["ccap"]


def test_box_cases_cover_what_they_are_meant_to():
    c = R.box_case("k3")
    assert c["counts"][1] == 0 and 0 < c["counts"][2] < c["pred"].shape[1]
    assert c["pred"].shape[1] % 64 != 0                                   # waves straddle images
    assert R.box_case("k1_wide_ld")["pred"].shape[2] > 5 * 1 + 1
    s = R.box_case("sized")
    ref = R.box_candidates_ref(s["pred"], s["props"], s["counts"], s["K"], s["thr"], s["img_hw"])
    other = R.box_candidates_ref(s["pred"], s["props"], s["counts"], s["K"], s["thr"], np.array([s["hw"]] * 3))
    for b in (1, 2):                                                      # the per-image size does change the clip
        assert np.nanmax(np.abs(ref[b]["boxes"] - other[b]["boxes"])) > 1.0


def test_sortkey_decoder_inverts_make_sortkey():
    rng = np.random.default_rng(3)
    score = rng.uniform(0, 1, 50).astype(F32)
    pos, cat = rng.integers(0, 1 << 24, 50), rng.integers(0, 256, 50)
    u = score.view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000).astype(np.uint64)          # make_sortkeys, test_rpn_nms_levels_gpu.py
    keys = (o << np.uint64(32)) | ((np.uint64(0xffffff) - pos.astype(np.uint64)) << np.uint64(8)) | cat.astype(np.uint64)
    s, p, k, used = R.decode_sortkeys(np.concatenate([keys, np.zeros(1, np.uint64)]).view(np.int64))
    assert np.array_equal(s[:-1], score) and np.array_equal(p[:-1], pos) and np.array_equal(k[:-1], cat)
    assert used[:-1].all() and not used[-1]


def test_plain_indexing_refs():
    rng = np.random.default_rng(4)
    B, cap, D = 2, 9, 4
    sb, ss, sc = rng.normal(size=(B, cap, 4)).astype(F32), rng.normal(size=(B, cap)).astype(F32), rng.integers(0, 5, (B, cap)).astype(np.int32)
    keep = np.array([[3, 1, 8, 0], [2, 2, 2, 2]])
    ob, os_, oc, op = R.gather_dets_ref(sb, ss, sc, keep, np.array([3, 0]), D, payload=sc + 10)
    assert np.array_equal(ob[0, :3], sb[0, [3, 1, 8]]) and not ob[0, 3:].any() and not ob[1].any() and not os_[1].any()
    assert list(oc[0]) == list(sc[0, [3, 1, 8]]) + [-1] and list(op[0]) == list(sc[0, [3, 1, 8]] + 10) + [-1] and (oc[1] == -1).all()
    cb, cs, cc, cbatch = R.compact_dets_ref(np.array([3, 9]), ob, os_, oc)
    assert list(cbatch) == [0, 0, 0, 1, 1, 1, 1] and np.array_equal(cs, np.concatenate([os_[0, :3], os_[1]]))
    assert np.array_equal(cb[:3], ob[0, :3]) and np.array_equal(cc[3:], oc[1])


def test_mask_prob_ref():
    x = np.zeros((2, 28, 28, 3), F32)
    x[0, :, :, 1], x[1, :, :, 0] = 30, -30
    p = R.mask_prob_ref(x, [1, 7])                                        # class 7 is outside [0, 3): channel 0
    assert np.allclose(p[0], 1 / (1 + np.exp(-30.0)), rtol=0, atol=1e-15) and np.allclose(p[1], 1 / (1 + np.exp(30.0)), rtol=0, atol=1e-15)
