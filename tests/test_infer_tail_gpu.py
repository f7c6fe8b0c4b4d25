"""The inference tail's kernels (csrc/mask_paste.hip: mask_prob_kernel, paste_rle_seg_kernel; csrc/box_infer.hip: box_candidates_kernel,
gather_dets_kernel, compact_dets_kernel) through their C entry points against the NumPy references of tests/infer_tail_ref.py, which
tests/test_infer_tail_ref.py proves against the oracle on the CPU.

Paste: the run lengths of every mask equal the reference's, np.array_equal, on every data path of paste_rle_seg_kernel (the table in
infer_tail_ref.PASTE_CASES: segments of <= 32 rows, of 33..64 rows with the bits kept, of > 64 rows evaluated twice, and more than
MAX_UNITS columns), with and without full-height (wrapping) columns, on every closing transition, at the threshold extremes, for
several images of different sizes in one launch, with per-image input sizes, with a separate position pool and with a pool that is
too small.  The detection tail: bit patterns for the two gathers, 1e-6 for the sigmoid, and for box_candidates the candidate SET
(the reference scores keep 1e-5 away from the threshold) with scores to 2e-6 and boxes to 2e-4 px (the bounds of
test_stages_gpu.py::test_box_inference_chain, same coordinate scale)."""
import functools

import numpy as np
import pytest
import torch

import infer_tail_ref as R
from oracle import rle as orle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(a):
    return torch.tensor(np.asarray(a).tolist(), dtype=torch.int32, device=DEV)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ paste
@functools.lru_cache(maxsize=None)
def _paste_case_ref(i):
    prob, boxes, hw, thr = R.paste_case_inputs(i)
    obs, valid, masks = R.paste_many_ref(prob, boxes, np.zeros(2, np.int32), [hw], hw, thr)
    return obs, valid, [orle.encode_counts(m) for m in masks]


def _check_paste(got, ref, out_hw, batch, fitted=None):
    """got = (out_boxes, valid, runs) of ops.paste_rle, ref = (out_boxes, valid, run lists); fitted: the masks whose runs are compared
    (None: all)."""
    ob, valid, runs = got[:3]
    robs, rvalid, rruns = ref
    assert np.array_equal(_bits(ob), _bits(robs))
    assert np.array_equal(valid.cpu().numpy().astype(bool), rvalid)
    for j in range(len(rvalid)):
        if not rvalid[j]:
            assert len(runs[j]) == 0
            continue
        if fitted is not None and not fitted[j]:
            continue
        H, W = out_hw[batch[j]]
        assert int(runs[j].astype(np.int64).sum()) == int(H) * int(W), j
        assert np.array_equal(runs[j], rruns[j]), (j, len(runs[j]), len(rruns[j]))


@pytest.mark.parametrize("i", range(len(R.PASTE_CASES)), ids=R.PASTE_IDS)
def test_paste_runs_equal_the_reference_on_every_path(gpu_ctx, i):
    from ampis_amd import ops
    name, hw, box, thr, nxy, path = R.PASTE_CASES[i]
    prob, boxes, _, _ = R.paste_case_inputs(i)
    H, W = hw
    ref = _paste_case_ref(i)
    if nxy is not None:                       # the case reaches the path it is named for
        _, _, reg = R.paste_region(boxes[0], hw, hw)
        assert (reg[2] - reg[0], reg[3] - reg[1]) == nxy and R.paste_path(*nxy)["path"] == path
    got = ops.paste_rle(gpu_ctx, _dev(prob), _dev(boxes), _i32([0, 0]), _i32([H]), _i32([W]), H, W, threshold=thr)
    _check_paste(got, ref, [hw], [0, 0])
    if name == "thr0_all":
        assert all(list(r) == [0, H * W] for r in got[2])
    if name in ("thr15", "thr15_all"):
        assert all(list(r) == [H * W] for r in got[2])
    if name == "empty":
        assert not ref[1].any()
    elif thr == 0.5:
        assert len(ref[2][1]) > 4 * len(ref[2][0]) or nxy == (3, 3)       # the noise mask does have many runs


@functools.lru_cache(maxsize=None)
def _multi_ref(per_image):
    m = R.multi_image_case()
    in_hw = m["in_hw"] if per_image else np.array(m["in_common"])
    obs, valid, masks = R.paste_many_ref(m["prob"], m["boxes"], m["batch"], m["out_hw"], in_hw, 0.5)
    return obs, valid, [orle.encode_counts(k) for k in masks]


def _multi_launch(ctx, per_image, **kw):
    from ampis_amd import ops
    m = R.multi_image_case()
    return ops.paste_rle(ctx, _dev(m["prob"]), _dev(m["boxes"]), _dev(m["batch"]), _i32(m["out_hw"][:, 0]), _i32(m["out_hw"][:, 1]),
                         m["in_common"][0], m["in_common"][1], in_hw=_dev(m["in_hw"]) if per_image else None, return_pool=True, **kw)


def _dense(off, ln, used):
    """the masks with runs tile [0, used) of the pool without a gap"""
    idx = [i for i in np.argsort(off, kind="stable") if ln[i] > 0]
    end = 0
    for i in idx:
        if int(off[i]) != end:
            return False
        end += int(ln[i])
    return end == used


@pytest.mark.parametrize("mode", ["scalar_in", "per_image_in", "pos_scratch"])
def test_paste_three_images_of_different_sizes_in_one_launch(gpu_ctx, mode):
    m = R.multi_image_case()
    per_image = mode != "scalar_in"
    ref = _multi_ref(per_image)
    got = _multi_launch(gpu_ctx, per_image, pos_scratch=mode == "pos_scratch")
    _check_paste(got, ref, m["out_hw"], m["batch"])
    info = got[-1]
    lens = np.array([len(r) if v else 0 for r, v in zip(ref[2], ref[1])])
    assert np.array_equal(info["len"], lens)
    if mode == "pos_scratch":           # the pool holds the run lengths only
        assert info["used"] == lens.sum() and info["pos_used"] == (lens[lens > 0] - 1).sum()
        assert _dense(info["off"], info["len"], info["used"])
    else:                               # T + 1 run lengths and the T positions they are made from
        assert info["used"] == (2 * lens[lens > 0] - 1).sum()
    if mode == "per_image_in":          # the per-image input size does change the masks
        other = _multi_ref(False)
        assert any(not np.array_equal(a, b) for a, b in zip(ref[2], other[2]))


@pytest.mark.parametrize("pos_scratch", [False, True])
def test_paste_pool_overflow_is_flagged_and_leaves_the_fitting_masks_exact(gpu_ctx, pos_scratch):
    m = R.multi_image_case()
    ref = _multi_ref(True)
    lens = np.array([len(r) if v else 0 for r, v in zip(ref[2], ref[1])])
    need = lens.sum() if pos_scratch else (2 * lens[lens > 0] - 1).sum()
    cap = int(need) // 2
    assert cap > lens.max()
    got = _multi_launch(gpu_ctx, True, pos_scratch=pos_scratch, pool_counts=cap, return_overflow=True)
    overflow, info = got[3], got[4]
    assert overflow == 1
    fitted = info["len"] > 0
    assert (ref[1] & ~fitted).any()                       # a valid mask did not fit
    assert not (fitted & ~ref[1]).any()
    _check_paste(got, ref, m["out_hw"], m["batch"], fitted=fitted)       # valid and out_boxes are unaffected; the masks that fitted are exact
    for j in np.nonzero(fitted)[0]:
        span = int(info["len"][j]) if pos_scratch else 2 * int(info["len"][j]) - 1
        assert int(info["off"][j]) + span <= cap
        assert info["len"][j] == lens[j]
    assert info["used"] == need                           # every mask asked for its room, fitting or not


# ------------------------------------------------------------------------------------------------------------------ mask_prob
def _logits(N, K, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 4, (N, R.MS, R.MS, K)).astype(F32)
    flat = x.reshape(-1)
    flat[::7], flat[3::11], flat[5::13] = 30.0, -30.0, 0.0
    return x


@pytest.mark.parametrize("N,K", [(1, 1), (3, 3), (100, 80)])
def test_mask_prob_is_the_sigmoid_of_the_class_channel(gpu_ctx, N, K):
    from ampis_amd import ops
    x = _logits(N, K, 30 + N)
    classes = np.random.default_rng(N).integers(0, K, N).astype(np.int32)
    classes[-1] = K - 1
    got = ops.mask_prob(gpu_ctx, _dev(x), _dev(classes)).cpu().numpy()
    ref = R.mask_prob_ref(x, classes)
    err = np.abs(got - ref).max()
    print(f"mask_prob N={N} K={K}: max |d| = {err:.3g}")
    assert err <= 1e-6
    picked = x[np.arange(N), :, :, classes]
    assert (picked == 30).any() and (picked == -30).any() and (picked == 0).any()
    assert np.all(got[picked == 0] == 0.5)


def test_mask_prob_reads_channel_0_for_a_class_outside_the_range(gpu_ctx):
    """include/ampis_hip.h, amp_mask_prob: a class outside [0, K) (the -1 of an unused detection row) reads channel 0."""
    from ampis_amd import ops
    N, K = 5, 3
    x = _logits(N, K, 41)
    classes = np.array([-1, K, 2, 1 << 20, -(1 << 31)], np.int32)
    got = ops.mask_prob(gpu_ctx, _dev(x), _dev(classes)).cpu().numpy()
    zero = ops.mask_prob(gpu_ctx, _dev(x), _dev(np.array([0, 0, 2, 0, 0], np.int32))).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(zero))
    assert np.abs(got - R.mask_prob_ref(x, classes)).max() <= 1e-6
    assert np.abs(got[0] - R.mask_prob_ref(x, [1])[0]).max() > 0.1         # and not another channel


# ------------------------------------------------------------------------------------------------------------------ gather_dets / compact_dets
def _pattern(rng, shape):
    """float32 of arbitrary bit patterns (NaNs and denormals included): a gather moves bits"""
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(F32)


@pytest.mark.parametrize("with_payload", [False, True], ids=["no_payload", "payload"])
@pytest.mark.parametrize("D", [1, 50])
def test_gather_dets_moves_bits_and_blanks_the_rest(gpu_ctx, D, with_payload):
    from ampis_amd import ops
    rng = np.random.default_rng(50 + D)
    B, cap = 3, 64
    sb, ss = _pattern(rng, (B, cap, 4)), _pattern(rng, (B, cap))
    sc = rng.integers(0, 80, (B, cap)).astype(np.int32)
    pay = rng.integers(0, 1 << 20, (B, cap)).astype(np.int32) if with_payload else None
    keep = rng.integers(0, cap, (B, D)).astype(np.int32)           # the entries from keep_count on are valid positions that must not be used
    count = np.array([0, 1, D], np.int32)
    db, ds, dc, po = ops.gather_dets(gpu_ctx, _dev(sb), _dev(ss), _dev(sc), _dev(keep), _dev(count), payload=_dev(pay) if with_payload else None)
    torch.cuda.synchronize()
    rb, rs, rc, rp = R.gather_dets_ref(sb, ss, sc, keep, count, D, payload=pay)
    assert np.array_equal(_bits(db), _bits(rb)) and np.array_equal(_bits(ds), _bits(rs))
    assert np.array_equal(dc.cpu().numpy(), rc)
    assert (po is None) == (rp is None)
    if with_payload:
        assert np.array_equal(po.cpu().numpy(), rp)
    # spelled out: rows at and beyond the count are zeros, class (and payload) -1
    for b in range(B):
        assert not _bits(db)[b, count[b]:].any() and not _bits(ds)[b, count[b]:].any()
        assert (dc.cpu().numpy()[b, count[b]:] == -1).all()
        if with_payload:
            assert (po.cpu().numpy()[b, count[b]:] == -1).all()


def test_compact_dets_packs_the_clamped_counts_and_touches_nothing_else(gpu_ctx):
    from ampis_amd import ops
    rng = np.random.default_rng(60)
    B, D = 4, 100
    count = np.array([0, D, D + 7, 1], np.int32)                    # the third is clamped to D
    boxes, scores = _pattern(rng, (B, D, 4)), _pattern(rng, (B, D))
    classes = rng.integers(-1, 80, (B, D)).astype(np.int32)
    SENT = 0x5a5a5a5a
    out = (torch.full((B * D, 4), SENT, dtype=torch.int32, device=DEV).view(torch.float32),
           torch.full((B * D,), SENT, dtype=torch.int32, device=DEV).view(torch.float32),
           torch.full((B * D,), SENT, dtype=torch.int32, device=DEV), torch.full((B * D,), SENT, dtype=torch.int32, device=DEV))
    ob, os_, oc, obatch = ops.compact_dets(gpu_ctx, _dev(count), _dev(boxes), _dev(scores), _dev(classes), out=out)
    torch.cuda.synchronize()
    rb, rs, rc, rbatch = R.compact_dets_ref(count, boxes, scores, classes)
    total = 2 * D + 1
    assert len(rs) == total
    assert np.array_equal(_bits(ob)[:total], _bits(rb)) and np.array_equal(_bits(os_)[:total], _bits(rs))
    assert np.array_equal(oc.cpu().numpy()[:total], rc) and np.array_equal(obatch.cpu().numpy()[:total], rbatch)
    for t in (ob, os_, oc, obatch):                                 # rows beyond the total are untouched
        assert (_bits(t)[total:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------------ box_candidates
def _run_box(ctx, c, ccap=8192):
    from ampis_amd import ops
    dense, keys, cnt, ovf = ops.box_candidates(ctx, _dev(c["pred"]), _dev(c["props"]), _dev(c["counts"]), c["K"], c["thr"], c["hw"][0], c["hw"][1],
                                               ccap=ccap, img_hw=_dev(c["img_hw"]) if c["sized"] else None)
    torch.cuda.synchronize()
    return dense.cpu().numpy(), keys.cpu().numpy(), cnt.cpu().numpy(), int(ovf.item())


def _ref_box(c):
    return R.box_candidates_ref(c["pred"], c["props"], c["counts"], c["K"], c["thr"], c["img_hw"])


def _check_image_complete(c, r, dense_b, keys_b, cnt_b, tag):
    """One image whose candidates all fit: the keys written are exactly the reference set, scores and boxes within the bounds."""
    K = c["K"]
    score, pos, cat, used = R.decode_sortkeys(keys_b)
    n = len(r["cand"])
    assert cnt_b == n, (tag, cnt_b, n)
    assert used[:n].all() and not used[n:].any(), tag                # compacted: the first cand_count slots and no other
    got = list(zip(pos[:n].tolist(), cat[:n].tolist()))
    assert len(set(got)) == n and set(got) == set(r["cand"]), tag
    if n:
        err = np.abs(score[:n].astype(np.float64) - r["probs"].reshape(-1)[pos[:n]]).max()
        print(f"{tag}: {n} candidates, max score |d| = {err:.3g}")
        assert err < 2e-6, tag
    rows = r["finite"]
    if rows.any():
        d = dense_b.reshape(-1, K, 4)[rows].astype(np.float64)
        berr = np.abs(d - r["boxes"][rows]).max()
        print(f"{tag}: {int(rows.sum())} rows, max box |d| = {berr:.3g} px")
        assert berr < 2e-4, tag


@pytest.mark.parametrize("name", list(R.BOX_CASES))
def test_box_candidates_writes_the_reference_set(gpu_ctx, name):
    c = R.box_case(name)
    ref = _ref_box(c)
    dense, keys, cnt, ovf = _run_box(gpu_ctx, c)
    assert ovf == 0
    for b, r in enumerate(ref):
        _check_image_complete(c, r, dense[b], keys[b], cnt[b], f"{name}[{b}]")
    assert sum(len(r["cand"]) for r in ref) > 20
    if name == "k3":
        assert cnt[1] == 0 and not keys[1].any()                     # prop_count == 0


def test_box_candidates_drops_rows_that_are_not_finite(gpu_ctx):
    c, bad = R.nonfinite_case()
    ref = _ref_box(c)
    dense, keys, cnt, ovf = _run_box(gpu_ctx, c)
    assert ovf == 0
    for b, r in enumerate(ref):
        _check_image_complete(c, r, dense[b], keys[b], cnt[b], f"nonfinite[{b}]")
    for b, row in bad:                                               # spelled out: absent for all K classes
        _, pos, _, used = R.decode_sortkeys(keys[b])
        assert not (pos[used] // c["K"] == row).any()


def test_box_candidates_overflow_keeps_the_true_count(gpu_ctx):
    c = R.overflow_case()
    ref = _ref_box(c)
    ccap = c["ccap"]
    assert len(ref[0]["cand"]) > 300 and len(ref[1]["cand"]) < ccap
    dense, keys, cnt, ovf = _run_box(gpu_ctx, c, ccap=ccap)
    assert ovf == 1
    assert cnt[0] == len(ref[0]["cand"])                             # the model's score-floor bisection reads cand_count[b] > ccap
    score, pos, cat, used = R.decode_sortkeys(keys[0])
    assert used.all()                                                # all 64 slots hold distinct members of the reference set
    got = list(zip(pos.tolist(), cat.tolist()))
    assert len(set(got)) == ccap and set(got) <= set(ref[0]["cand"])
    assert np.abs(score.astype(np.float64) - ref[0]["probs"].reshape(-1)[pos]).max() < 2e-6
    _check_image_complete(c, ref[1], dense[1], keys[1], cnt[1], "overflow[1]")
