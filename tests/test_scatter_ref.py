"""CPU checks on the references and case tables of tests/scatter_ref.py (no GPU): the float64 sum against float64 autograd of the oracle's
differentiable RoIAlign and as the adjoint of the forward reference, the fp32-ordered reference against the float64 sum on the NARROW class
(bit for bit: the class is order-free), every seeded defect caught by the families built for it, and every case's own premise."""
import numpy as np
import pytest
import torch

import proposal_ref as PR
import scatter_ref as S

F32 = np.float32
U = 2.0 ** -24
CASES = S.roi_cases()
NARROW = [n for n, c in CASES.items() if c["cls"] == "narrow"]
WIDE = [n for n, c in CASES.items() if c["cls"] == "wide"]
KEEP = 3                      # channels kept where a check is per channel anyway

# which families catch which seeded defect (every listed pair is asserted; test_every_defect_is_caught needs one family per defect at least)
CATCHES = {
    "drop_top_clamp": ("edge-p7", "maps-ragged-p7", "maps-multiples-p14", "whole-p5-one-bin", "taps-128-y", "taps-128-x"),
    "skip_upper_tap": ("edge-p7", "maps-ragged-p7", "tile-ownership", "bin-slots-p16-narrow", "p1", "wide-p7", "c4", "taps-280px-y"),
    "reverse_roi_order": ("same-box-100", "130-rois-one-tile-wide", "wide-p7", "wide-p14"),
    "footprint_minus_one": ("tile-ownership", "maps-ragged-p7", "edge-p7"),
    "first_64_rois_only": ("130-rois-one-tile-narrow", "130-rois-one-tile-wide", "same-box-100"),
    "bins_capped_at_14": ("bin-slots-p15-narrow", "bin-slots-p15-wide", "bin-slots-p16-narrow", "bin-slots-p16-wide", "bin-slots-p17-narrow"),
}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def few(c):
    """the case with KEEP channels (every check below is per channel)"""
    d = dict(c)
    d["dout"] = np.ascontiguousarray(c["dout"][..., :KEEP])
    d["maps"] = [np.ascontiguousarray(m[..., :KEEP]) for m in c["maps"]]
    return d


def ref(c, **kw):
    return S.roi_align_bwd_ref(c["maps"], c["rois"], c["bidx"], c["P"], c["levels"], c["dout"], **kw)


def sum64(c):
    return S.roi_align_bwd_sum64([m.shape for m in c["maps"]], c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])


def grids(c):
    """largest sampling grid of the case per axis"""
    g = [1, 1]
    for r, lv in zip(c["rois"], c["levels"]):
        if np.isfinite(r).all():
            ys, xs = PR.roi_samples(r, c["P"], S.STRIDES[lv], *c["hw"][lv])
            if ys is not None:
                g = [max(g[0], ys.shape[1]), max(g[1], xs.shape[1])]
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_sum64_equals_float64_autograd(name):
    """roi_align_bwd_sum64 against torch autograd of oracle.train.roi_align_torch on float64 maps.  The oracle's tap weights are fp32 products
    hy * hx summed in float64, the reference's the fp32 running sums wy, wx multiplied in float64: both within (gh + gw) * 2^-24 of the exact
    weight, relative, which is the bound; on NARROW cases every weight is exact and the two must agree to the last float64 bit."""
    from oracle import train as T
    c = few(CASES[name])
    bi = np.zeros(len(c["rois"]), np.int64) if c["bidx"] is None else c["bidx"]
    maps = [torch.zeros(m.shape, dtype=torch.float64).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in c["maps"]]
    loss = torch.zeros((), dtype=torch.float64)
    with np.errstate(invalid="ignore"):
        for r in range(len(c["rois"])):
            if not np.isfinite(c["rois"][r]).all():
                continue                                      # (int(ceil(NaN)) has no meaning in the oracle either)
            lv = int(c["levels"][r])
            out = T.roi_align_torch(maps[lv][int(bi[r])], torch.from_numpy(c["rois"][r:r + 1]), c["P"], 1.0 / S.STRIDES[lv])
            loss = loss + (out[0] * torch.from_numpy(c["dout"][r].astype(np.float64)).permute(2, 0, 1)).sum()
    if loss.requires_grad:
        loss.backward()
    gh, gw = grids(c)
    for l, (s, sa, cnt) in enumerate(sum64(c)):
        want = np.zeros(s.shape) if maps[l].grad is None else maps[l].grad.permute(0, 2, 3, 1).numpy()
        if c["cls"] == "narrow":
            assert np.array_equal(s, want), (name, l)
        else:
            assert (np.abs(s - want) <= (gh + gw + 2) * U * sa + 1e-300).all(), (name, l, float(np.abs(s - want).max()))


@pytest.mark.parametrize("name", ["maps-ragged-p7", "tile-ownership", "whole-p5-bins-of-8", "bin-slots-p16-narrow", "edge-p7", "wide-p7", "p1-wide"])
def test_sum64_is_the_adjoint_of_the_forward_reference(name):
    """<roi_align_ref(x), g> == <x, bwd(g)>: exactly on NARROW cases (x of small integers: the forward is exact there too), on WIDE ones within the
    fp32 roundings of the forward (4 * gh * gw products and sums per bin) and of the weights"""
    c = few(CASES[name])
    rng = np.random.default_rng(3)
    x = [S.ints(rng, -4, 4, m.shape) if c["cls"] == "narrow" else rng.standard_normal(m.shape, dtype=F32) for m in c["maps"]]
    bi = np.zeros(len(c["rois"]), np.int64) if c["bidx"] is None else c["bidx"]
    ok = np.isfinite(c["rois"]).all(1)
    fwd = PR.roi_align_ref(x, c["rois"][ok], bi[ok], c["P"], c["levels"][ok]).astype(np.float64)
    lhs = float((fwd * c["dout"][ok].astype(np.float64)).sum())
    sums = sum64(c)
    rhs = float(sum((xm.astype(np.float64) * s).sum() for xm, (s, _, _) in zip(x, sums)))
    if c["cls"] == "narrow":
        assert lhs == rhs, (name, lhs, rhs)
    else:
        gh, gw = grids(c)
        scale = float(sum((np.abs(xm.astype(np.float64)) * sa).sum() for xm, (_, sa, _) in zip(x, sums)))
        assert abs(lhs - rhs) <= (4 * gh * gw + gh + gw + 4) * U * scale, (name, lhs, rhs, scale)


@pytest.mark.parametrize("name", NARROW)
def test_narrow_class_is_order_free(name):
    """narrow_premise asserts the class from the inputs (gh * gw powers of two, sum |terms| + |preset| < 2^24 units per cell); then the fp32-ordered
    reference equals the float64 sum bit for bit, accumulating and with init, and in the reverse RoI order as well (KEEP channels here; the GPU
    test asserts the premise over all of them before it launches)"""
    c = few(CASES[name])
    want = S.narrow_premise(c["maps"], c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])
    got = ref(c)
    rev = ref(c, defect="reverse_roi_order")
    zero = [np.zeros_like(m) for m in c["maps"]]
    want0 = S.narrow_premise(zero, c["rois"], c["bidx"], c["P"], c["levels"], c["dout"])
    got0 = ref(c, init=True)
    for l in range(4):
        assert np.array_equal(got[l].astype(np.float64), want[l]) and np.array_equal(bits(got[l]), bits(want[l].astype(F32))), (name, l)
        assert np.array_equal(bits(rev[l]), bits(got[l])), (name, l)
        assert np.array_equal(bits(got0[l]), bits(want0[l].astype(F32))), (name, l)


@pytest.mark.parametrize("defect", S.ROI_DEFECTS)
def test_every_defect_is_caught(defect):
    assert CATCHES[defect]
    for name in CATCHES[defect]:
        c = few(CASES[name])
        good, bad = ref(c), ref(c, defect=defect)
        n = sum(int((bits(g) != bits(b)).sum()) for g, b in zip(good, bad))
        print(f"{defect} on {name}: {n} words differ")
        assert n > 0, (defect, name)


def test_defects_the_other_families_cannot_see():
    """what makes the families necessary: 14 bins are not cut at P = 14, 64 RoIs fit one ballot trip, and no seeded defect changes an empty case"""
    c = few(CASES["bin-slots-p14-wide"])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref(c), ref(c, defect="bins_capped_at_14")))
    c = few(CASES["wide-p7"])                                  # 60 RoIs
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref(c), ref(c, defect="first_64_rois_only")))
    c = few(CASES["empty-only"])
    for d in S.ROI_DEFECTS:
        assert all(np.array_equal(bits(a), bits(m)) for a, m in zip(ref(c, defect=d), c["maps"]))


# ---- premises of the cases ----------------------------------------------------------------------------------------------------------
def test_every_case_has_its_levels_decided():
    for name, c in CASES.items():
        lv, decided = PR.level_ref(c["rois"])
        assert decided.all() and (lv == c["levels"]).all(), name


def test_edge_table_lands_on_its_targets():
    """the samples exactly on -1, 0, H - 1 and H, one step below -1 and one above H, per level and axis (the table of the forward, P = 7)"""
    c = CASES["edge-p7"]
    assert len(c["rois"]) == len(PR.ROI_EDGE) + len(S.EMPTY_ROIS) and set(np.unique(c["bidx"])) == {0, 1}
    for roi, tgt in zip(PR.ROI_EDGE, PR.ROI_EDGE_TARGETS):
        if tgt is None:
            continue
        lv, axis, tag = tgt
        ys, xs = PR.roi_samples(roi, 7, S.STRIDES[lv], *PR.MAP_HW[lv])
        for ax, v in (("y", ys), ("x", xs)):
            if axis in (ax, "both"):
                assert (v == PR.roi_edge_target_value(lv, ax, tag)).any(), (lv, axis, tag)


def test_empty_rois_are_empty():
    c = CASES["empty-only"]
    assert all(cnt.sum() == 0 for _, _, cnt in sum64(few(c)))
    assert np.isnan(c["rois"]).any(1).sum() == 1


def _rows_cols(c, r):
    """rows and columns of non-zero weight of RoI r"""
    lv = int(c["levels"][r])
    WY, WX, _ = S._roi_weights(c["rois"][r], c["P"], lv, *c["hw"][lv], None)
    return np.flatnonzero((WY != 0).any(0)), np.flatnonzero((WX != 0).any(0))


def test_tile_ownership_premises():
    c = CASES["tile-ownership"]
    fp = {n: _rows_cols(c, i) for i, n in enumerate(c["tile_names"])}
    y, x = fp["straddles-corner"]
    assert y[0] < 4 <= y[-1] and x[0] < 4 <= x[-1]
    for n in ("last-row-is-tile-first", "last-row-on-tile-first-exactly"):
        assert fp[n][0][-1] % 4 == 0 and fp[n][0][0] // 4 == fp[n][0][-1] // 4 - 1, (n, fp[n][0])
    for n in ("last-col-is-tile-first", "last-col-on-tile-first-exactly"):
        assert fp[n][1][-1] % 4 == 0 and fp[n][1][0] // 4 == fp[n][1][-1] // 4 - 1, (n, fp[n][1])
    # ... exactly: the last sample sits on the row itself, so the row above it (the kernel's conservative footprint) has no weight
    i = c["tile_names"].index("last-row-on-tile-first-exactly")
    ys, _ = PR.roi_samples(c["rois"][i], 7, 4, *c["hw"][0])
    assert ys.max() == F32(8.0)
    assert fp["first-row-is-tile-last"][0][0] % 4 == 3 and fp["first-col-is-tile-last"][1][0] % 4 == 3
    y, x = fp["both-ends"]
    assert y[0] % 4 == 3 and x[0] % 4 == 3
    for name, P, bigger in (("whole-p5-one-bin", 1, 16), ("whole-p5-bins-of-8", 7, 8)):
        c = CASES[name]
        H, W = c["hw"][3]
        for r in range(len(c["rois"])):
            y, x = _rows_cols(c, r)
            assert (y[0], y[-1], x[0], x[-1]) == (0, H - 1, 0, W - 1), name              # the whole coarsest map
            ys, _ = PR.roi_samples(c["rois"][r], P, 32, H, W)
            assert ys[0, -1] - ys[0, 0] > 4 and bigger > 4                               # one bin larger than a tile


def test_bin_slot_premises():
    """under one cell a side, inside one tile; at P = 16 the kernel's bin range (restated from roi_align_bwd_tile_kernel) is all 16 slots"""
    for P in (14, 15, 16, 17):
        c = CASES["bin-slots-p%d-narrow" % P]
        for r in range(len(c["rois"])):
            y, x = _rows_cols(c, r)
            assert y[0] // 4 == y[-1] // 4 and x[0] // 4 == x[-1] // 4
            sc = F32(1) / F32(4)
            sh = c["rois"][r][1] * sc - F32(0.5)
            rh = (c["rois"][r][3] * sc - F32(0.5)) - sh
            assert 0 < rh < 1
            if P == 16:
                bh, ty0 = rh / F32(P), 4 * (y[0] // 4)
                lo = max(0, int(np.floor((F32(ty0 - 1) - sh) / bh)) - 1)
                hi = min(P - 1, int(np.floor((F32(ty0 + 4) - sh) / bh)) + 1)
                assert (lo, hi) == (0, 15)


def test_roi_loop_premises():
    c = CASES["130-rois-one-tile-narrow"]
    assert (c["bidx"] == 1).sum() == 130 and (c["bidx"] == 0).sum() == 5
    one = np.flatnonzero(c["bidx"] == 1)
    assert one[-1] - one[0] + 1 > 128 and (c["bidx"][one[0]:one[-1]] == 0).any()            # three trips of 64; foreign RoIs inside the range
    tiles = {(frozenset(y // 4), frozenset(x // 4)) for y, x in (_rows_cols(c, r) for r in range(135))}
    assert len(tiles) == 1 and all(len(t) == 1 for t in tiles.pop())
    c = CASES["image-without-rois"]
    assert c["B"] == 3 and set(np.unique(c["bidx"])) == {0, 2}
    assert CASES["batch-idx-none"]["bidx"] is None
    c = CASES["same-box-100"]
    assert (c["rois"] == c["rois"][0]).all() and len(c["rois"]) == 100


def test_wide_grids_round():
    """the WIDE cases hold grids of 3 and 5 samples (inv = 1 / 9, 1 / 15, 1 / 25 is no fp32 number)"""
    seen = set()
    for name in ("wide-p7", "wide-p14"):
        c = CASES[name]
        for r, lv in zip(c["rois"], c["levels"]):
            ys, xs = PR.roi_samples(r, c["P"], S.STRIDES[lv], *c["hw"][lv])
            seen |= {ys.shape[1], xs.shape[1]}
    assert {3, 5} <= seen


def test_tap_branch_premises():
    """more than 64 rows (columns) of non-zero weight under the one bin: roi_align_bwd_kernel leaves its shuffle branch"""
    for ax in ("y", "x"):
        for name in ("taps-128-%s" % ax, "taps-280px-%s" % ax):
            c = CASES[name]
            assert c["P"] == 1 and c["hw"][0] == ((70, 3) if ax == "y" else (3, 70))
            y, x = _rows_cols(c, 0)
            assert len(y if ax == "y" else x) > 64, name
        r = CASES["taps-280px-%s" % ax]["rois"][0]
        assert (r[3] - r[1] if ax == "y" else r[2] - r[0]) == 280


# ---- sparse RPN backward --------------------------------------------------------------------------------------------------------------
SPARSE = S.sparse_cases()
SPARSE_CATCHES = {
    "border_tap_wraps": ("borders-and-1x1-levels", "no-scale", "recompute", "a5-batch-256"),
    "duplicate_pixel_twice": ("one-pixel-all-anchors", "a9-batch-512"),
    "relu_mask_ignored": ("one-pixel-all-anchors", "adjacent-pixels", "batch-1", "recompute-shift"),
    "last_row_dropped": ("batch-1", "batch-1-three-images", "same-pixel-levels-images", "a9-k45-one-image", "recompute"),
}
_SPARSE_REF = {}


def sparse_ref(name):
    if name not in _SPARSE_REF:
        _SPARSE_REF[name] = S.sparse_ref_of(SPARSE[name])          # (asserts the NARROW premises of a narrow case)
    return _SPARSE_REF[name]


def _close(a, b, narrow, what):
    a, b = np.asarray(a), np.asarray(b)
    if narrow:
        assert np.array_equal(a, b), (what, float(np.abs(a - b).max()))
    else:
        assert np.allclose(a, b, rtol=1e-11, atol=1e-13 * max(1.0, float(np.abs(b).max()))), (what, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name", list(SPARSE))
def test_rpn_sparse_ref_equals_float64_autograd(name):
    """torch float64 autograd of conv3x3 (pad 1) * scale + shift -> ReLU -> 1x1 with d loss / d pred = d_pred.  With recompute_t the whole chain;
    with a stored t (which need not be the conv's output) the two halves on their own: the 1x1 on t, the conv under the reference's d_t.
    NARROW operands are exact in float64 in any order: equality; WIDE ones to float64 rounding."""
    import torch.nn.functional as Fn
    c, o = SPARSE[name], sparse_ref(name)
    narrow = c["cls"] == "narrow"
    T64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    K, B = c["K"], c["B"]
    wp = T64(c["w_pred"]).requires_grad_(True)
    wc = T64(c["w_conv"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)            # [n, c, ky, kx]
    sc = T64(np.ones(256) if c["scale"] is None else c["scale"])
    bc = T64(np.zeros(256) if c["shift"] is None else c["shift"]).requires_grad_(True)
    bp = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    feats, ts, loss = [], [], 0
    for l, (h, w) in enumerate(c["levels"]):
        x = T64(c["feat"][l]).reshape(B, h, w, 256).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        feats.append(x)
        hid = Fn.conv2d(x, wc, padding=1) * sc[None, :, None, None] + bc[None, :, None, None]
        dp = T64(c["dpred"][l])[..., :K]
        if c["recompute"]:
            t = torch.relu(hid).permute(0, 2, 3, 1).reshape(B, h * w, 256)
            loss = loss + ((t @ wp.T + bp) * dp).sum()
        else:
            t = T64(c["t"][l]).requires_grad_(True)
            ts.append(t)
            # the 1x1 alone: d / d t of relu(t) . W is the masked d_t; W's and the bias' gradients are linear in t as stored
            loss = loss + ((torch.relu(t) @ wp.detach().T) * dp).sum() + ((t.detach() @ wp.T + bp) * dp).sum() + (hid.permute(0, 2, 3, 1).reshape(B, h * w, 256) * T64(o["dt"][l])).sum()
    loss.backward()
    _close(o["gw_pred"], wp.grad.numpy(), narrow, "dW_pred")
    _close(o["gb_pred"], bp.grad.numpy(), narrow, "db_pred")
    _close(o["gb_conv"], bc.grad.numpy(), narrow, "db_conv")
    # dW_conv as the kernel applies the FrozenBN scale: autograd's gradient of the unscaled weight IS scale[n] * wgrad
    _close(o["gw_conv"], wc.grad.permute(0, 2, 3, 1).numpy(), narrow, "dW_conv")
    for l, (h, w) in enumerate(c["levels"]):
        _close(o["dfeat"][l] - c["dfeat"][l].astype(np.float64), feats[l].grad.permute(0, 2, 3, 1).reshape(B, h * w, 256).numpy(), narrow, f"d_feat {l}")
        if not c["recompute"]:
            _close(o["dt"][l], ts[l].grad.numpy(), narrow, f"d_t {l}")


@pytest.mark.parametrize("name", [n for n, c in SPARSE.items() if c["cls"] == "narrow"])
def test_sparse_fp32_restatements_equal_float64_on_narrow_data(name):
    c, o = SPARSE[name], sparse_ref(name)
    t32 = [t.astype(F32) for t in o["t"]]
    dr, ar = S.rpn_gather_rows_ref(c["levels"], c["rows"], c["batch"], c["dpred"], t32, c["K"])
    dt = S.rpn_dt_rows_ref(dr, ar, c["w_pred"], c["K"])
    for r, key in enumerate(c["rows"]):
        want = np.zeros(256) if key == S.NOROW else o["dt"][int(key >> 26)][r // c["batch"], int(key & 0x3ffffff)]
        assert np.array_equal(dt[r].astype(np.float64), want), (name, r)
    gw, gb, gc = S.rpn_head_sums_ref(dr, ar, dt, c["K"])
    for got, want in ((gw, o["gw_pred"]), (gb, o["gb_pred"]), (gc, o["gb_conv"])):
        assert np.array_equal(bits(got), bits(want.astype(F32))) and np.array_equal(got.astype(np.float64), want), name


@pytest.mark.parametrize("defect", S.SPARSE_DEFECTS)
def test_every_sparse_defect_is_caught(defect):
    for name in SPARSE_CATCHES[defect]:
        c, good = SPARSE[name], sparse_ref(name)
        bad = S.sparse_ref_of(c, defect=defect)
        diff = {k: int((np.asarray(good[k]) != np.asarray(bad[k])).sum()) for k in ("gw_pred", "gb_pred", "gw_conv", "gb_conv")}
        diff["dfeat"] = sum(int((g != b).sum()) for g, b in zip(good["dfeat"], bad["dfeat"]))
        print(f"{defect} on {name}: {diff}")
        assert sum(diff.values()) > 0, (defect, name)
    if defect == "border_tap_wraps":        # an interior pixel has no tap off the map: the family of border pixels is needed
        c = SPARSE["one-pixel-all-anchors"]
        bad = S.sparse_ref_of(c, defect=defect)
        assert all(np.array_equal(g, b) for g, b in zip(sparse_ref("one-pixel-all-anchors")["dfeat"], bad["dfeat"]))
    if defect == "duplicate_pixel_twice":
        c = SPARSE["adjacent-pixels"]
        assert np.array_equal(S.sparse_ref_of(c, defect=defect)["gw_pred"], sparse_ref("adjacent-pixels")["gw_pred"])


def test_sparse_case_premises():
    L = S.SPARSE_LEVELS
    key = lambda l, p: (l << 26) | p
    rows_of = lambda c, b: set(c["rows"].reshape(c["B"], c["batch"])[b][:c["nrows"][b]].tolist())
    assert {c["ld"] for c in SPARSE.values()} == {16, 32, 48} and {c["batch"] for c in SPARSE.values()} == {1, 8, 256, 512}
    assert {c["B"] for c in SPARSE.values()} == {1, 3} and any(c["K"] < c["ld"] for c in SPARSE.values())
    for c in SPARSE.values():        # R < 64: the head sums' partials are the larger use of G
        assert (c["B"] * c["batch"] < 64) == (c["B"] * c["batch"] * 2304 < (c["ld"] + 2) * 32 * 256)
    assert sum(c["B"] * c["batch"] < 64 for c in SPARSE.values()) >= 5
    c = SPARSE["one-pixel-all-anchors"]
    assert c["counts"].sum() == 3 and rows_of(c, 0) == {key(0, 17)}
    c = SPARSE["borders-and-1x1-levels"]
    want = {key(l, p) for l in range(5) for p in S._border_pixels(*L[l])}
    assert rows_of(c, 0) == want and {key(0, 0), key(0, 6), key(0, 35), key(0, 41), key(3, 0), key(4, 0)} <= want
    assert rows_of(SPARSE["adjacent-pixels"], 0) == {key(0, 16), key(0, 17)} and 16 // 7 == 17 // 7
    c = SPARSE["same-pixel-levels-images"]
    assert rows_of(c, 0) == rows_of(c, 2) == {key(0, 2), key(1, 2), key(2, 2)} and c["counts"][1].sum() == 0 and c["nrows"][1] == 0
    c = SPARSE["invalid-entries-and-overfull"]
    pre = c["sampled"][0][:8]
    total = S.anchor_offsets(L, 3)[-1]
    assert c["counts"][0].sum() > c["batch"] and (pre == -1).any() and (pre >= total).any() and c["nrows"][0] == 4
    for name, c in SPARSE.items():
        if c["recompute"]:
            o = sparse_ref(name)
            act = np.stack([o["t"][int(k >> 26)][r // c["batch"], int(k & 0x3ffffff)] for r, k in enumerate(c["rows"]) if k != S.NOROW])
            assert (act == 0).any() and (act > 0).any(), name
        elif c["nrows"].sum() >= 1:
            act = np.stack([c["t"][int(k >> 26)][r // c["batch"], int(k & 0x3ffffff)] for r, k in enumerate(c["rows"]) if k != S.NOROW])
            assert (act == 0).any() and (act < 0).any() and (act > 0).any(), name
        # junk behind the counted prefix names pixels that are no rows; d_pred is zero off the rows
        for b in range(c["B"]):
            rows = rows_of(c, b)
            for l, (h, w) in enumerate(L):
                nz = np.flatnonzero(np.abs(c["dpred"][l][b, :, :c["K"]]).sum(1))
                assert {key(l, int(p)) for p in nz} <= rows, name


def test_the_gpu_files_run_every_case():
    import test_roi_bwd_exact_gpu as GR
    import test_rpn_sparse_exact_gpu as GS
    assert list(GR.CASE_NAMES) == list(CASES) and list(GS.CASE_NAMES) == list(SPARSE)
    assert set(GR.ATOMIC_ONLY) == {n for n, c in CASES.items() if c["C"] != 256 or c["P"] > 16}
