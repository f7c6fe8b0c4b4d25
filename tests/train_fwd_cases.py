"""Case tables of the training-forward tests: the smallest inputs at which anchor labelling, the two samplers, the loss kernels and the polygon
mask targets can go wrong.  Generated from fixed seeds; every case carries the coverage conditions tests/test_train_fwd_ref.py asserts on the
CPU against the reference alone, so a case that lost its edge fails there and not silently on the GPU."""
import numpy as np

import train_fwd_ref as R

F32 = np.float32
STRIDES = (4, 8, 16, 32, 64)
LV180 = tuple(zip((6, 3, 2, 1, 1), (7, 4, 2, 1, 1), STRIDES))                    # 180 anchors at A = 3; waves 0-63, 64-127, 128-179
LV2K = tuple(zip((26, 3, 2, 1, 1), (25, 4, 2, 1, 1), STRIDES))                   # 2 004
LV50K = tuple(zip((128, 1, 1, 1, 1), (130, 1, 1, 1, 1), STRIDES))                # 49 932: two chunks
LV196K = tuple(zip((256, 1, 1, 1, 1), (256, 1, 1, 1, 1), STRIDES))               # 196 620: five chunks
SIZES_A9 = ((24, 32, 48), (48, 64, 96), (96, 128, 192), (192, 256, 384), (384, 512, 768))
RATIOS = (0.5, 1.0, 2.0)


_CACHE = {}


def cases(kind):
    """the table `kind` (the name of one of the *_cases functions below), built once and left unchanged"""
    if kind not in _CACHE:
        _CACHE[kind] = globals()[kind]()
    return _CACHE[kind]


def total(levels, A=3):
    return int(R.level_offsets(levels, A)[-1])


def _rand_gt(rng, n, lo=-30, hi=70):
    c = rng.integers(lo * 4, hi * 4, size=(n, 2)) / 4.0
    s = rng.integers(16, 240, size=(n, 2)) / 4.0
    return np.concatenate([c - s / 2, c + s / 2], axis=1).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- anchor labels
DUP_PAIRS = ((0, 1), (63, 64), (255, 256), (3, 260))


def label_cases():
    rng = np.random.default_rng(2201)
    cells3, cells9, cells1 = R.default_cells(), R.default_cells(SIZES_A9), R.default_cells(ratios=(1.0,))
    anc3 = R.anchors_ref(LV180, cells3)
    c = {}
    # IoU exactly 0.5 = hi and 0.25 = lo in fp32.  P = [0,0,32,32] is the 32-px square anchor at pixel (4,4) of p2; the left half of it has a
    # better anchor among the 24-px ones, so P gets its label from the equality alone; likewise the quarter box of P2 = [8,4,40,36]
    c["thresholds-a9"] = dict(levels=LV180, cells=cells9, sizes=SIZES_A9, ratios=RATIOS, lo=0.25, hi=0.5,
                              gt=[np.asarray([[0, 0, 16, 32], [8, 4, 24, 20]], F32)])
    c["a1-g1-b1"] = dict(levels=LV180, cells=cells1, sizes=(32, 64, 128, 256, 512), ratios=(1.0,), lo=0.3, hi=0.7, gt=[np.asarray([[2, 3, 30, 33]], F32)])
    g = _rand_gt(rng, 300)
    for k, (i, j) in enumerate(DUP_PAIRS):          # a duplicated box is the box of an anchor: IoU 1 there, the first of the pair must win
        g[i] = g[j] = anc3[(7 + 31 * k) % len(anc3)]
    c["dups-g300"] = dict(levels=LV180, cells=cells3, lo=0.3, hi=0.7, gt=[g])
    c["counts"] = dict(levels=LV180, cells=cells3, lo=0.3, hi=0.7, gt=[_rand_gt(rng, n) for n in (1, 64, 65, 256, 257, 300)])
    ordinary = np.asarray([4, 2, 30, 26], F32)
    c["waves"] = dict(levels=LV180, cells=cells3, lo=0.3, hi=0.7, gt=[
        np.asarray([[-250, -250, -240, -240], [-22, -22, -17, -17], ordinary], F32),          # last wave only; inside wave 0's box, none of its anchors
        np.zeros((0, 4), F32),                                                                 # an image without GT between two that have some
        np.asarray([[5000, 5000, 5010, 5010], ordinary], F32),                                 # no wave's bounding box
        np.asarray([[10, 10, 10, 20], ordinary], F32)])                                        # zero area
    for v in c.values():
        v.setdefault("sizes", (32, 64, 128, 256, 512))
        v.setdefault("ratios", RATIOS)
    return c


# ---------------------------------------------------------------------------------------------------------------- RPN sampler
def _labels(rng, N, B, npos, nneg, pos_in=None, neg_in=None, same=False):
    lab = np.full((B, N), -1, np.int8)
    for b in range(B):
        if same and b:
            lab[b] = lab[0]
            continue
        pool = np.arange(N)
        pi = rng.choice(pool if pos_in is None else pool[pos_in[0]:pos_in[1]], npos, replace=False)
        lab[b, pi] = 1
        free = np.flatnonzero(lab[b] != 1)
        if neg_in is not None:
            free = free[(free >= neg_in[0]) & (free < neg_in[1])]
        lab[b, rng.choice(free, nneg, replace=False)] = 0
    return lab


QUOTAS = ("more-pos", "fewer-pos", "scarce", "no-pos", "no-neg", "pos-max-0", "batch-1", "batch-512")
SHAPES = {"180": LV180, "2k": LV2K, "50k": LV50K, "196k": LV196K}


def rpn_sample_cases():
    rng = np.random.default_rng(2202)
    c = {}
    for sname, lv in SHAPES.items():
        N = total(lv)
        many_pos, many_neg = min(3 * N // 4, 600), min(N // 5, 4000)
        for q in QUOTAS:
            batch, pos_max = {"batch-1": (1, 1), "batch-512": (512, 256), "pos-max-0": (256, 0)}.get(q, (256, 128))
            npos, nneg = {"fewer-pos": (min(N // 9, 40), min(7 * N // 10, 5000)), "scarce": (10, 30), "no-pos": (0, min(7 * N // 10, 5000)),
                          "no-neg": (many_pos, 0)}.get(q, (many_pos, many_neg))
            c[f"{sname}/{q}"] = dict(levels=lv, B=2, batch=batch, pos_max=pos_max, seed=1000 + len(c), label=_labels(rng, N, 2, npos, nneg), quota=q)
    N = total(LV50K)
    c["50k/pos-in-second-chunk"] = dict(levels=LV50K, B=2, batch=256, pos_max=128, seed=7, label=_labels(rng, N, 2, 200, 3000, pos_in=(R.SAMPLE_CHUNK, N)))
    lab = _labels(rng, N, 2, 0, 3000)
    lab[:, R.SAMPLE_CHUNK - 12:R.SAMPLE_CHUNK + 12] = 1          # 24 positives on both sides of 49 151 / 49 152: all are taken
    c["50k/pos-across-chunks"] = dict(levels=LV50K, B=2, batch=256, pos_max=128, seed=8, label=lab)
    lab = _labels(rng, N, 2, 50, 3000, pos_in=(0, R.SAMPLE_CHUNK), neg_in=(0, R.SAMPLE_CHUNK))
    lab[:, R.SAMPLE_CHUNK + rng.choice(N - R.SAMPLE_CHUNK, 30, replace=False)] = 0          # a chunk with fewer candidates than batch
    c["50k/thin-second-chunk"] = dict(levels=LV50K, B=2, batch=256, pos_max=128, seed=9, label=lab)
    c["2k/same-labels-two-images"] = dict(levels=LV2K, B=2, batch=256, pos_max=128, seed=10, label=_labels(rng, total(LV2K), 2, 300, 1200, same=True))
    for sname in ("180", "2k", "50k"):          # the floor key: image 1, the positives' stream, one of few positives -> taken, and last
        lv = SHAPES[sname]
        lab = _labels(rng, total(lv), 2, 20, min(total(lv) // 2, 2000))
        idx = int(np.flatnonzero(lab[1] == 1)[7])
        c[f"{sname}/floor-key"] = dict(levels=lv, B=2, batch=256, pos_max=128, seed=R.floor_key_seed(1, 0, idx), label=lab, floor=(1, idx))
    return c


# ---------------------------------------------------------------------------------------------------------------- RoI sampler
def _roi_case(rng, B, Pcap, counts, G, K, batch, fg_max, thresh=0.5, num_anchors=200000, seed=5, **kw):
    gt = [_rand_gt(rng, g, 0, 400) for g in G]
    cls = [rng.integers(0, K, size=g).astype(np.int32) for g in G]
    prop = np.zeros((B, Pcap, 4), F32)
    for b in range(B):
        if G[b]:          # a third near a GT box (foreground), the rest anywhere
            src = gt[b][rng.integers(0, G[b], size=Pcap)]
            jit = rng.integers(-12, 13, size=(Pcap, 4)) / 4.0
            near = np.stack([src[:, 0] + jit[:, 0], src[:, 1] + jit[:, 1], np.maximum(src[:, 2] + jit[:, 2], src[:, 0] + 2), np.maximum(src[:, 3] + jit[:, 3], src[:, 1] + 2)], 1)
            prop[b] = np.where((np.arange(Pcap) % 3 == 0)[:, None], near, _rand_gt(rng, Pcap, 0, 400))
        else:
            prop[b] = _rand_gt(rng, Pcap, 0, 400)
    anchor = np.stack([rng.permutation(num_anchors)[:Pcap] for _ in range(B)]).astype(np.int32)
    d = dict(B=B, Pcap=Pcap, prop=prop, count=np.asarray(counts, np.int32), anchor=anchor, gt=gt, cls=cls, K=K, batch=batch, fg_max=fg_max,
             thresh=thresh, num_anchors=num_anchors, seed=seed)
    d.update(kw)
    return d


def roi_sample_cases():
    rng = np.random.default_rng(2203)
    c = {}
    c["empty-edges"] = _roi_case(rng, 4, 40, (0, 30, 0, 55), (5, 0, 0, 6), 3, 64, 16)          # P = 0 with G > 0; G = 0; both 0; prop_count > Pcap
    c["n-below-batch"] = _roi_case(rng, 2, 100, (60, 100), (7, 3), 80, 512, 128)
    c["n-1025"] = _roi_case(rng, 2, 1020, (1020, 1019), (5, 6), 80, 512, 128)                 # cap binds in image 0 ...
    c["n-8193-batch-2048"] = _roi_case(rng, 1, 8190, (8190,), (3,), 1, 2048, 2048)            # ... and does not here (K = 1)
    d = _roi_case(rng, 1, 8, (8,), (4,), 3, 16, 8)
    d["gt"] = [np.asarray([[0, 0, 32, 32], [100, 100, 140, 150], [100, 100, 140, 150], [60, 10, 60, 30]], F32)]          # duplicates; zero area
    d["cls"] = [np.asarray([2, 0, 1, 1], np.int32)]
    d["prop"][0, 0] = [0, 0, 16, 32]          # IoU exactly 0.5
    d["prop"][0, 1] = [100, 100, 140, 150]    # both duplicates at IoU 1: the first wins
    d["prop"][0, 2] = [0, 0, 16, 31.75]       # just below
    c["iou-edges"] = d
    d = _roi_case(rng, 2, 300, (300, 300), (6, 6), 3, 64, 16)
    d["anchor"][0, :] = 1234                                       # one identity: pure index order, the cap cuts inside the tie
    d["anchor"][1, :] = np.repeat(np.arange(150), 2) + 77         # pairs of equal identities
    c["repeated-identities"] = d
    d = _roi_case(rng, 1, 50, (50,), (4,), 3, 64, 40)
    d["floor"] = True
    c["floor-key"] = d
    for name, d in c.items():
        if d.get("floor"):          # the floor key on the first foreground proposal: taken last among the foreground
            r = R.roi_sample_ref(d["prop"], d["count"], d["anchor"], d["gt"], d["cls"], d["K"], d["batch"], d["fg_max"], d["thresh"], 0, d["num_anchors"])
            first = r[0][0, 0]
            i = int(np.flatnonzero((d["prop"][0] == first).all(1))[0])
            d["seed"] = R.floor_key_seed(0, 2, int(d["anchor"][0, i]))
            d["floor_ident"] = int(d["anchor"][0, i])
    return c


def roi_ref_of(d, defect=None):
    return R.roi_sample_ref(d["prop"], d["count"], d["anchor"], d["gt"], d["cls"], d["K"], d["batch"], d["fg_max"], d["thresh"], d["seed"],
                            d["num_anchors"], defect)


# ---------------------------------------------------------------------------------------------------------------- mask targets
_H = float.fromhex
# integer-pixel triangles on which 28 / max(side, 0.1) in double and in fp32 give different targets (found by search on the CPU)
RATIO_INSTANCES = (
    ([86.0, 46.0, 128.0, 49.0, 86.0, 64.0], ("0x1.54eff8p+6", "0x1.fp+4", "0x1.36851cp+7", "0x1.0cp+6")),
    ([85.0, 55.0, 142.0, 61.0, 85.0, 65.0], ("0x1.53d08p+6", "0x1.98p+5", "0x1.804f4cp+7", "0x1.08p+6")),
    ([6.0, 100.0, 37.0, 105.0, 6.0, 109.0], ("0x1.7521a4p+2", "0x1.8cp+6", "0x1.6a9222p+5", "0x1.bcp+6")),
    ([54.0, 33.0, 116.0, 39.0, 54.0, 52.0], ("0x1.a9b7b4p+5", "0x1.cp+4", "0x1.5666a8p+7", "0x1.a8p+5")),
    ([145.0, 43.0, 195.0, 55.0, 145.0, 60.0], ("0x1.21fd3cp+7", "0x1.38p+5", "0x1.c5bfe4p+7", "0x1.3cp+6")),
    ([110.0, 96.0, 125.0, 103.0, 110.0, 109.0], ("0x1.b69ac4p+6", "0x1.7cp+6", "0x1.0bdd18p+7", "0x1.e8p+6")),
)


def mask_cases():
    """-> list of (name, polygons of the instance, box fp32[4])"""
    rng = np.random.default_rng(2204)
    c = []
    for i, (p, b) in enumerate(RATIO_INSTANCES):
        c.append((f"ratio-{i}", [np.asarray(p)], np.asarray([_H(v) for v in b], F32)))
    for i in range(12):          # integer-pixel polygons, what annotation tools produce
        k = int(rng.integers(3, 12))
        cx, cy, r = rng.integers(30, 200), rng.integers(30, 200), rng.integers(4, 60)
        th = np.sort(rng.uniform(0, 2 * np.pi, k))
        p = np.stack([np.round(cx + r * np.cos(th)), np.round(cy + r * np.sin(th))], 1).reshape(-1)
        j = rng.uniform(-0.3, 0.3, 4) * r
        c.append((f"integer-{i}", [p], np.asarray([cx - r + j[0], cy - r + j[1], cx + r + j[2], cy + r + j[3]], F32)))
    # vertices on the rounding boundaries of the 5x grid: box [0,0,28,28] has ratio 1, so x = (m + 0.5) / 5 scales to m + 0.5 + 0.5 exactly;
    # one double below it truncates to m, at it to m + 1
    box = np.asarray([0, 0, 28, 28], F32)
    for i, m in enumerate((7, 52, 99)):
        at = (m + 0.5) / 5.0
        for side, x in (("below", np.nextafter(at, 0.0)), ("at", at), ("above", np.nextafter(at, 100.0))):
            c.append((f"boundary-{m}-{side}", [np.asarray([x, 2.0, 25.0, x, x, 26.0])], box))
    c.append(("outside", [np.asarray([100.0, 100, 120, 100, 110, 130])], np.asarray([10, 10, 50, 40], F32)))
    c.append(("covering", [np.asarray([-50.0, -50, 200, -50, 200, 200, -50, 200])], np.asarray([10, 10, 50, 40], F32)))          # all ones
    c.append(("left-and-above", [np.asarray([3.3, 2.2, 40.6, 8.1, 20.2, 45.7])], np.asarray([12.5, 11.25, 50, 40], F32)))      # negative scaled coordinates
    c.append(("thin-box", [np.asarray([10.0, 10, 10.06, 10, 10.06, 30, 10, 30])], np.asarray([10, 10, 10.05, 30], F32)))          # sides below 0.1 px
    c.append(("thin-both", [np.asarray([10.0, 10, 10.06, 10, 10.06, 10.05, 10, 10.05])], np.asarray([10, 10, 10.05, 10.03125], F32)))
    c.append(("three-polygons", [np.asarray([12.0, 12, 25, 12, 25, 22, 12, 22]), np.asarray([30.0, 25, 48, 25, 40, 38]),
                                 np.asarray([20.0, 18, 35, 18, 35, 30, 20, 30])], np.asarray([10, 10, 50, 40], F32)))
    return c


# ---------------------------------------------------------------------------------------------------------------- loss stages
def _solve(fn, target, guess):
    """an fp32 p near `guess` with fn(p) == target bit for bit (None when the neighbours hold none)"""
    p = F32(guess)
    cand = [p]
    lo = hi = p
    for _ in range(4):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        cand += [lo, hi]
    for q in cand:
        if F32(fn(F32(q))) == F32(target):
            return F32(q)
    return None


def shape_rows(mode, beta, p4, src, gt, w, equal_rows=(), edge_sign=None):
    """Rewrite the predicted deltas p4 [n, 4] of some rows so that the edges of `mode` occur; -> the facts the rows now hold (coverage).
    equal_rows: rows whose source box equals their GT box bit for bit: deltas 0 there, or, with edge_sign, (edge_sign * beta, 0, 0, 0): the
    target deltas are exact zeros (logf(1) = 0), so |d| == beta holds bit for bit and the row's loss has no rounding on its path."""
    n = len(p4)
    t = [q.f for q in R.deltas_ref(src, gt, w)]
    cover = dict(d_zero=0, beta_edge=0, beta_edge_exact=0, clamp_at=0, clamp_above=0)
    w = [F32(v) for v in w]
    for i in range(n):
        m = i % 7
        if i in equal_rows:
            p4[i] = 0
            if edge_sign is not None and mode == "smooth_l1":
                p4[i, 0] = F32(edge_sign) * F32(beta)
                cover["beta_edge_exact"] += 1
        elif mode == "l1" and m == 0:
            p4[i, 0] = t[0][i]
            cover["d_zero"] += 1
        elif mode == "smooth_l1" and m < 3:          # |d| == beta exactly on q = 0 / 1, both signs (p - t is exact only for a small t)
            sgn = F32(1 if (i // 7) % 2 else -1)
            for q in range(2):
                p = _solve(lambda v: v - t[q][i], sgn * F32(beta), t[q][i] + sgn * F32(beta))
                if p is not None:
                    p4[i, q] = p
                    cover["beta_edge"] += 1
        elif mode == "giou" and m == 0:
            p = _solve(lambda v: v / w[2], R.SCALE_CLAMP, R.SCALE_CLAMP * w[2])
            if p is not None:
                p4[i, 2] = p
                cover["clamp_at"] += 1
        elif mode == "giou" and m == 1:
            above = np.nextafter(R.SCALE_CLAMP, F32(np.inf))
            p = _solve(lambda v: v / w[3], above, above * w[3])
            if p is not None:
                p4[i, 3] = p
                cover["clamp_above"] += 1
        elif mode == "giou" and m == 2:
            p4[i, 0] += F32(5) * w[0]          # far away: disjoint
        elif mode == "giou" and m == 3:
            p4[i] = [t[q][i] for q in range(4)]          # the GT box, shrunk about its centre: nested
            p4[i, 2:] -= np.asarray(w[2:], F32)
    return cover


# (mode, amp_loss_opts type, beta).  beta 0.1: at |d| == beta the quadratic and the linear branch give different fp32 bits (0.5 d^2 / beta against
# |d| - 0.5 beta), so the strict < is visible in the loss term; the gradient is +-1 on both sides
REG_MODES = (("l1", "smooth_l1", 0.0), ("smooth_l1", "smooth_l1", 0.1), ("giou", "giou", 0.0))


def rpn_loss_cases():
    """-> dict name -> case: labels and samples come from the references; the predictions are shaped per sampled row"""
    c = {}
    for A, sizes in ((3, (32, 64, 128, 256, 512)), (9, SIZES_A9)):
        cells = R.default_cells(sizes)
        anc = R.anchors_ref(LV180, cells)
        ld = 16 * ((5 * A + 15) // 16)
        for mode, ltype, beta in REG_MODES:
            for batch, pos_max, edge in ((256, 128, False), (1, 1, False), (1, 0, False), (1, 1, True)):
                if (batch == 1 and A == 9) or (edge and mode != "smooth_l1"):
                    continue
                rng = np.random.default_rng(2205 + 10 * A + len(c))
                sq = anc[[i for i in range(len(anc)) if float(anc[i, 2] - anc[i, 0]) == float(anc[i, 3] - anc[i, 1])][:2]]          # two square anchors as GT
                if edge:          # the one positive of each image IS its GT box (hi = 0.95 leaves no other): p = (+-beta, 0, 0, 0) on it
                    gt = [sq[:1], sq[1:2]]
                    lab = R.anchor_labels_ref(LV180, cells, gt, 0.3, 0.95)
                else:
                    gt = [np.concatenate([sq, _rand_gt(rng, 5, 0, 30)]), _rand_gt(rng, 3, 0, 30)]
                    lab = R.anchor_labels_ref(LV180, cells, gt, 0.3, 0.7)
                seed = 31 + len(c)
                sampled, counts = R.rpn_sample_ref(lab["label"], seed, batch, pos_max)
                preds = [(rng.standard_normal((2, h * w, ld)) * 0.5).astype(F32) for h, w, _ in LV180]
                for p in preds:
                    p[..., 5 * A:] = 0
                off = R.level_offsets(LV180, A)
                cover = dict(d_zero=0, beta_edge=0, beta_edge_exact=0, clamp_at=0, clamp_above=0, equal=0, big_logit=0)
                for b in range(2):
                    npos = int(counts[b, 0])
                    an = sampled[b, :npos + int(counts[b, 1])].astype(np.int64)
                    lvl = np.searchsorted(off, an, side="right") - 1
                    pix, k = (an - off[lvl]) // A, (an - off[lvl]) % A
                    for i in range(len(an)):          # saturated logits on positives and negatives
                        if i % 5 == 2:
                            preds[lvl[i]][b, pix[i], k[i]] = 80.0 if i % 2 else -80.0
                            cover["big_logit"] += 1
                    if npos:
                        g = gt[b][lab["match_idx"][b][an[:npos]]]
                        p4 = np.stack([[preds[lvl[i]][b, pix[i], A + 4 * k[i] + q] for q in range(4)] for i in range(npos)]).astype(F32)
                        eq = [i for i in range(npos) if np.array_equal(anc[an[i]], g[i])]
                        cv = shape_rows(mode, beta, p4, anc[an[:npos]], g, (1.0, 1.0, 1.0, 1.0), eq, (1, -1)[b] if edge else None)
                        for key, v in cv.items():
                            cover[key] += v
                        cover["equal"] += len(eq)
                        for i in range(npos):
                            preds[lvl[i]][b, pix[i], A + 4 * k[i]:A + 4 * k[i] + 4] = p4[i]
                c[f"a{A}-{mode}-{'edge-' if edge else ''}b{batch}-p{pos_max}"] = dict(levels=LV180, A=A, sizes=sizes, cells=cells, ld=ld, gt=gt, lab=lab, seed=seed, batch=batch, pos_max=pos_max,
                                                             sampled=sampled, counts=counts, preds=preds, mode=mode, ltype=ltype, beta=beta, w_cls=0.5, w_loc=2.0, cover=cover)
    return c


def rpn_loss_ref_of(d, defect=None):
    inv = F32(1.0) / F32(d["batch"] * 2)
    cls_scale = inv * F32(d["w_cls"])
    loc_scale = inv * F32(d["w_cls"]) * F32(d["w_loc"])
    return R.rpn_loss_ref(d["levels"], d["cells"], d["preds"], d["gt"], d["lab"]["match_idx"], d["sampled"], d["counts"], d["mode"], d["beta"], cls_scale,
                          loc_scale, defect)


def box_loss_cases():
    c = {}
    W = (10.0, 10.0, 5.0, 5.0)
    for K, batch, shape in ((3, 64, "mixed"), (1, 64, "mixed"), (80, 64, "mixed"), (1, 2048, "strided"), (3, 1, "one"), (3, 1, "edge")):
        for mode, ltype, beta in REG_MODES:
            if shape == "edge" and mode != "smooth_l1":
                continue
            rng = np.random.default_rng(2206 + len(c))
            if shape == "mixed":          # image 0: fewer candidates than batch (unused rows); image 1: no GT (all background); image 2: full
                d = _roi_case(rng, 3, 90, (40, 90, 90), (5, 0, 6), K, batch, batch // 4, seed=17 + len(c))
            elif shape == "strided":
                d = _roi_case(rng, 1, 2100, (2100,), (8,), K, batch, 1024, seed=17 + len(c))
            elif shape == "edge":          # no proposals: the one row of each image is its appended GT box; p = (+-beta, 0, 0, 0) on it
                d = _roi_case(rng, 2, 30, (0, 0), (1, 1), K, 1, 1, seed=17 + len(c))
            else:
                d = _roi_case(rng, 2, 30, (30, 30), (2, 0), K, 1, 1, seed=17 + len(c))          # one foreground row; one background row
            rois, roi_cls, roi_gti, counts = roi_ref_of(d)
            B = d["B"]
            ld = 16 * ((5 * K + 1 + 15) // 16)
            pred = (rng.standard_normal((B * batch, ld)) * 0.6).astype(F32)
            cover = dict(d_zero=0, beta_edge=0, beta_edge_exact=0, clamp_at=0, clamp_above=0, equal=0, big_logit=0)
            for b in range(B):
                rows = b * batch + np.arange(batch)
                for r in np.flatnonzero(roi_cls[b] >= 0):
                    if r % 5 == 2:
                        pred[rows[r], int(rng.integers(0, K + 1))] = 80.0 if r % 2 else -80.0
                        cover["big_logit"] += 1
                fg = np.flatnonzero((roi_cls[b] >= 0) & (roi_cls[b] < K))
                if len(fg):
                    g = d["gt"][b][roi_gti[b, fg]]
                    col = K + 1 + 4 * roi_cls[b, fg]
                    p4 = np.stack([pred[rows[fg], col + q] for q in range(4)], 1)
                    eq = [i for i in range(len(fg)) if np.array_equal(rois[b, fg[i]], g[i])]
                    cv = shape_rows(mode, beta, p4, rois[b, fg], g, W, eq, (1, -1)[b] if shape == "edge" else None)
                    for key, v in cv.items():
                        cover[key] += v
                    cover["equal"] += len(eq)
                    for q in range(4):
                        pred[rows[fg], col + q] = p4[:, q]
            total_rois = int(counts.sum())
            c[f"k{K}-b{batch}-{mode}{'-edge' if shape == 'edge' else ''}"] = dict(roi=d, K=K, batch=batch, B=B, ld=ld, pred=pred, rois=rois, roi_cls=roi_cls, roi_gti=roi_gti, counts=counts, mode=mode,
                                             ltype=ltype, beta=beta, w=W, w_reg=3.0, total_rois=total_rois, cover=cover)
    return c


def box_loss_ref_of(d, defect=None):
    inv = F32(1.0) / F32(max(d["total_rois"], 1))
    return R.box_loss_ref(d["pred"], d["K"], d["rois"], d["roi_cls"], d["roi_gti"], d["roi"]["gt"], d["batch"], d["w"], d["mode"], d["beta"], inv,
                          inv * F32(d["w_reg"]), defect)


def focal_cases():
    """-> dict name -> (x [N, K], labels [N], K, alpha, gamma, scale).  In the 'single' layout only the first row of each 256 is live, so a
    workgroup's partial sum is ONE element's loss (K = 1)."""
    rng = np.random.default_rng(2207)
    c = {}
    edge = np.asarray([0, 30, -30, 100, -100, 1e-3, -1e-3, 5, -5, 17.5, -17.5, 88, -88], F32)
    for gamma in (0.0, 1.0, 2.0):
        for alpha in (0.25, -1.0):
            K = 5
            x = (rng.standard_normal((70, K)) * 3).astype(F32)
            x[:len(edge), 0], x[:len(edge), 1] = edge, edge[::-1]
            labels = rng.integers(-1, K + 1, size=70).astype(np.int32)          # -1 ignored, K background
            labels[:len(edge)] = np.where(np.arange(len(edge)) % 3 == 0, 0, np.where(np.arange(len(edge)) % 3 == 1, 1, K))
            labels[20], labels[21] = -1, K
            c[f"g{gamma:g}-a{alpha:g}"] = (x, labels, K, alpha, gamma, 1.0 / 37)
            n = 2 * len(edge) + 6
            xs = np.zeros((256 * n, 1), F32)
            ls = np.full(256 * n, -1, np.int32)
            xs[::256, 0] = np.concatenate([edge, edge, (rng.standard_normal(6) * 3).astype(F32)])
            ls[::256] = np.concatenate([np.zeros(len(edge)), np.ones(len(edge)), rng.integers(0, 2, 6)]).astype(np.int32)
            c[f"single-g{gamma:g}-a{alpha:g}"] = (xs, ls, 1, alpha, gamma, 1.0)
    return c


# ---------------------------------------------------------------------------------------------------------------- names
# The parametrised tests take their case names from here, so collecting them builds no case; tests/test_train_fwd_ref.py asserts that each
# list equals the keys of its table.
LABEL_NAMES = ("thresholds-a9", "a1-g1-b1", "dups-g300", "counts", "waves")
RPN_SAMPLE_NAMES = tuple(f"{s}/{q}" for s in SHAPES for q in QUOTAS) + (
    "50k/pos-in-second-chunk", "50k/pos-across-chunks", "50k/thin-second-chunk", "2k/same-labels-two-images", "180/floor-key", "2k/floor-key", "50k/floor-key")
ROI_SAMPLE_NAMES = ("empty-edges", "n-below-batch", "n-1025", "n-8193-batch-2048", "iou-edges", "repeated-identities", "floor-key")
RPN_LOSS_NAMES = tuple(f"a3-{m}-b{b}-p{p}" for m, _, _ in REG_MODES for b, p in ((256, 128), (1, 1), (1, 0))) + ("a3-smooth_l1-edge-b1-p1",) + \
    tuple(f"a9-{m}-b256-p128" for m, _, _ in REG_MODES)
BOX_LOSS_NAMES = tuple(f"k{k}-b{b}-{m}" for k, b in ((3, 64), (1, 64), (80, 64), (1, 2048), (3, 1)) for m, _, _ in REG_MODES) + ("k3-b1-smooth_l1-edge",)
FOCAL_NAMES = tuple(f"{pre}g{g}-a{a}" for g in (0, 1, 2) for a in ("0.25", "-1") for pre in ("", "single-"))
