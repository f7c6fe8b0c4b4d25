"""Times mask_edge_distance on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations, its
polygons as ground truth, the same masks shifted (even instances) or dilated (odd instances) by 2 px as predictions, every instance matched to its
own twin, tight boxes, ALL pairs in one call.  Three evaluations alternate inside one process, after a warm-up of each:

  device   amp_mask_edge_distance with a context (csrc/edge_distance.hip): upload, five launches, download, stream synchronise -- all inside the window
  host     the same call with a NULL context (csrc/mask_analysis_host.hip)
  dense    the reference's formulation (ampis/analyze.py:379-413: a [queries x targets x 2] float64 broadcast per pair, torch.sqrt, min) with torch
           on the same card, pair after pair, from crops decoded beforehand; pairs whose broadcast would pass --dense-gib are left out and counted

The first two are checked against each other (identical) and the third against them (rint(v^2) equal) before anything is timed.  Prints one JSON
line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_edge_distance.py [--reps 7] [--warmup 2] [--dense-gib 8] [--md profiles/r08/edge_distance.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ampis_amd import _lib, rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shift(m, dy, dx):
    out = np.zeros_like(m)
    h, w = m.shape
    out[max(dy, 0): h + min(dy, 0), max(dx, 0): w + min(dx, 0)] = m[max(-dy, 0): h + min(-dy, 0), max(-dx, 0): w + min(-dx, 0)]
    return out


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    gt, pred, boxes = [], [], []
    for i, reg in enumerate(img["regions"]):
        sa = reg["shape_attributes"]
        xy = np.stack([sa["all_points_x"], sa["all_points_y"]], axis=1).astype(np.float64).reshape(-1)
        if len(xy) < 6:
            continue
        g = rle.frPyObjects(xy.tolist(), h, w)
        m = rle.decode(g).astype(bool)
        if not m.any():
            continue
        if i % 2 == 0:
            p = shift(m, 2, -2)
        else:
            p = m.copy()
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dy * dy + dx * dx <= 4:
                        p |= shift(m, dy, dx)
        if not (p & m).any():
            continue
        u = m | p
        rows, cols = np.flatnonzero(u.any(axis=1)), np.flatnonzero(u.any(axis=0))
        gt.append(g)
        pred.append(rle.encode(np.asfortranarray(p.astype(np.uint8))))
        boxes.append([rows[0], rows[-1] + 1, cols[0], cols[-1] + 1])
    return h, w, gt, pred, np.asarray(boxes, dtype=np.int32)


class Call:
    """amp_mask_edge_distance on arrays pooled once: what is timed is the C call alone."""

    def __init__(self, gt, pred, boxes, h, w):
        self.n, self.h, self.w = len(gt), h, w
        gc, pc = [rle._counts(x) for x in gt], [rle._counts(x) for x in pred]
        self.g, self.p = rle._pool(gc), rle._pool(pc)
        self.idx = np.arange(self.n, dtype=np.int32)
        self.boxes = np.ascontiguousarray(boxes, dtype=np.int32)
        self.fp_cap, self.fn_cap = int(sum(int(c[1::2].sum()) for c in pc)), int(sum(int(c[1::2].sum()) for c in gc))
        self.fp, self.fn = np.empty(self.fp_cap, np.uint32), np.empty(self.fn_cap, np.uint32)
        self.fpo, self.fno = np.zeros(self.n + 1, np.uint64), np.zeros(self.n + 1, np.uint64)

    def __call__(self, ctx):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.lib().amp_mask_edge_distance(ctx.handle if ctx is not None else None, *(vp(a) for a in self.g), self.n, *(vp(a) for a in self.p), self.n,
                                                     vp(self.idx), vp(self.idx), vp(self.boxes), self.n, self.h, self.w, vp(self.fp), self.fp_cap, vp(self.fpo),
                                                     vp(self.fn), self.fn_cap, vp(self.fno)), "amp_mask_edge_distance")
        if ctx is not None:
            ctx.sync()
        return (self.fp[: int(self.fpo[-1])].copy(), self.fpo.copy(), self.fn[: int(self.fno[-1])].copy(), self.fno.copy())


def dense_pairs(torch, crops, budget_bytes):
    """The reference's evaluation on the card.  crops: per pair (gt, pred) bool arrays.  Returns (fp list, fn list, pairs left out)."""
    def min_euclid(a, b):
        return torch.sqrt(torch.pow(a.unsqueeze(1).double() - b.double(), 2).sum(axis=2)).min(axis=1)[0]
    fps, fns, skipped = [], [], 0
    for g, p in crops:
        if 3 * 16 * max(int((p & ~g).sum()) * int(g.sum()), int((g & ~p).sum()) * int(p.sum())) > budget_bytes:     # the broadcast, its square and the sum's input
            skipped += 1
            fps.append(None); fns.append(None)
            continue
        gm, pm = torch.from_numpy(g).cuda(), torch.from_numpy(p).cuda()
        gw, pw = torch.stack(torch.where(gm), 1), torch.stack(torch.where(pm), 1)
        fpw, fnw = torch.stack(torch.where(pm & ~gm), 1), torch.stack(torch.where(gm & ~pm), 1)
        fps.append(min_euclid(fpw, gw).cpu() if fpw.numel() else torch.zeros(0, dtype=torch.double))
        fns.append(min_euclid(fnw, pw).cpu() if fnw.numel() else torch.zeros(0, dtype=torch.double))
    torch.cuda.synchronize()
    return fps, fns, skipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-gib", type=float, default=8.0)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_edge_distance.py measures on a HIP device and none is visible: not measured")
    h, w, gt, pred, boxes = workload()
    call = Call(gt, pred, boxes, h, w)
    ctx = _lib.Context(0)
    crops = [(rle.decode(g)[b[0]:b[1], b[2]:b[3]].astype(bool), rle.decode(p)[b[0]:b[1], b[2]:b[3]].astype(bool)) for g, p, b in zip(gt, pred, boxes)]
    budget = int(a.dense_gib * (1 << 30))
    dev, host = call(ctx), call(None)
    assert all(np.array_equal(x, y) for x, y in zip(dev, host)), "device and host paths disagree"
    fps, fns, skipped = dense_pairs(torch, crops, budget)
    for k in range(call.n):
        for lst, (val, off) in ((fps, dev[0:2]), (fns, dev[2:4])):
            if lst[k] is not None:
                v = lst[k].numpy()
                assert np.array_equal(np.rint(v * v).astype(np.uint32), val[int(off[k]): int(off[k + 1])]), f"dense evaluation disagrees on pair {k}"
    ms = {"device": [], "host": [], "dense": []}
    for i in range(a.warmup + a.reps):
        for name, fn in (("device", lambda: call(ctx)), ("host", lambda: call(None)), ("dense", lambda: dense_pairs(torch, crops, budget))):
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t) * 1e3
            if i >= a.warmup:
                ms[name].append(dt)
    out = {"metric": "mask_edge_distance, all matched pairs of one 1024 x 1536 image in one call, ms per call (host clock around a synchronised call)",
           "image": [h, w], "pairs": call.n, "fp_pixels": int(dev[1][-1]), "fn_pixels": int(dev[3][-1]), "query_pixels": int(dev[1][-1] + dev[3][-1]),
           "crop_pixels": int(((boxes[:, 1] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 2])).sum()), "max_d2": int(max(dev[0].max(initial=0), dev[2].max(initial=0))),
           "reps": a.reps, "warmup": a.warmup, "dense_pairs_left_out": skipped, "dense_budget_gib": a.dense_gib}
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3)}
    ctx.close()
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# mask_edge_distance on one user-size image (tools/bench_edge_distance.py)\n\n")
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons as ground truth; predictions = the masks shifted or dilated by 2 px), "
                    f"{call.n} matched pairs in ONE call, {out['query_pixels']} query pixels ({out['fp_pixels']} false positive, {out['fn_pixels']} false negative), "
                    f"{out['crop_pixels']} crop pixels, largest squared distance {out['max_d2']}.  {a.reps} timed repetitions after {a.warmup} warm-ups, the three "
                    f"evaluations alternating in one process; host clock around a call that ends in a device synchronise.\n\n")
            f.write("| evaluation | median ms | min ms | max ms |\n|---|---|---|---|\n")
            names = {"device": "device path (amp_mask_edge_distance, context; upload + 5 launches + download)", "host": "host path (amp_mask_edge_distance, NULL context)",
                     "dense": f"dense pairwise distances with torch on the same card, pair by pair ({skipped} pairs left out for memory, budget {a.dense_gib} GiB)"}
            for k in ("device", "host", "dense"):
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} |\n")
            f.write("\nThe three agree on every value (device == host exactly; the dense evaluation through rint(v^2)).  Speed is recorded, not gated.\n")


if __name__ == "__main__":
    main()
