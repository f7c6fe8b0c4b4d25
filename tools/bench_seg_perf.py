"""Times the segmentation class map of ONE 1024 x 1536 micrograph with the full set of matched pairs: the 351 polygon ground truths of
tests/golden/via_subset.json against the 257 committed particle predictions (tests/golden/rle_pickles.json.gz), every pair the matcher makes.
Evaluations alternate inside one process, after a warm-up of each:

  seg-cuda / seg-cpu    ampis_amd.analyze.seg_class_map(device='cuda' / 'cpu') from RLE dicts with the matches given: string decoding, ONE
                        amp_seg_class_map call, string encoding of the class masks -- what a user waits for
  call-device           the bare amp_seg_class_map call on arrays pooled once, with a context (csrc/seg_class_map.hip: upload, one memset, five
                        launches, download, stream synchronise -- all in the window)
  call-host             the same call with a NULL context (csrc/mask_analysis_host.hip)
  dense                 the dense method as tests/seg_class_ref.py restates it (decode the two masks of every pair, OR into three planes, code,
                        encode the classes) -- already kinder than the reference, which holds every mask of both sides decoded at once

All ways are checked to give the same bytes before anything is timed.  A call-* sample is the mean over --inner back-to-back calls.  Prints one
JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_seg_perf.py [--reps 7] [--warmup 2] [--inner 10] [--dense-reps 2] [--mode reduced] [--md profiles/r12/seg_perf.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from ampis_amd import _lib, analyze, rle

IMAGE = "Sc1Tile_001-002-000_0-000.png"


class Call:
    """amp_seg_class_map on arrays pooled once: what is timed is the C call alone."""

    def __init__(self, gt, pred, pairs, mode, size):
        self.gp, self.pp = rle._pool([rle._counts(x) for x in gt]), rle._pool([rle._counts(x) for x in pred])
        self.ng, self.np_ = len(gt), len(pred)
        self.pg, self.pq = np.ascontiguousarray(pairs[:, 0], np.int32), np.ascontiguousarray(pairs[:, 1], np.int32)
        self.mode, self.K, (self.h, self.w) = mode, (7 if mode else 4), size
        named_g, named_p = set(self.pg.tolist()), set(self.pq.tolist())
        self.cap = self.K * (1 + sum(int(self.gp[2][i]) - 1 for i in named_g) + sum(int(self.pp[2][i]) - 1 for i in named_p))
        self.counts, self.coff, self.px = np.zeros(self.cap, np.uint32), np.zeros(self.K + 1, np.uint64), np.zeros(8, np.uint64)
        self.runs = int(len(self.gp[0]) + len(self.pp[0]))

    def __call__(self, ctx):
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.lib().amp_seg_class_map(ctx.handle if ctx is not None else None, *(vp(x) for x in self.gp), self.ng, *(vp(x) for x in self.pp),
                                                self.np_, vp(self.pg), vp(self.pq), len(self.pg), self.h, self.w, self.mode, vp(self.counts), self.cap,
                                                vp(self.coff), vp(self.px)), "amp_seg_class_map")
        return self.counts[: int(self.coff[self.K])].copy(), self.coff.copy(), self.px.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--dense-reps", type=int, default=2)
    ap.add_argument("--mode", default="reduced", choices=("reduced", "all"))
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_seg_perf.py measures on a HIP device and none is visible: not measured")
    import seg_class_ref as ref
    import seg_perf_data as data
    gt, (pred, _) = data.gt_rles(IMAGE), data.pred_rles(IMAGE)
    match = analyze.rle_instance_matcher(gt, pred)
    pairs = np.asarray(match["tp"]).reshape(-1, 2)
    ctx = _lib.Context(0)
    call = Call(gt, pred, pairs, int(a.mode == "all"), data.SIZE)
    dev, host = call(ctx), call(None)
    assert all(d.tobytes() == h.tobytes() for d, h in zip(dev, host)), "device and host paths disagree"
    want, want_px, _ = ref.dense(gt, pred, pairs, a.mode, data.SIZE)                     # the dense method's warm-up
    assert np.concatenate(want).astype(np.uint32).tobytes() == dev[0].tobytes() and want_px.tolist() == dev[2].tolist(), "the dense method disagrees"
    seg = lambda d: analyze.seg_class_map(gt, pred, match, a.mode, device=d)
    assert [m["counts"] for m in seg("cuda")["masks"]] == [m["counts"] for m in seg("cpu")["masks"]]
    runs = {"seg-cuda": (lambda: seg("cuda"), 1), "seg-cpu": (lambda: seg("cpu"), 1), "call-device": (lambda: call(ctx), a.inner),
            "call-host": (lambda: call(None), a.inner)}
    ms = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):
        for name, (fn, inner) in runs.items():
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.sync()
            if i >= a.warmup:
                ms[name].append((time.perf_counter() - t) * 1e3 / inner)
    ms["dense"] = []
    for _ in range(a.dense_reps):
        t = time.perf_counter()
        ref.dense(gt, pred, pairs, a.mode, data.SIZE)
        ms["dense"].append((time.perf_counter() - t) * 1e3)
    ctx.close()
    out = {"metric": "segmentation class map of one 1024 x 1536 micrograph, ms per evaluation (host clock around synchronised calls)", "mode": a.mode,
           "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "dense_reps": a.dense_reps, "image": IMAGE, "ground_truths": len(gt),
           "predictions": len(pred), "pairs": int(len(pairs)), "runs": call.runs, "counts_out": int(dev[1][call.K]), "pixel_counts": dev[2].tolist(),
           "reference_dense_bytes": int(len(gt) + len(pred) + 5 * len(pairs)) * data.SIZE[0] * data.SIZE[1]}
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        names = {"seg-cuda": "analyze.seg_class_map(device='cuda'), from RLE dicts", "seg-cpu": "analyze.seg_class_map(device='cpu'), from RLE dicts",
                 "call-device": "amp_seg_class_map, context (upload + memset + 5 launches + download)", "call-host": "amp_seg_class_map, NULL context",
                 "dense": "the dense method (tests/seg_class_ref.py: decode per pair, three planes, code, encode)"}
        with open(a.md, "w") as f:
            f.write("# Segmentation class map of one micrograph (tools/bench_seg_perf.py)\n\n")
            f.write(f"{IMAGE}, 1024 x 1536: {len(gt)} polygon ground truths (tests/golden/via_subset.json) against {len(pred)} predictions "
                    f"(tests/golden/rle_pickles.json.gz), the {len(pairs)} matched pairs of rle_instance_matcher, mode '{a.mode}'; {call.runs} runs in, "
                    f"{out['counts_out']} counts out.  {a.reps} timed samples after {a.warmup} warm-ups, the evaluations alternating in one process; a "
                    f"bare-call sample is the mean of {a.inner} back-to-back calls, each ending in a stream synchronise; the dense method is sampled "
                    f"{a.dense_reps} times after its checking pass.  Host clock, MI355X.\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            for k in ("seg-cuda", "seg-cpu", "call-device", "call-host", "dense"):
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")
            f.write(f"\nAll ways give the same bytes (checked before timing).  Speed is recorded, not gated.  The gain claimed is the method: the run "
                    f"lists in, three bit planes of the image ({3 * data.SIZE[0] * data.SIZE[1] // 8} bytes) and the run lists out, where the reference "
                    f"holds [G + P + 5 pairs, H, W] bools = {out['reference_dense_bytes'] / 2 ** 30:.1f} GiB for this image (both sides decoded, the "
                    f"matched copies, TP / FN / FP).\n")


if __name__ == "__main__":
    main()
