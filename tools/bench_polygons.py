"""Times polygon ground truth -> run lists on the 351-instance micrograph of tests/golden/via_subset.json (1024 x 1536).  Evaluations alternate inside
one process, after a warm-up of each:

  composition    the per-polygon path the callers used before: rle.merge(rle.frPyObjects(polygons, h, w)) per instance -- a list conversion, a fresh
                 buffer, one amp_rle_from_polygon call, a counts-string encode and a merge that decodes it again, per polygon
  host           rle.polygons_to_rle(ctx=None): one amp_polygons_to_rle call with a NULL context (csrc/polygon_runs_host.hip) and one counts_to_strings
  device         rle.polygons_to_rle(ctx=...): the same with a context (csrc/polygon_runs.hip: upload, the launches, download, stream synchronise)
                 -- all in the window
  masks-cpu      analyze.masks_to_rle(PolygonMasks, size, device='cpu') end to end
  masks-cuda     analyze.masks_to_rle(PolygonMasks, size, device='cuda') end to end

The three paths are checked identical, every counts string, before anything is timed.  Prints one JSON line; --md PATH also writes the figures as a
markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_polygons.py [--reps 21] [--warmup 3] [--inner 3] [--md profiles/r17/polygons_to_rle.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from ampis_amd import _lib, analyze, rle
from ampis_amd.structures import PolygonMasks

NAMES = {"composition": "the per-polygon composition: rle.merge(rle.frPyObjects(...)) per instance",
         "host": "rle.polygons_to_rle(ctx=None): one call on the host, counts strings included",
         "device": "rle.polygons_to_rle(ctx): upload, launches, download, counts strings",
         "masks-cpu": "analyze.masks_to_rle(PolygonMasks, size, device='cpu') end to end",
         "masks-cuda": "analyze.masks_to_rle(PolygonMasks, size, device='cuda') end to end"}


def composition(polys, h, w):
    return [rle.merge(rle.frPyObjects([np.asarray(p).reshape(-1).tolist() for p in inst], h, w)) for inst in polys]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_polygons.py measures on a HIP device and none is visible: not measured")
    import seg_perf_data as D
    ctx = analyze._current_device_context("bench_polygons")
    fn = max(D.file_names(), key=lambda f: len(D.gt_polygons(f)[0]))
    polys, _, (h, w) = D.gt_polygons(fn)
    pm = PolygonMasks(polys)
    runs = {"composition": lambda: composition(polys, h, w), "host": lambda: rle.polygons_to_rle(polys, h, w, ctx=None),
            "device": lambda: rle.polygons_to_rle(polys, h, w, ctx=ctx), "masks-cpu": lambda: analyze.masks_to_rle(pm, (h, w), device="cpu"),
            "masks-cuda": lambda: analyze.masks_to_rle(pm, (h, w), device="cuda")}
    first = {k: [bytes(r["counts"]) for r in f()] for k, f in runs.items()}
    assert all(v == first["composition"] for v in first.values()), "the paths disagree"
    ms = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):
        for key, f in runs.items():
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.inner):
                f()
            dt = (time.perf_counter() - t) * 1e3 / a.inner
            if i >= a.warmup:
                ms[key].append(dt)
    out = {"metric": "polygon instances of one image as RLE dicts, ms per image (host clock; every call ends synchronised)", "file": fn,
           "image": [h, w], "instances": len(polys), "vertices": int(sum(len(p) // 2 for inst in polys for p in inst)),
           "counts": int(sum(len(rle.string_to_counts(c)) for c in first["device"])), "reps": a.reps, "warmup": a.warmup, "inner": a.inner}
    for key, t in ms.items():
        t = np.sort(np.asarray(t))
        out[key] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Polygon instances to run lists (tools/bench_polygons.py)\n\n")
            f.write(f"`python tools/bench_polygons.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} --md {a.md}`\n\n")
            f.write(f"{a.reps} timed samples after {a.warmup} warm-ups, the evaluations alternating in one process; a sample is the mean of {a.inner} "
                    "back-to-back calls.  Host clock, MI355X.  The paths are checked identical, every counts string, before anything is timed.  Speed "
                    "is recorded, not gated.\n")
            f.write(f"\n## {fn}: {h} x {w}, {out['instances']} instances, {out['vertices']} vertices, {out['counts']} counts\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            for k, label in NAMES.items():
                f.write(f"| {label} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")


if __name__ == "__main__":
    main()
