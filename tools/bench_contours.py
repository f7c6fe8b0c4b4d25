"""Times mask_contours on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations, its polygons
rasterised through masks_to_rle.  ALL instances in one call, connectivity 2.  Evaluations alternate inside one process, after a warm-up of each:

  dense      the reference tracer of the tests (tests/contours_ref.py): decode each mask, collect its unit boundary edges, walk them
  host       rle.mask_contours(ctx=None): amp_mask_contours with a NULL context (csrc/contours_host.hip), from RLE dicts to the flat arrays
  device     the same with the device's context (csrc/contours.hip): upload, the launches, download, stream synchronise -- all in the window

The three are checked equal -- device == host byte for byte, both == the dense tracer ring for ring -- before anything is timed.  A host /
device sample is the mean over --inner back-to-back calls; the dense tracer takes seconds and is sampled --ref-reps times, the checking pass
being the first.  Also records VGPRs / LDS / scratch of the kernels from the compiler's resource report and the number of pointer-jumping
rounds.  Launches are counted from a kernel trace, which a profiler writes in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_contours.py --trace-calls 4
    python tools/bench_contours.py --kernel-trace DIR/.../*_kernel_trace.csv --trace-calls 4 --md profiles/r23/mask_contours.md

--trace-calls N alone makes N device calls and nothing else (no warm-up: every dispatch of the process belongs to one of them).  Prints one
JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_contours.py [--reps 11] [--warmup 2] [--inner 5] [--ref-reps 1] [--md profiles/r23/mask_contours.md]
"""
import argparse
import collections
import csv
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from ampis_amd import _lib, analyze, rle
from ampis_amd.structures import PolygonMasks

import contours_ref


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    return h, w, analyze.masks_to_rle(PolygonMasks(polys), (h, w), device="cpu")


def dense_tracer(rles):
    """per mask the rings of tests/contours_ref.py, the way a user without this call would get them: decode, then trace"""
    return [contours_ref.rings(rle.decode(r).astype(bool), 2) for r in rles]


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/contours.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "contours.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"ct_[a-z]+_kernel", m.group(1))
            name = k.group(0) if k else ("rocprim" if "rocprim" in m.group(1) else None)
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:                                           # rocprim's instantiations share one row: the largest of each figure
                out[name][key] = max(out[name].get(key, 0), int(m.group(1)))
    return out


def most_pieces(counts, h):
    """an upper bound on the vertical pieces of one mask: every run of ones cut at the column ends it crosses"""
    best = 0
    for c in counts:
        b = np.cumsum(c.astype(np.int64))
        e = b[1::2]
        s = b[0::2][: len(e)]
        keep = e > s
        best = max(best, int(((e[keep] - 1) // h - s[keep] // h + 1).sum()))
    return best


def launches(path, calls):
    """{kernel: dispatches per call} from a kernel trace CSV of a --trace-calls run"""
    count = collections.Counter()
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("kernel_name") or ""
            k = re.search(r"ct_[a-z]+_kernel", name)
            lib = (re.search(r"wrapped_(\w+?)_config", name) or re.search(r"(\w+)_kernel", name)) if "rocprim" in name else None
            count[k.group(0) if k else ("rocprim " + lib.group(1) if lib else name[:60])] += 1
    return {k: v / calls for k, v in sorted(count.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_contours.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    ctx = analyze._current_device_context("bench_contours")
    if a.trace_calls and not a.kernel_trace:
        for _ in range(a.trace_calls):
            rle.mask_contours(rles, 2, ctx=ctx)
        ctx.sync()
        return

    t = time.perf_counter()
    ref = dense_tracer(rles)
    ref_ms = (time.perf_counter() - t) * 1e3
    dev, host = rle.mask_contours(rles, 2, ctx=ctx), rle.mask_contours(rles, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dev, host)), "device and host disagree"
    first, off, ln, area2, length, xy = host
    flat = [r for m in ref for r in m]
    assert first.tolist() == np.cumsum([0] + [len(m) for m in ref]).tolist() and len(flat) == len(off), "the dense tracer disagrees on the rings"
    assert xy.tobytes() == np.concatenate([r["xy"] for r in flat]).tobytes() and area2.tolist() == [r["area2"] for r in flat] \
        and length.tolist() == [r["length"] for r in flat], "the dense tracer disagrees on the corners"
    arrays = [{"size": r["size"], "counts": rle._counts(r)} for r in rles]              # the counts strings read once: the C call and its copies alone
    runs = {"device": (lambda: rle.mask_contours(rles, 2, ctx=ctx), a.inner), "host": (lambda: rle.mask_contours(rles, 2), a.inner),
            "device-arrays": (lambda: rle.mask_contours(arrays, 2, ctx=ctx), a.inner), "host-arrays": (lambda: rle.mask_contours(arrays, 2), a.inner),
            "dense": (lambda: dense_tracer(rles), 1)}
    ms = {k: [] for k in runs}
    ms["dense"].append(ref_ms)                                       # the checking pass is the dense tracer's first sample: it takes seconds
    for i in range(a.warmup + a.reps):
        for name, (fn, inner) in runs.items():
            ref_run = name == "dense"
            if ref_run and i >= a.ref_reps - 1:
                continue
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3 / inner
            if ref_run or i >= a.warmup:
                ms[name].append(dt)
    counts = [rle._counts(r) for r in rles]
    most = most_pieces(counts, h)
    rounds = int(np.ceil(np.log2(max(2 * most, 2))))
    out = {"metric": "mask_contours of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": len(rles), "mask_pixels": int(area2.sum() // 2), "counts_in": int(sum(len(c) for c in counts)),
           "rings": int(len(off)), "hole_rings": int((area2 < 0).sum()), "vertices": int(len(xy)), "connectivity": 2,
           "jumping_rounds_at_most": rounds, "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "ref_reps": a.ref_reps, "kernels": kernel_resources()}
    if a.kernel_trace:
        out["launches_per_call"] = launches(a.kernel_trace, max(a.trace_calls, 1))
        out["launches_per_call_total"] = sum(out["launches_per_call"].values())
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Boundary rings of the masks of one user-size image (tools/bench_contours.py)\n\n")
            f.write(f"`python tools/bench_contours.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} --ref-reps {a.ref_reps} --md ...`\n\n")
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons rasterised through masks_to_rle), {len(rles)} masks in ONE call at "
                    f"connectivity 2: {out['mask_pixels']} mask pixels in {out['counts_in']} counts give {out['rings']} rings ({out['hole_rings']} of "
                    f"them holes) with {out['vertices']} vertices.  {a.reps} timed samples after {a.warmup} warm-ups, the evaluations alternating in "
                    f"one process; a host / device sample is the mean of {a.inner} back-to-back calls, each ending in a stream synchronise; the dense "
                    f"tracer is sampled {a.ref_reps} times, the checking pass included.  Host clock, MI355X.  The three are checked equal (device == "
                    f"host byte for byte, both == the dense tracer ring for ring) before anything is timed.  Speed is recorded, not gated.\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            names = {"dense": "dense tracer (tests/contours_ref.py): decode each mask, collect its unit boundary edges, walk them",
                     "host": "rle.mask_contours(ctx=None): one amp_mask_contours call, NULL context",
                     "device": "rle.mask_contours(ctx=device): one call; upload, the launches, download",
                     "host-arrays": "the host path from uint32 counts arrays instead of counts strings",
                     "device-arrays": "the device path from uint32 counts arrays instead of counts strings"}
            for k in ("dense", "host", "device", "host-arrays", "device-arrays"):
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")
            ratio = out["device"]["median_ms"] / out["host"]["median_ms"]
            verdict = "ahead" if ratio < 0.95 else "NOT ahead: the host walk is the faster one here" if ratio > 1.05 else "level with it, not ahead"
            f.write(f"\nThe device path takes {ratio:.2f} x the host path's time at this size ({verdict}); from counts arrays "
                    f"{out['device-arrays']['median_ms'] / out['host-arrays']['median_ms']:.2f} x.\n")
            if a.kernel_trace:
                f.write(f"\nLaunches per call, counted from a kernel trace of {a.trace_calls} device calls in a process of their own (a profiler run "
                        f"without timing); at most {rounds} pointer-jumping rounds for this image, each phase as many:\n\n| kernel | dispatches per call |\n|---|---|\n")
                for k, v in out["launches_per_call"].items():
                    f.write(f"| {k} | {v:g} |\n")
                f.write(f"| total | {out['launches_per_call_total']:g} |\n")
            else:
                f.write("\nLaunches per call: not counted in this run (no kernel trace was given).\n")
            f.write("\nKernels of csrc/contours.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags; rocprim: the largest figure "
                    "over its sort and scan kernels as this file instantiates them):\n\n")
            f.write("| kernel | VGPRs | LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")
            own = [k for k, v in out["kernels"].items() if v.get("scratch") and k != "rocprim"]
            f.write(f"\n{'No ct_ kernel uses scratch: nothing of this file spills.' if not own else 'ct_ kernels with scratch (spills): ' + ', '.join(own) + '.'}")
            if out["kernels"].get("rocprim", {}).get("scratch"):
                f.write(f"  rocprim's radix sort of 64-bit keys has an instantiation with {out['kernels']['rocprim']['scratch']} bytes of scratch a lane; "
                        f"it is the library's kernel, built as the library configures it; the kernel trace's Scratch_Size column says whether a call dispatched it.")
            f.write("\n")

if __name__ == "__main__":
    main()
