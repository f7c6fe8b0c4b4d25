"""Times mask morphology on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations, its
polygons rasterised through masks_to_rle.  ALL instances in one call: dilate, erode and open with the disk at radius 2 and 8, and boundary_iou
at the default ratio (d = 37 on this image) of every instance against itself dilated by a disk of radius 2.  Evaluations alternate inside one
process, after a warm-up of each:

  scipy      what a user without this call does: per mask rle.decode, scipy.ndimage.binary_dilation / binary_erosion with the element of
             tests/morphology_ref.py on the whole image, rle.encode (boundary_iou: the 3 x 3 erosion iterated d times on both masks of a pair)
  host       rle.morphology(ctx=None): amp_mask_morphology with a NULL context (csrc/morphology_host.hip), from RLE dicts to RLE dicts
  device     the same with the device's context (csrc/morphology.hip): upload, the launches, download, stream synchronise -- all in the window

The three are checked equal -- device == host byte for byte, both == scipy's encoded results -- before anything is timed.  Host and device are
sampled --reps times; the scipy loop takes seconds to minutes a sample, so it is sampled --ref-reps times where a sample takes less than
--ref-budget seconds and once (the checking pass) where it takes longer.  Also records VGPRs / LDS / scratch of the kernels from the
compiler's resource report.  Launches are counted from a kernel trace, which a profiler writes in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_morphology.py --trace-calls 4 --trace-op dilate
    python tools/bench_morphology.py --kernel-trace dilate=DIR/.../*_kernel_trace.csv --trace-calls 4 --md profiles/r26/morphology.md

--trace-calls N alone makes N device calls of --trace-op at radius 2 and nothing else (no warm-up: every dispatch of the process belongs to
one of them).  Prints one JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_morphology.py [--reps 21] [--warmup 2] [--ref-reps 3] [--ref-budget 15] [--md profiles/r26/morphology.md]
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
from scipy import ndimage

from ampis_amd import _lib, analyze, rle
from ampis_amd.structures import PolygonMasks

import morphology_ref as ref

WORK = [("dilate", 2), ("erode", 2), ("open", 2), ("dilate", 8), ("erode", 8), ("open", 8)]


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    return h, w, analyze.masks_to_rle(PolygonMasks(polys), (h, w), device="cpu")


def scipy_loop(rles, op, r):
    fp = ref.element("disk", r)
    out = []
    for x in rles:
        m = rle.decode(x).astype(bool)
        if op == "dilate":
            m = ref.dilate(m, fp)
        elif op == "erode":
            m = ref.erode(m, fp, 0)
        else:
            m = ref.dilate(ref.erode(m, fp, 0), fp)
        out.append(rle.encode(np.asfortranarray(m)))
    return out


def scipy_boundary_iou(gt, pred, d):
    ones = np.ones((3, 3), bool)
    inter, union = [], []
    for g, p in zip(gt, pred):
        g, p = rle.decode(g).astype(bool), rle.decode(p).astype(bool)
        bg = g & ~ndimage.binary_erosion(g, structure=ones, iterations=d, border_value=0)
        bp = p & ~ndimage.binary_erosion(p, structure=ones, iterations=d, border_value=0)
        inter.append(int((bg & bp).sum())); union.append(int((bg | bp).sum()))
    return np.asarray(inter, np.int64), np.asarray(union, np.int64)


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/morphology.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "morphology.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"(?:mo_[a-z]+|count_offsets|run_counts)_kernel", m.group(1))
            name = (k.group(0) + ("<EMIT>" if "ILb1E" in m.group(1) else "<COUNT>" if "ILb0E" in m.group(1) else "")) if k else \
                ("rocprim" if "rocprim" in m.group(1) else None)
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:                                           # rocprim's instantiations share one row: the largest of each figure
                out[name][key] = max(out[name].get(key, 0), int(m.group(1)))
    return out


def launches(path, calls):
    """{kernel: dispatches per call} from a kernel trace CSV of a --trace-calls run"""
    count = collections.Counter()
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("kernel_name") or ""
            k = re.search(r"(?:mo_[a-z]+|count_offsets|run_counts)_kernel", name)
            lib = (re.search(r"wrapped_(\w+?)_config", name) or re.search(r"(\w+)_kernel", name)) if "rocprim" in name else None
            count[k.group(0) if k else ("rocprim " + lib.group(1) if lib else name[:60])] += 1
    return {k: v / calls for k, v in sorted(count.items())}


def stats(t):
    t = np.sort(np.asarray(t))
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--ref-budget", type=float, default=15.0)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--trace-op", default="dilate")
    ap.add_argument("--kernel-trace", action="append", default=[], help="OP=PATH of a --trace-calls run of --trace-op OP")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_morphology.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    ctx = analyze._current_device_context("bench_morphology")
    if a.trace_calls and not a.kernel_trace:
        for _ in range(a.trace_calls):
            rle.morphology(rles, a.trace_op, "disk", 2, 0, ctx=ctx)
        ctx.sync()
        return

    n = len(rles)
    pred = rle.morphology(rles, "dilate", "disk", 2, 0)
    pairs = np.stack([np.arange(n), np.arange(n)], axis=1)
    runs = {}
    for op, r in WORK:
        runs[f"{op} disk {r}"] = {"device": (lambda op=op, r=r: rle.morphology(rles, op, "disk", r, 0, ctx=ctx)),
                                  "host": (lambda op=op, r=r: rle.morphology(rles, op, "disk", r, 0)),
                                  "scipy": (lambda op=op, r=r: scipy_loop(rles, op, r))}
    d = analyze.boundary_iou(rles, pred, matches=pairs, device="cpu")["distance"]
    biou = f"boundary_iou d = {d}"
    runs[biou] = {"device": lambda: analyze.boundary_iou(rles, pred, matches=pairs, device="cuda"),
                  "host": lambda: analyze.boundary_iou(rles, pred, matches=pairs, device="cpu"),
                  "scipy": lambda: scipy_boundary_iou(rles, pred, d)}
    out = {"metric": "mask morphology of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": n, "counts_in": int(sum(len(rle._counts(r)) for r in rles)), "reps": a.reps, "warmup": a.warmup,
           "ref_reps": a.ref_reps, "ref_budget_s": a.ref_budget, "kernels": kernel_resources(), "work": {}}
    for name, fns in runs.items():
        t = time.perf_counter()
        want = fns["scipy"]()
        ms = {"scipy": [(time.perf_counter() - t) * 1e3], "device": [], "host": []}
        dev, host = fns["device"](), fns["host"]()
        if name == biou:
            assert dev["boundary_iou"].tobytes() == host["boundary_iou"].tobytes() and dev["inter"].tolist() == host["inter"].tolist(), "device and host disagree"
            assert host["inter"].tolist() == want[0].tolist() and host["union"].tolist() == want[1].tolist(), "scipy disagrees"
            extra = {"mean_boundary_iou": round(float(np.nanmean(host["boundary_iou"])), 4)}
        else:
            assert [x["counts"] for x in dev] == [x["counts"] for x in host], "device and host disagree"
            assert [x["counts"] for x in host] == [x["counts"] for x in want], "scipy disagrees"
            extra = {"counts_out": int(sum(len(rle._counts(x)) for x in host)), "pixels_out": int(rle.area(host).sum(dtype=np.int64))}
        for _ in range((a.ref_reps - 1) if ms["scipy"][0] < a.ref_budget * 1e3 else 0):
            t = time.perf_counter()
            fns["scipy"]()
            ms["scipy"].append((time.perf_counter() - t) * 1e3)
        for i in range(a.warmup + a.reps):
            for path in ("device", "host"):
                ctx.sync(); torch.cuda.synchronize()
                t = time.perf_counter()
                fns[path]()
                ctx.sync()
                if i >= a.warmup:
                    ms[path].append((time.perf_counter() - t) * 1e3)
        out["work"][name] = dict({k: stats(v) for k, v in ms.items()}, **extra)
        print(name, json.dumps(out["work"][name]), file=sys.stderr, flush=True)
    for item in a.kernel_trace:
        op, path = item.split("=", 1)
        per = launches(path, max(a.trace_calls, 1))
        out.setdefault("launches_per_call", {})[op] = dict(per, total=sum(per.values()))
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Mask morphology of the masks of one user-size image (tools/bench_morphology.py)\n\n")
            f.write(f"`python tools/bench_morphology.py --reps {a.reps} --warmup {a.warmup} --ref-reps {a.ref_reps} --ref-budget {a.ref_budget:g} --md ...`\n\n")
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons rasterised through masks_to_rle), {n} masks of {out['counts_in']} counts in "
                    f"ONE call per evaluation; boundary_iou pairs every mask with itself dilated by a disk of radius 2.  {a.reps} timed samples after "
                    f"{a.warmup} warm-ups for the host and the device path, alternating in one process, every call ending in a stream synchronise.  The "
                    f"scipy loop (per mask: decode, scipy.ndimage on the whole image, encode) is sampled {a.ref_reps} times where a sample takes less "
                    f"than {a.ref_budget:g} s and once, the checking pass, where it takes longer: the samples column says which.  Host clock, MI355X.  "
                    f"The three are checked equal (device == host byte for byte, both == scipy's encoded results) before anything is timed.  Speed is "
                    f"recorded, not gated.\n\n")
            f.write("| work | device median ms (min .. max) | host median ms (min .. max) | scipy loop median ms (samples) | device / host | scipy / device |\n"
                    "|---|---|---|---|---|---|\n")
            behind = []
            for name, v in out["work"].items():
                dv, ho, sc = v["device"], v["host"], v["scipy"]
                f.write(f"| {name} | {dv['median_ms']} ({dv['min_ms']} .. {dv['max_ms']}) | {ho['median_ms']} ({ho['min_ms']} .. {ho['max_ms']}) | "
                        f"{sc['median_ms']} ({sc['samples']}) | {dv['median_ms'] / ho['median_ms']:.2f} | {sc['median_ms'] / dv['median_ms']:.0f} |\n")
                if dv["median_ms"] > 0.95 * ho["median_ms"]:
                    behind.append(name)
            f.write(f"\n{'The device path is ahead of the host path on every row.' if not behind else 'The device path is NOT ahead of the host path on: ' + ', '.join(behind) + '.'}\n")
            if out.get("launches_per_call"):
                for op, per in out["launches_per_call"].items():
                    f.write(f"\nLaunches per call of `{op}` (disk, radius 2), counted from a kernel trace of {a.trace_calls} device calls in a process of "
                            f"their own (a profiler run without timing):\n\n| kernel | dispatches per call |\n|---|---|\n")
                    for k, c in per.items():
                        f.write(f"| {k} | {c:g} |\n")
            else:
                f.write("\nLaunches per call: not counted in this run (no kernel trace was given).\n")
            f.write("\nKernels of csrc/morphology.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags; rocprim: the largest figure over "
                    "its sort and scan kernels as this file instantiates them):\n\n")
            f.write("| kernel | VGPRs | LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")
            own = [k for k, v in out["kernels"].items() if v.get("scratch") and k != "rocprim"]
            f.write(f"\n{'No mo_ kernel uses scratch: nothing of this file spills.' if not own else 'mo_ kernels with scratch (spills): ' + ', '.join(own) + '.'}")
            if out["kernels"].get("rocprim", {}).get("scratch"):
                f.write(f"  rocprim's radix sort of 64-bit keys has an instantiation with {out['kernels']['rocprim']['scratch']} bytes of scratch a lane; "
                        f"it is the library's kernel, built as the library configures it.")
            f.write("\n")


if __name__ == "__main__":
    main()
