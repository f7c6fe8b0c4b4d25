"""Times the distance maps of masks on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations,
its polygons rasterised through masks_to_rle.  ALL instances in one call, at border_value 0: the statistics only (what inscribed_circles
asks for), the statistics with a 65-entry erosion curve (erosion_curve(masks, 64)), and the statistics with the map (mask_distance_maps).
Evaluations alternate inside one process, after a warm-up of each:

  scipy      what a user without this call does: per mask rle.decode, scipy.ndimage.distance_transform_edt with indices on the whole image
             padded by one zero (tests/mask_distance_ref.py), then the statistics, the curve or the crop from the dense array
  host       rle.mask_distance(ctx=None): amp_mask_distance with a NULL context (csrc/mask_distance_host.hip), from RLE dicts to arrays
  device     the same with the device's context (csrc/mask_distance.hip): upload, the launches, download, stream synchronise -- all in the window

The three are checked equal -- device == host byte for byte, both == the reference's integers -- before anything is timed.  Host and device
are sampled --reps times; the scipy loop takes seconds a sample, so it is sampled --ref-reps times where a sample takes less than --ref-budget
seconds and once (the checking pass) where it takes longer.  Also records VGPRs / LDS / scratch of the kernel from the compiler's resource
report.  Launches are counted from a kernel trace, which a profiler writes in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_mask_distance.py --trace-calls 4
    python tools/bench_mask_distance.py --kernel-trace DIR/.../*_kernel_trace.csv --trace-calls 4 --md profiles/r28/mask_distance.md

--trace-calls N alone makes N device calls with the curve and the map and nothing else (no warm-up: every dispatch of the process belongs to
one of them).  Prints one JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_mask_distance.py [--reps 21] [--warmup 2] [--ref-reps 3] [--ref-budget 15] [--md profiles/r28/mask_distance.md]
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

import mask_distance_ref as ref

WORK = [("statistics only", 0, False), ("statistics + 65-entry curve", 65, False), ("statistics + map", 0, True)]


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    return h, w, analyze.masks_to_rle(PolygonMasks(polys), (h, w), device="cpu")


def scipy_loop(rles, ncurve, want_map):
    """the same four arrays as rle.mask_distance, from one decoded mask and one whole-image transform per instance"""
    out = [ref.outputs(m, ref.scipy_d2(m, 0), (ncurve,)) for m in (rle.decode(x).astype(bool) for x in rles)]
    return (np.asarray([x["stats"] for x in out], np.int64).reshape(-1, 4), np.asarray([x["box"] for x in out], np.int64).reshape(-1, 4),
            np.asarray([x["curve"][ncurve] for x in out], np.int64).reshape(len(out), ncurve), [x["map"] for x in out] if want_map else None)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and (a[3] is None) == (b[3] is None) and \
        (a[3] is None or all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3])))


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/mask_distance.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "mask_distance.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"md_[a-z]+_kernel", m.group(1))
            name = k.group(0) if k else None
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = max(out[name].get(key, 0), int(m.group(1)))
    return out


def launches(path, calls):
    """{kernel: dispatches per call} from a kernel trace CSV of a --trace-calls run"""
    count = collections.Counter()
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("kernel_name") or ""
            k = re.search(r"md_[a-z]+_kernel", name)
            count[k.group(0) if k else name[:60]] += 1
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
    ap.add_argument("--kernel-trace", default=None, help="PATH of the kernel trace CSV of a --trace-calls run")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_mask_distance.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    ctx = analyze._current_device_context("bench_mask_distance")
    if a.trace_calls and not a.kernel_trace:
        for _ in range(a.trace_calls):
            rle.mask_distance(rles, 0, 65, True, ctx=ctx)
        ctx.sync()
        return

    n = len(rles)
    out = {"metric": "distance maps of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": n, "counts_in": int(sum(len(rle._counts(r)) for r in rles)), "reps": a.reps, "warmup": a.warmup,
           "ref_reps": a.ref_reps, "ref_budget_s": a.ref_budget, "kernels": kernel_resources(), "work": {}}
    for name, ncurve, want_map in WORK:
        fns = {"device": lambda: rle.mask_distance(rles, 0, ncurve, want_map, ctx=ctx), "host": lambda: rle.mask_distance(rles, 0, ncurve, want_map),
               "scipy": lambda: scipy_loop(rles, ncurve, want_map)}
        t = time.perf_counter()
        want = fns["scipy"]()
        ms = {"scipy": [(time.perf_counter() - t) * 1e3], "device": [], "host": []}
        dev, host = fns["device"](), fns["host"]()
        assert same(dev, host), "device and host disagree"
        assert same(host, want), "scipy disagrees"
        extra = {"pixels": int(host[0][:, 3].sum()), "largest_d2": int(host[0][:, 0].max()), "map_words": int(sum(m.size for m in host[3])) if want_map else 0}
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
    if a.kernel_trace:
        per = launches(a.kernel_trace, max(a.trace_calls, 1))
        out["launches_per_call"] = dict(per, total=sum(per.values()))
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Distance maps of the masks of one user-size image (tools/bench_mask_distance.py)\n\n")
            f.write(f"`python tools/bench_mask_distance.py --reps {a.reps} --warmup {a.warmup} --ref-reps {a.ref_reps} --ref-budget {a.ref_budget:g} --md ...`\n\n")
            first = next(iter(out["work"].values()))
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons rasterised through masks_to_rle), {n} masks of {out['counts_in']} counts and "
                    f"{first['pixels']} pixels in ONE call per evaluation, border_value 0; the largest squared distance of the image is {first['largest_d2']}.  "
                    f"{a.reps} timed samples after {a.warmup} warm-ups for the host and the device path, alternating in one process, every call ending in "
                    f"a stream synchronise.  The scipy loop (per mask: decode, scipy.ndimage.distance_transform_edt with indices on the whole padded "
                    f"image, the outputs from the dense array) is sampled {a.ref_reps} times where a sample takes less than {a.ref_budget:g} s and once, "
                    f"the checking pass, where it takes longer: the samples column says which.  Host clock, MI355X.  The three are checked equal (device "
                    f"== host byte for byte, both == the integers from scipy's indices) before anything is timed.  Speed is recorded, not gated.\n\n")
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
            f.write(f"\nThe map of the third row is {out['work'][WORK[2][0]]['map_words']} uint32 words, the sum of the box areas.\n")
            if out.get("launches_per_call"):
                f.write(f"\nLaunches per call (curve and map asked for), counted from a kernel trace of {a.trace_calls} device calls in a process of their "
                        f"own (a profiler run without timing; a memset the runtime performs as a kernel shows up under the runtime's name):\n\n"
                        f"| kernel | dispatches per call |\n|---|---|\n")
                for k, c in out["launches_per_call"].items():
                    f.write(f"| {k} | {c:g} |\n")
            else:
                f.write("\nLaunches per call: not counted in this run (no kernel trace was given); the code issues one memset and one md_tile_kernel launch.\n")
            f.write("\nKernel of csrc/mask_distance.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags):\n\n")
            f.write("| kernel | VGPRs | LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")
            own = [k for k, v in out["kernels"].items() if v.get("scratch")]
            f.write(f"\n{'No md_ kernel uses scratch: nothing of this file spills.' if not own else 'md_ kernels with scratch (spills): ' + ', '.join(own) + '.'}\n")


if __name__ == "__main__":
    main()
