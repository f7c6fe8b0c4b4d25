"""Times the grey-level statistics under the masks of a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most
annotations, its polygons rasterised through masks_to_rle.  The repository holds the annotations of that micrograph, not its pixels, so the
image is seeded noise of its size: uint8, grey [h, w] and RGB [h, w, 3]; the work does not depend on the values.  ALL instances in one call,
without and with the 256-bin histogram.  Evaluations alternate inside one process, after a warm-up of each:

  dense      what a user without this call does: per mask rle.decode to the full image and img[mask], then the sums, the extremes and
             np.bincount from the indexed values -- instances x image
  host       rle.mask_intensity(ctx=None): amp_mask_intensity with a NULL context (csrc/mask_intensity_host.hip), from RLE dicts to arrays
  device     the same with the device's context (csrc/mask_intensity.hip): upload of the image and the runs, the launches, download, stream
             synchronise -- all in the window

The three are checked equal -- device == host byte for byte, both == the dense loop's integers -- before anything is timed.  Every path is
sampled --reps times and the median is reported.  Also records VGPRs / LDS / scratch of the kernels from the compiler's resource report.
Prints one JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_mask_intensity.py [--reps 21] [--warmup 2] [--md profiles/r31/mask_intensity.md]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from ampis_amd import _lib, analyze, rle
from ampis_amd.structures import PolygonMasks

WORK = [("grey uint8", 0, None), ("grey uint8 + 256-bin histogram", 0, 0), ("RGB uint8", 3, None), ("RGB uint8 + 256-bin histogram", 3, 0)]


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    return h, w, analyze.masks_to_rle(PolygonMasks(polys), (h, w), device="cpu")


def dense_loop(rles, img, shift):
    """the same two arrays as rle.mask_intensity, from one decoded mask per instance"""
    hwc = img.reshape(img.shape[0], img.shape[1], -1)
    n, ch = len(rles), hwc.shape[2]
    vals = np.zeros((n, ch, 8), np.uint64)
    hist = None if shift is None else np.zeros((n, ch, 256 >> shift), np.uint32)
    for i, r in enumerate(rles):
        mask = rle.decode(r).astype(bool)
        rr, cc = np.nonzero(mask)
        px = hwc[mask].astype(np.uint64)                             # [N, ch]
        if len(px) == 0:
            continue
        vals[i, :, 0] = len(px)
        vals[i, :, 1] = px.sum(axis=0)
        vals[i, :, 2] = (px * px).sum(axis=0)
        vals[i, :, 3] = (rr.astype(np.uint64)[:, None] * px).sum(axis=0)
        vals[i, :, 4] = (cc.astype(np.uint64)[:, None] * px).sum(axis=0)
        vals[i, :, 5] = px.min(axis=0)
        vals[i, :, 6] = px.max(axis=0)
        if hist is not None:
            for k in range(ch):
                hist[i, k] = np.bincount(px[:, k].astype(np.int64) >> shift, minlength=hist.shape[2])
    return vals, hist


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and (a[1] is None) == (b[1] is None) and (a[1] is None or a[1].tobytes() == b[1].tobytes())


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/mask_intensity.hip from hipcc's resource report, built with the Makefile's
    flags; the largest over the uint8 and the uint16 instance of a kernel"""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "mask_intensity.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"mi_[a-z]+_kernel", m.group(1))
            name = k.group(0) if k else None
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = max(out[name].get(key, 0), int(m.group(1)))
    return out


def stats(t):
    t = np.sort(np.asarray(t))
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_mask_intensity.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    ctx = analyze._current_device_context("bench_mask_intensity")
    rng = np.random.RandomState(31)
    images = {0: rng.randint(0, 256, (h, w)).astype(np.uint8), 3: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)}
    n = len(rles)
    out = {"metric": "grey-level statistics of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": n, "counts_in": int(sum(len(rle._counts(r)) for r in rles)), "reps": a.reps, "warmup": a.warmup,
           "kernels": kernel_resources(), "work": {}}
    for name, ch, shift in WORK:
        img = images[ch]
        fns = {"device": lambda: rle.mask_intensity(rles, img, shift, ctx=ctx), "host": lambda: rle.mask_intensity(rles, img, shift),
               "dense": lambda: dense_loop(rles, img, shift)}
        want, dev, host = fns["dense"](), fns["device"](), fns["host"]()
        assert same(dev, host), "device and host disagree"
        assert same(host, want), "the dense loop disagrees"
        ms = {"device": [], "host": [], "dense": []}
        for i in range(a.warmup + a.reps):
            for path in ("device", "host", "dense"):
                ctx.sync(); torch.cuda.synchronize()
                t = time.perf_counter()
                fns[path]()
                ctx.sync()
                if i >= a.warmup:
                    ms[path].append((time.perf_counter() - t) * 1e3)
        out["work"][name] = dict({k: stats(v) for k, v in ms.items()}, pixels=int(host[0][:, 0, 0].sum()),
                                 hist_words=0 if host[1] is None else int(host[1].size))
        print(name, json.dumps(out["work"][name]), file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            first = next(iter(out["work"].values()))
            f.write("# Grey-level statistics under the masks of one user-size image (tools/bench_mask_intensity.py)\n\n")
            f.write(f"`python tools/bench_mask_intensity.py --reps {a.reps} --warmup {a.warmup} --md ...`\n\n")
            f.write(f"Image {h} x {w} (the annotations of tests/golden/via_subset.json, polygons rasterised through masks_to_rle; the pixels are seeded "
                    f"uint8 noise, the repository does not hold the micrograph's), {n} masks of {out['counts_in']} counts and {first['pixels']} pixels in "
                    f"ONE call per evaluation.  {a.reps} timed samples after {a.warmup} warm-ups for each of the three paths, alternating in one "
                    f"process, every call ending in a stream synchronise; medians.  The dense loop is per mask: rle.decode to the full image, "
                    f"img[mask], NumPy sums, extremes and bincount.  Host clock, MI355X.  The three are checked equal (device == host byte for byte, "
                    f"both == the dense loop's integers) before anything is timed.  Speed is recorded, not gated.\n\n")
            f.write("| work | device median ms (min .. max) | host median ms (min .. max) | dense loop median ms (min .. max) | device / host | dense / device |\n"
                    "|---|---|---|---|---|---|\n")
            behind = []
            for name, v in out["work"].items():
                dv, ho, de = v["device"], v["host"], v["dense"]
                f.write(f"| {name} | {dv['median_ms']} ({dv['min_ms']} .. {dv['max_ms']}) | {ho['median_ms']} ({ho['min_ms']} .. {ho['max_ms']}) | "
                        f"{de['median_ms']} ({de['min_ms']} .. {de['max_ms']}) | {dv['median_ms'] / ho['median_ms']:.2f} | {de['median_ms'] / dv['median_ms']:.0f} |\n")
                if dv["median_ms"] > 0.95 * ho["median_ms"]:
                    behind.append(name)
            f.write(f"\n{'The device path is ahead of the host path on every row.' if not behind else 'The device path is NOT ahead of the host path on: ' + ', '.join(behind) + '.'}\n")
            f.write(f"\nThe histograms of the second and fourth row are {out['work'][WORK[1][0]]['hist_words']} and {out['work'][WORK[3][0]]['hist_words']} "
                    f"uint32 words.\n")
            f.write("\nA device call, from the code (not traced in this run): three kernel launches whatever the masks hold -- mi_fill_kernel, "
                    "mi_transpose_kernel, mi_reduce_kernel --, five copies to the device (the image, the run starts, their prefix, the masks, the work "
                    "items) and one copy back (the per-mask words), two with a histogram.\n")
            f.write("\nKernels of csrc/mask_intensity.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags; the larger of the uint8 and "
                    "the uint16 instance; mi_reduce_kernel's LDS is dynamic, 4 bytes a bin: 1024 bytes at 256 bins, at most 16384):\n\n")
            f.write("| kernel | VGPRs | static LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")
            own = [k for k, v in out["kernels"].items() if v.get("scratch")]
            f.write(f"\n{'No mi_ kernel uses scratch: nothing of this file spills.' if not own else 'mi_ kernels with scratch (spills): ' + ', '.join(own) + '.'}\n")


if __name__ == "__main__":
    main()
