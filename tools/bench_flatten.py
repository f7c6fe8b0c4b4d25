"""Times resolve_overlaps and instances_to_label_image on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the
most annotations, its polygons rasterised through masks_to_rle, and -- because hand-drawn polygons hardly overlap and pasted Mask R-CNN masks do
-- every mask grown by 2 .. 5 pixels (binary dilation, seeded, the same on every run) so that neighbours really share a rim.  ALL instances in
one call, priority 'area'.  Evaluations alternate inside one process, after a warm-up of each:

  dense      the loop users run today: decode each mask, labels[m] = i + 1 in reverse priority, then encode(labels == i + 1) per instance
  host-*     analyze.resolve_overlaps / instances_to_label_image(device='cpu'): amp_flatten_instances with a NULL context
             (csrc/flatten_host.hip), from RLE dicts to the list of RLE dicts / the label image
  device-*   the same with device='cuda' (csrc/flatten.hip): upload, the launches, download, stream synchronise -- all in the window

The three are checked equal -- device == host byte for byte, both == the dense loop -- before anything is timed.  A host / device sample is the
mean over --inner back-to-back calls; the dense loop takes seconds and is sampled --ref-reps times, the checking pass being the first.  Also
records VGPRs / LDS / scratch of the kernels from the compiler's resource report.  Prints one JSON line; --md PATH also writes the figures as
a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_flatten.py [--reps 11] [--warmup 2] [--inner 5] [--ref-reps 2] [--md profiles/r19/flatten.md]
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
from scipy import ndimage

from ampis_amd import _lib, analyze, rle
from ampis_amd.structures import PolygonMasks


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    rng = np.random.default_rng(19)
    out = []
    for r in analyze.masks_to_rle(PolygonMasks(polys), (h, w), device="cpu"):
        m = ndimage.binary_dilation(rle.decode(r).astype(bool), iterations=int(rng.integers(2, 6)))
        out.append(rle.encode(np.asfortranarray(m)))
    return h, w, out


def dense_loop(rles, h, w):
    """(visible RLE dicts, label image) the way users do it today, priority 'area': smaller masks on top, ties to the lower index"""
    masks = [rle.decode(r).astype(bool) for r in rles]
    areas = np.array([int(m.sum()) for m in masks], np.int64)
    labels = np.zeros((h, w), np.int32)
    for i in np.argsort(areas, kind="stable")[::-1]:
        labels[masks[i]] = i + 1
    return [rle.encode(np.asfortranarray(labels == i + 1)) for i in range(len(rles))], labels


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/flatten.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "flatten.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"(fl|lr)_[a-z]+_kernel", m.group(1))
            name = k.group(0) if k else None
            if name:
                out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_flatten.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    resolve = lambda device: analyze.resolve_overlaps(rles, "area", device=device, return_stats=True)
    label = lambda device: analyze.instances_to_label_image(rles, "area", device=device)

    t = time.perf_counter()
    ref, ref_labels = dense_loop(rles, h, w)
    ref_ms = (time.perf_counter() - t) * 1e3
    (dev, dev_s), (host, host_s) = resolve("cuda"), resolve("cpu")
    assert dev == host and all(dev_s[k].tobytes() == host_s[k].tobytes() for k in host_s), "device and host disagree"
    assert host == ref, "the dense loop disagrees on the visible masks"
    assert label("cuda").tobytes() == label("cpu").tobytes() == ref_labels.tobytes(), "the label images disagree"
    ctx = analyze._current_device_context("bench_flatten")
    runs = {"device-resolve": (lambda: resolve("cuda"), a.inner), "host-resolve": (lambda: resolve("cpu"), a.inner),
            "device-label": (lambda: label("cuda"), a.inner), "host-label": (lambda: label("cpu"), a.inner),
            "dense": (lambda: dense_loop(rles, h, w), 1)}
    ms = {k: [] for k in runs}
    ms["dense"].append(ref_ms)                                       # the checking pass is the dense loop's first sample: it takes seconds
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
    px = host_s["pixels"]
    out = {"metric": "resolve_overlaps / instances_to_label_image of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": len(rles), "mask_pixels": int(host_s["area"].sum()), "visible_pixels": int(host_s["visible_area"].sum()),
           "pixels_none_one_more": [int(v) for v in px], "counts_in": int(sum(len(rle._counts(x)) for x in rles)),
           "counts_out": int(sum(len(rle._counts(x)) for x in host)), "masks_that_lost_pixels": int((host_s["visible_area"] < host_s["area"]).sum()),
           "priority": "area", "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "ref_reps": a.ref_reps, "kernels": kernel_resources()}
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Overlap-free instances of one user-size image (tools/bench_flatten.py)\n\n")
            f.write(f"`python tools/bench_flatten.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} --ref-reps {a.ref_reps} --md ...`\n\n")
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons rasterised through masks_to_rle, every mask grown by 2 .. 5 pixels, seeded), "
                    f"{len(rles)} masks in ONE call at priority 'area': {out['mask_pixels']} mask pixels in {out['counts_in']} counts, {int(px[2])} pixels under "
                    f"two or more masks, {out['masks_that_lost_pixels']} masks lose pixels, {out['visible_pixels']} visible pixels in {out['counts_out']} counts.  "
                    f"{a.reps} timed samples after {a.warmup} warm-ups, the evaluations alternating in one process; a host / device sample is the mean of "
                    f"{a.inner} back-to-back calls, each ending in a stream synchronise; the dense loop is sampled {a.ref_reps} times, the checking pass "
                    f"included.  Host clock, MI355X.  The three are checked equal (device == host byte for byte) before anything is timed.  Speed is "
                    f"recorded, not gated.\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            names = {"dense": "dense loop: decode each mask, labels[m] = i + 1 in reverse priority, encode(labels == i + 1) per instance",
                     "host-resolve": "resolve_overlaps(device='cpu'): one emitting amp_flatten_instances call, NULL context, counts strings",
                     "device-resolve": "resolve_overlaps(device='cuda'): one emitting call; upload, the launches, download, counts strings",
                     "host-label": "instances_to_label_image(device='cpu'): one call without lists, NULL context",
                     "device-label": "instances_to_label_image(device='cuda'): one call without lists; upload, 1 launch, download of the label image"}
            for k in ("dense", "host-resolve", "device-resolve", "host-label", "device-label"):
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")
            f.write("\nKernels of csrc/flatten.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags; the lr_ kernels are those of "
                    "label_runs_kernels.h as this file instantiates them):\n\n")
            f.write("| kernel | VGPRs | LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")


if __name__ == "__main__":
    main()
