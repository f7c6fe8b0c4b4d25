"""Times mask_topology and clean_masks on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations,
its polygons rasterised through masks_to_rle, and -- because hand-drawn polygons are clean and a pasted Mask R-CNN mask is not -- every instance
given what the repair is for: a pinhole at an interior pixel, a 2 x 2 hole beside it where it fits and a speck just outside its box (seeded,
the same on every run).  ALL instances in one call.  Evaluations alternate inside one process, after a warm-up of each:

  scipy-*    the composition users run today on one decoded full-image array per mask (scipy.ndimage only, skimage is not available here):
             topology = label + bincount, label of the complement, binary_fill_holes; clean = what remove_small_objects and remove_small_holes
             do (label, bincount, mask out; the same on the complement), then an encode
  host-*     analyze.mask_topology / analyze.clean_masks(device='cpu'): amp_mask_parts with a NULL context (csrc/mask_parts_host.hip), from RLE
             dicts to the dict of arrays / the list of RLE dicts
  device-*   the same with device='cuda' (csrc/mask_parts.hip): upload, the launches, download, stream synchronise -- all in the window

The three are checked equal -- device == host byte for byte, both == the scipy composition -- before anything is timed.  A host / device sample
is the mean over --inner back-to-back calls; the composition takes a minute and is sampled --ref-reps times, the checking pass being the first.  Also
records VGPRs / LDS / scratch of the kernels from the compiler's resource report.  Prints one JSON line; --md PATH also writes the figures as
a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_mask_parts.py [--reps 11] [--warmup 2] [--inner 5] [--ref-reps 1] [--md profiles/r18/mask_parts.md]
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

MIN_SIZE, AREA_THRESHOLD = 16, 16
FULL, CROSS = np.ones((3, 3), int), ndimage.generate_binary_structure(2, 1)


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    rng = np.random.default_rng(18)
    out = []
    for r in analyze.masks_to_rle(PolygonMasks(polys), (h, w), device="cpu"):
        m = rle.decode(r).astype(bool)
        ys, xs = np.nonzero(m)
        if len(ys):
            k = int(rng.integers(len(ys)))
            m[ys[k], xs[k]] = False                                  # a pinhole (on the rim it is a notch: that happens too)
            y, x = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])
            m[y:y + 2, x:x + 2] = False
            m[min(int(ys.max()) + 2, h - 1), min(int(xs.max()) + 2, w - 1)] = True       # a speck beside the particle
        out.append(rle.encode(np.asfortranarray(m)))
    return h, w, out


def scipy_topology(rles):
    rows = []
    for r in rles:
        m = rle.decode(r).astype(bool)
        lab, n = ndimage.label(m, structure=FULL)
        areas = np.bincount(lab.ravel())[1:]
        zl, zn = ndimage.label(~m, structure=CROSS)
        inner = np.setdiff1d(np.arange(1, zn + 1), np.concatenate([zl[0], zl[-1], zl[:, 0], zl[:, -1]]))
        rows.append((n, len(inner), n - len(inner), int(m.sum()), int(ndimage.binary_fill_holes(m).sum()), int(areas.max()) if n else 0))
    return np.array(rows, np.int64).reshape(-1, 6)


def scipy_clean(rles):
    out = []
    for r in rles:
        m = rle.decode(r).astype(bool)
        lab, _ = ndimage.label(m, structure=FULL)                    # remove_small_objects(m, MIN_SIZE, connectivity=2)
        small = np.bincount(lab.ravel()) < MIN_SIZE
        small[0] = False
        m = m & ~small[lab]
        lab, _ = ndimage.label(~m, structure=CROSS)                  # remove_small_holes(m, AREA_THRESHOLD): the small objects of ~m, 4 neighbours ...
        small = np.bincount(lab.ravel()) < AREA_THRESHOLD
        small[0] = False
        small[np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])] = False          # ... but background that reaches the border is no hole
        m = m | small[lab]
        out.append(rle.encode(np.asfortranarray(m)))
    return out


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/mask_parts.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "mask_parts.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"mp_[a-z]+_kernel", m.group(1))
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
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_mask_parts.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    topo = lambda device: analyze.mask_topology(rles, 2, device=device)
    clean = lambda device: analyze.clean_masks(rles, MIN_SIZE, AREA_THRESHOLD, connectivity=2, device=device)
    keys = ["n_parts", "n_holes", "euler_number", "area", "filled_area", "largest_part_area"]

    def timed(fn):
        t = time.perf_counter()
        res = fn()
        return res, (time.perf_counter() - t) * 1e3

    dev_t, host_t, (ref_t, ref_t_ms) = topo("cuda"), topo("cpu"), timed(lambda: scipy_topology(rles))
    assert all(dev_t[k].tobytes() == host_t[k].tobytes() for k in keys), "device and host topology disagree"
    assert np.stack([host_t[k] for k in keys], axis=1).tolist() == ref_t.tolist(), "the scipy composition disagrees on the topology"
    dev_c, host_c, (ref_c, ref_c_ms) = clean("cuda"), clean("cpu"), timed(lambda: scipy_clean(rles))
    assert dev_c == host_c, "device and host cleaning disagree"
    assert host_c == ref_c, "the scipy composition disagrees on the cleaned masks"
    ctx = analyze._current_device_context("bench_mask_parts")
    runs = {"device-topology": (lambda: topo("cuda"), a.inner), "host-topology": (lambda: topo("cpu"), a.inner),
            "device-clean": (lambda: clean("cuda"), a.inner), "host-clean": (lambda: clean("cpu"), a.inner),
            "scipy-topology": (lambda: scipy_topology(rles), 1), "scipy-clean": (lambda: scipy_clean(rles), 1)}
    ms = {k: [] for k in runs}
    ms["scipy-topology"].append(ref_t_ms); ms["scipy-clean"].append(ref_c_ms)      # the checking pass is the composition's first sample: it takes seconds
    for i in range(a.warmup + a.reps):
        for name, (fn, inner) in runs.items():
            ref = name.startswith("scipy")
            if ref and i >= a.ref_reps - 1:
                continue
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3 / inner
            if ref or i >= a.warmup:
                ms[name].append(dt)
    changed = sum(x != y for x, y in zip(rles, host_c))
    out = {"metric": "mask_topology / clean_masks of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": len(rles), "mask_pixels": int(host_t["area"].sum()), "counts": int(sum(len(rle._counts(x)) for x in rles)),
           "parts": int(host_t["n_parts"].sum()), "holes": int(host_t["n_holes"].sum()), "masks_changed_by_cleaning": int(changed),
           "min_size": MIN_SIZE, "area_threshold": AREA_THRESHOLD, "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "ref_reps": a.ref_reps,
           "kernels": kernel_resources()}
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Parts and holes of the masks of one user-size image (tools/bench_mask_parts.py)\n\n")
            f.write(f"`python tools/bench_mask_parts.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} --ref-reps {a.ref_reps} --md ...`\n\n")
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons rasterised through masks_to_rle, every instance given a pinhole, a 2 x 2 hole and a "
                    f"speck), {len(rles)} masks in ONE call, {out['mask_pixels']} mask pixels in {out['counts']} counts, {out['parts']} parts and {out['holes']} "
                    f"holes; cleaning with min_size = {MIN_SIZE}, area_threshold = {AREA_THRESHOLD} at connectivity 2 changes {changed} masks.  {a.reps} timed "
                    f"samples after {a.warmup} warm-ups, the evaluations alternating in one process; a host / device sample is the mean of {a.inner} back-to-back "
                    f"calls, each ending in a stream synchronise; the scipy composition is sampled {a.ref_reps} times, the checking pass included.  Host clock, "
                    f"MI355X.  The three are checked equal (device == host byte for byte) before anything is timed.  Speed is recorded, not gated.\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            names = {"scipy-topology": "scipy composition on decoded masks: label, label of the complement, binary_fill_holes",
                     "host-topology": "mask_topology(device='cpu'): two statistics-only amp_mask_parts calls, NULL context",
                     "device-topology": "mask_topology(device='cuda'): two statistics-only calls; upload, 5 launches, download each",
                     "scipy-clean": "scipy composition on decoded masks: remove small objects, remove small holes, encode",
                     "host-clean": "clean_masks(device='cpu'): two emitting amp_mask_parts calls, NULL context, counts strings",
                     "device-clean": "clean_masks(device='cuda'): two emitting calls; upload, 8 launches, download each, counts strings"}
            for k in ("scipy-topology", "host-topology", "device-topology", "scipy-clean", "host-clean", "device-clean"):
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")
            f.write("\nKernels of csrc/mask_parts.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags):\n\n")
            f.write("| kernel | VGPRs | LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")


if __name__ == "__main__":
    main()
