"""Times region properties on a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations, its polygons
rasterised through masks_to_rle, ALL instances in one call.  Evaluations alternate inside one process, after a warm-up of each:

  device     amp_mask_region_props with a context (csrc/region_props.hip): upload, five launches, download, stream synchronise -- all in the window
  host       the same call with a NULL context (csrc/mask_analysis_host.hip)
  table-*    ampis_amd.analyze.region_properties(device='cuda' / 'cpu') from the RLE dicts, every key: the call plus run-length string decoding
             and the float derivation in Python -- what a user of the function waits for
  reference  the reference's method (ampis/structures.py:507): every mask decoded to the full image, then the dense scipy / numpy evaluation
             of tests/region_props_ref.py on it (skimage itself is not available here; this is the same erosion + convolution + hull per mask)

device and host are checked identical, and the reference equal to them on every integer, before anything is timed.  A device / host sample is
the mean over --inner back-to-back calls (one call is milliseconds: a single one would time the clock); the reference takes seconds and is
sampled --ref-reps times, in the first iterations.  Also records VGPRs / LDS / scratch of the kernels from the compiler's resource report.
Prints one JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_region_props.py [--reps 7] [--warmup 2] [--inner 20] [--ref-reps 2] [--md profiles/r10/region_props.md]
"""
import argparse
import ctypes as C
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


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys = [[np.stack([r["shape_attributes"]["all_points_x"], r["shape_attributes"]["all_points_y"]], axis=1).astype(np.float64).reshape(-1)]
             for r in img["regions"]]
    return h, w, analyze.masks_to_rle(PolygonMasks(polys), (h, w))


class Call:
    """amp_mask_region_props on arrays pooled once: what is timed is the C call alone."""

    def __init__(self, rles, h, w):
        self.n, self.h, self.w = len(rles), h, w
        self.pool = rle._pool([rle._counts(x) for x in rles])
        self.bbox, self.vals = np.zeros((self.n, 4), np.int64), np.zeros((self.n, 13), np.uint64)

    def __call__(self, ctx):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.lib().amp_mask_region_props(ctx.handle if ctx is not None else None, *(vp(a) for a in self.pool), self.n, self.h, self.w,
                                                    vp(self.bbox), vp(self.vals)), "amp_mask_region_props")
        return self.bbox.copy(), self.vals.copy()


def reference_method(rles):
    import region_props_ref as ref
    return [ref.ref_integers(rle.decode(r).astype(bool)) for r in rles]


def kernel_resources():
    """{kernel: (VGPRs, LDS bytes, scratch bytes / lane)} of csrc/region_props.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "region_props.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", m.group(1))
            name = re.match(r"rp_[a-z]+_kernel(ILb[01]E)?", name).group(0).replace("ILb0E", "<false>").replace("ILb1E", "<true>")
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--ref-reps", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_region_props.py measures on a HIP device and none is visible: not measured")
    h, w, rles = workload()
    call = Call(rles, h, w)
    ctx = _lib.Context(0)
    dev, host = call(ctx), call(None)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes(), "device and host paths disagree"
    want = reference_method(rles)
    assert all(tuple(b) == tuple(wb) and v == wv for b, v, (wb, wv) in zip(dev[0].tolist(), dev[1].tolist(), want)), "the reference's method disagrees"
    keys = list(analyze.RPROPS_KEYS)
    runs = {"device": (lambda: call(ctx), a.inner), "host": (lambda: call(None), a.inner),
            "table-cuda": (lambda: analyze.region_properties(rles, keys, device="cuda"), 1),
            "table-cpu": (lambda: analyze.region_properties(rles, keys, device="cpu"), 1), "reference": (lambda: reference_method(rles), 1)}
    ms = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):
        for name, (fn, inner) in runs.items():
            if name == "reference" and i >= a.ref_reps:              # the checking pass above was its warm-up
                continue
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3 / inner
            if name == "reference" or i >= a.warmup:
                ms[name].append(dt)
    boxes = dev[0]
    out = {"metric": "region properties of all instances of one 1024 x 1536 image in one call, ms per call (host clock around synchronised calls)",
           "image": [h, w], "masks": call.n, "mask_pixels": int(dev[1][:, 0].sum()), "runs": int(sum(len(rle._counts(x)) for x in rles)),
           "box_pixels": int(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).sum()), "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
           "ref_reps": a.ref_reps, "kernels": kernel_resources()}
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    ctx.close()
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Region properties on one user-size image (tools/bench_region_props.py)\n\n")
            f.write(f"Image {h} x {w} (tests/golden/via_subset.json, polygons rasterised through masks_to_rle), {call.n} masks in ONE call, {out['mask_pixels']} mask "
                    f"pixels in {out['runs']} runs, {out['box_pixels']} pixels of tight boxes.  {a.reps} timed samples after {a.warmup} warm-ups, the evaluations "
                    f"alternating in one process; a device / host sample is the mean of {a.inner} back-to-back calls, each ending in a stream synchronise; the "
                    f"reference's method is sampled {a.ref_reps} times after the checking pass.  Host clock, MI355X.\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            names = {"device": "device path (amp_mask_region_props, context; upload + 5 launches + download)", "host": "host path (amp_mask_region_props, NULL context)",
                     "table-cuda": "region_properties(device='cuda'), all 13 keys, from RLE dicts", "table-cpu": "region_properties(device='cpu'), all 13 keys, from RLE dicts",
                     "reference": "the reference's method: each mask decoded to the full image, dense scipy / numpy evaluation (tests/region_props_ref.py)"}
            for k in runs:
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")
            f.write("\nAll three agree on every integer (device == host byte for byte).  Speed is recorded, not gated.\n\n")
            f.write("Kernels of csrc/region_props.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags):\n\n")
            f.write("| kernel | VGPRs | LDS bytes / workgroup | scratch bytes / lane |\n|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('lds')} | {v.get('scratch')} |\n")


if __name__ == "__main__":
    main()
