"""Times the instance overlay of a user-size image: the 1024 x 1536 micrograph of tests/golden/via_subset.json with the most annotations, its 351
polygons rasterised through masks_to_rle, with their boxes and fixed colours, ALL instances in one call.  Evaluations alternate inside one
process, after a warm-up of each:

  device         amp_render_instances with a context (csrc/render.hip): upload, one launch, download, stream synchronise -- all in the window
  host           the same call with a NULL context (csrc/mask_analysis_host.hip)
  overlay-*      Visualizer(img).overlay_instances(masks=RLE dicts, boxes=, assigned_colors=) end to end, drawn on the device ('cuda') or on the
                 host ('cpu'), without and with one label per instance (the labels are one PIL session)
  dense          the drawing as it was before the one call: every mask decoded to the full image, Visualizer.draw_binary_mask + draw_box per
                 instance, and with labels one Visualizer.draw_text (a PIL round trip of the image) per label

device, host and dense are checked identical byte for byte before anything is timed.  A device / host sample is the mean over --inner
back-to-back calls; the dense drawing takes seconds and is sampled --dense-reps times.  Also records VGPRs / LDS / scratch / occupancy of the
kernel from the compiler's resource report.  Prints one JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device:
there is no figure without one.

    python tools/bench_render.py [--reps 7] [--warmup 2] [--inner 10] [--dense-reps 2] [--md profiles/r16/render.md]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from ampis_amd import _lib, analyze, rle
from ampis_amd.structures import PolygonMasks
from ampis_amd.utils.visualizer import Visualizer


def workload():
    via = json.load(open(os.path.join(ROOT, "tests", "golden", "via_subset.json")))["via"]["_via_img_metadata"]
    img = max(via.values(), key=lambda v: len(v["regions"]))
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    xs = [np.asarray(r["shape_attributes"]["all_points_x"], np.float64) for r in img["regions"]]
    ys = [np.asarray(r["shape_attributes"]["all_points_y"], np.float64) for r in img["regions"]]
    polys = [[np.stack([x, y], axis=1).reshape(-1)] for x, y in zip(xs, ys)]
    boxes = np.array([[x.min(), y.min(), x.max(), y.max()] for x, y in zip(xs, ys)], np.float64)
    yy, xx = np.mgrid[:h, :w]
    image = np.stack([(yy * 7 + xx * 13) % 256, (yy * 11 + xx * 3 + 97) % 256, (yy + xx * 5) % 256], axis=2).astype(np.uint8)
    n = len(polys)
    colors = np.stack([(np.arange(n) * 37 % 101) / 100.0, (np.arange(n) * 53 % 89) / 88.0, (np.arange(n) * 71 % 97) / 96.0], axis=1)
    return image, analyze.masks_to_rle(PolygonMasks(polys), (h, w)), boxes, colors


def dense_overlay(image, rles, boxes, colors, labels=None):
    """overlay_instances as it was: decode, draw_binary_mask, draw_box per instance; one draw_text per label"""
    vis = Visualizer(image)
    order = analyze.render_order(boxes, len(rles))
    for i in order:
        vis.draw_binary_mask(rle.decode(rles[i]).astype(bool), colors[i], alpha=0.5)
        vis.draw_box(boxes[i], colors[i])
    if labels is not None:
        for i in order:
            vis.draw_text(labels[i], (boxes[i][0], boxes[i][1]))
    return vis.output.img


def overlay(image, rles, boxes, colors, device, labels=None):
    vis = Visualizer(image)
    vis.render_device = device
    return vis.overlay_instances(masks=rles, boxes=boxes, assigned_colors=colors, labels=labels).get_image()


def kernel_resources():
    """{kernel: VGPRs, LDS bytes, scratch bytes / lane, occupancy} of csrc/render.hip from hipcc's resource report, built with the Makefile's flags."""
    src = os.path.join(ROOT, "ampis_amd", "csrc", "render.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"render_kernel", m.group(1))
            name = name.group(0) if name else None
            if name:
                out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--dense-reps", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_render.py measures on a HIP device and none is visible: not measured")
    image, rles, boxes, colors = workload()
    h, w = image.shape[:2]
    n = len(rles)
    labels = [f"particle {i}" for i in range(n)]
    order = analyze.render_order(boxes, n)
    lw = max(1, round(max(h, w) / 600))
    tables, edge_rgb, ibox, box_rgb = analyze.render_inputs(colors[order], 0.5, boxes[order], h, w)
    ordered = [dict(r, counts=rle._counts(r)) for r in (rles[i] for i in order)]       # run lengths decoded once: the C call alone is timed
    call = lambda ctx: rle.render_instances(image, ordered, tables, edge_rgb, ibox, box_rgb, lw, ctx=ctx)
    ctx = _lib.Context(0)
    dev, host = call(ctx), call(None)
    assert dev.tobytes() == host.tobytes(), "device and host paths disagree"
    t = time.perf_counter()
    want = dense_overlay(image, rles, boxes, colors)
    first_dense = (time.perf_counter() - t) * 1e3
    assert dev.tobytes() == want.tobytes(), "the dense drawing disagrees"
    assert overlay(image, rles, boxes, colors, "cuda", labels).tobytes() == dense_overlay(image, rles, boxes, colors, labels).tobytes(), "labels disagree"
    runs = {"device": (lambda: call(ctx), a.inner), "host": (lambda: call(None), a.inner),
            "overlay-cuda": (lambda: overlay(image, rles, boxes, colors, "cuda"), 1), "overlay-cpu": (lambda: overlay(image, rles, boxes, colors, "cpu"), 1),
            "overlay-cuda-labels": (lambda: overlay(image, rles, boxes, colors, "cuda", labels), 1),
            "overlay-cpu-labels": (lambda: overlay(image, rles, boxes, colors, "cpu", labels), 1),
            "dense": (lambda: dense_overlay(image, rles, boxes, colors), 1), "dense-labels": (lambda: dense_overlay(image, rles, boxes, colors, labels), 1)}
    ms = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):
        for name, (fn, inner) in runs.items():
            if name.startswith("dense") and i >= a.dense_reps:       # the checking passes above were its warm-up
                continue
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3 / inner
            if name.startswith("dense") or i >= a.warmup:
                ms[name].append(dt)
    out = {"metric": "overlay of all instances of one 1024 x 1536 image, ms per call (host clock around synchronised calls)", "image": [h, w],
           "instances": n, "mask_pixels": int(sum(int(rle.area(r)) for r in rles)), "runs": int(sum(len(rle._counts(x)) for x in rles)),
           "changed_pixels": int((dev != image).any(axis=2).sum()), "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
           "dense_reps": a.dense_reps, "first_dense_ms": round(first_dense, 1), "kernels": kernel_resources()}
    for name, t in ms.items():
        t = np.sort(np.asarray(t))
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    ctx.close()
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Instance overlay of one user-size image (tools/bench_render.py)\n\n")
            f.write(f"Image {h} x {w} (synthetic pixels; the masks are the polygons of tests/golden/via_subset.json rasterised through masks_to_rle), {n} instances "
                    f"with boxes and fixed colours in ONE call, {out['mask_pixels']} mask pixels in {out['runs']} runs, {out['changed_pixels']} pixels changed.  "
                    f"{a.reps} timed samples after {a.warmup} warm-ups, the evaluations alternating in one process; a device / host sample is the mean of "
                    f"{a.inner} back-to-back calls, each ending in a stream synchronise; the dense drawing is sampled {a.dense_reps} times after the checking "
                    f"pass.  Host clock, MI355X.\n\n")
            f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
            names = {"device": "device path (amp_render_instances, context; upload + 1 launch + download)", "host": "host path (amp_render_instances, NULL context)",
                     "overlay-cuda": "Visualizer.overlay_instances from RLE dicts, drawn on the device, no labels",
                     "overlay-cpu": "Visualizer.overlay_instances from RLE dicts, drawn on the host, no labels",
                     "overlay-cuda-labels": f"the same on the device with {n} labels (one PIL session)",
                     "overlay-cpu-labels": f"the same on the host with {n} labels (one PIL session)",
                     "dense": "the drawing before the one call: decode + draw_binary_mask + draw_box per instance, no labels",
                     "dense-labels": f"the same with {n} labels (one draw_text, a PIL round trip of the image, each)"}
            for k in runs:
                f.write(f"| {names[k]} | {out[k]['median_ms']} | {out[k]['min_ms']} | {out[k]['max_ms']} | {out[k]['samples']} |\n")
            f.write("\nDevice, host and the dense drawing agree byte for byte, with and without labels.  Speed is recorded, not gated.\n\n")
            f.write("Kernel of csrc/render.hip (hipcc -Rpass-analysis=kernel-resource-usage, the build's flags):\n\n")
            f.write("| kernel | VGPRs | SGPRs | LDS bytes / workgroup | scratch bytes / lane | occupancy waves / SIMD |\n|---|---|---|---|---|---|\n")
            for k, v in out["kernels"].items():
                f.write(f"| {k} | {v.get('vgprs')} | {v.get('sgprs')} | {v.get('lds')} | {v.get('scratch')} | {v.get('occupancy')} |\n")


if __name__ == "__main__":
    main()
