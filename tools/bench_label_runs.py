"""Times the ingestion of an annotation image on two inputs: a spheroidite annotation (tests/golden/spheroidite_annotations, about 483 x 645, 598
components) and a synthetic 1024 x 1536 label image of about 350 blobs, the size and instance count of a powder micrograph.  Evaluations
alternate inside one process, after a warm-up of each:

  device      analyze.label_image_to_rle(device='cuda'): amp_label_runs with a context (csrc/label_runs.hip: upload, the launches, download, stream
              synchronise) plus the counts strings -- all in the window
  host        the same with device='cpu' (csrc/label_runs_host.hip)
  previous    the method the callers used before, the reference's (ampis/data_utils.py:412-428): scipy.ndimage.label, one dense `lab == v` mask,
              extract_boxes and rle.encode per instance
  ddicts-*    data_utils.get_ddicts('binary', device='cuda' / 'cpu') end to end on a folder that holds the one annotation as a PNG of its foreground:
              file read included; for the label image also get_ddicts('label') on the ids as .npy (ddicts-label-*)

device, host and previous are checked identical -- every box and every counts string -- before anything is timed.  The previous method takes
seconds and is sampled --ref-reps times.  Prints one JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device:
there is no figure without one.

    python tools/bench_label_runs.py [--reps 7] [--warmup 2] [--inner 5] [--ref-reps 2] [--md profiles/r15/label_runs.md]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from ampis_amd import _lib, analyze, data_utils, rle

ANNOTATION = os.path.join(ROOT, "tests", "golden", "spheroidite_annotations", "train_800C-24H-Q-2_sizeRC_484_645.png")


def spheroidite():
    from PIL import Image
    a = np.asarray(Image.open(ANNOTATION))
    return (a if a.ndim == 2 else a[..., 0]).astype(bool)


def powder(h=1024, w=1536, n=350, seed=7):
    """Discs of radius 8 .. 30 at seeded positions, later ones on top: a label image of at most n ids"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    lab = np.zeros((h, w), np.int32)
    for k in range(n):
        cy, cx, r = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(8, 31))
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, h), max(cx - r, 0), min(cx + r + 1, w)
        disc = (yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r
        lab[y0:y1, x0:x1][disc] = k + 1
    return lab


def previous_method(ann, kind):
    from scipy import ndimage
    if kind == "binary":
        ann = ndimage.label(ann.astype(bool), structure=np.ones((3, 3), int))[0]
    ids = np.unique(ann)
    masks = [ann == u for u in ids[ids != 0]] if ids.size and ids[0] == 0 else [ann == u for u in ids]
    return [rle.encode(np.asfortranarray(m)) for m in masks], [data_utils.extract_boxes(m)[0] for m in masks]


def bench_input(name, ann, kind, a, ctx, tmp):
    import torch
    from PIL import Image
    one = lambda d: analyze.label_image_to_rle(ann, kind, 2, device=d)
    dev, host, prev = one("cuda"), one("cpu"), previous_method(ann, kind)
    assert dev[0] == host[0] == prev[0] and all(x.tobytes() == y.tobytes() for x, y in zip(dev[1:], host[1:])), "the paths disagree"
    assert np.asarray(prev[1]).reshape(-1, 4).tobytes() == dev[1].tobytes(), "the previous method's boxes disagree"
    def folder(fmt):
        """A dataset folder that holds the one annotation: a PNG of the foreground ('binary') or the ids as .npy ('label')"""
        im_root, ann_root = os.path.join(tmp, name, fmt, "images"), os.path.join(tmp, name, fmt, "annotations")
        os.makedirs(im_root); os.makedirs(ann_root)
        open(os.path.join(im_root, "a.png"), "wb").close()
        if fmt == "binary":
            Image.fromarray((ann != 0).astype(np.uint8) * 255).save(os.path.join(ann_root, "a.png"))
        else:
            np.save(os.path.join(ann_root, "a.npy"), ann)
        return im_root, ann_root

    runs = {"device": (lambda: one("cuda"), a.inner), "host": (lambda: one("cpu"), a.inner), "previous": (lambda: previous_method(ann, kind), 1)}
    for fmt in ("binary", "label") if kind == "label" else ("binary",):
        roots = folder(fmt)
        key = "ddicts" if fmt == "binary" else "ddicts-label"
        cuda, cpu = (data_utils.get_ddicts(fmt, *roots, device=d) for d in ("cuda", "cpu"))
        assert [x["segmentation"] for x in cuda[0]["annotations"]] == [x["segmentation"] for x in cpu[0]["annotations"]], "get_ddicts disagrees"
        runs[key + "-cuda"] = (lambda fmt=fmt, roots=roots: data_utils.get_ddicts(fmt, *roots, device="cuda"), a.inner)
        runs[key + "-cpu"] = (lambda fmt=fmt, roots=roots: data_utils.get_ddicts(fmt, *roots, device="cpu"), a.inner)
    ms = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):
        for key, (fn, inner) in runs.items():
            if key == "previous" and i >= a.ref_reps:                # the checking pass above was its warm-up
                continue
            ctx.sync(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            dt = (time.perf_counter() - t) * 1e3 / inner
            if key == "previous" or i >= a.warmup:
                ms[key].append(dt)
    out = {"image": list(ann.shape), "kind": kind, "instances": len(dev[0]), "counts": int(sum(len(rle._counts(r)) for r in dev[0]))}
    for key, t in ms.items():
        t = np.sort(np.asarray(t))
        out[key] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_label_runs.py measures on a HIP device and none is visible: not measured")
    ctx = analyze._current_device_context("bench_label_runs")
    out = {"metric": "instances of one annotation image as RLE dicts and boxes, ms per image (host clock; every call ends synchronised)",
           "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "ref_reps": a.ref_reps}
    with tempfile.TemporaryDirectory() as tmp:
        out["spheroidite"] = bench_input("spheroidite", spheroidite(), "binary", a, ctx, tmp)
        out["powder"] = bench_input("powder", powder(), "label", a, ctx, tmp)
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        names = {"device": "label_image_to_rle(device='cuda'): upload, launches, download, counts strings",
                 "host": "label_image_to_rle(device='cpu'): run-based union-find on the host",
                 "previous": "the previous method: scipy label, one dense mask, box and encode per instance",
                 "ddicts-cuda": "get_ddicts('binary', device='cuda') end to end on a PNG of the foreground, file read included",
                 "ddicts-cpu": "get_ddicts('binary', device='cpu') end to end, file read included",
                 "ddicts-label-cuda": "get_ddicts('label', device='cuda') end to end on the ids as .npy, file read included",
                 "ddicts-label-cpu": "get_ddicts('label', device='cpu') end to end, file read included"}
        with open(a.md, "w") as f:
            f.write("# Annotation image to instances (tools/bench_label_runs.py)\n\n")
            f.write(f"`python tools/bench_label_runs.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} --ref-reps {a.ref_reps} --md {a.md}`\n\n")
            f.write(f"{a.reps} timed samples after {a.warmup} warm-ups, the evaluations alternating in one process; a sample is the mean of {a.inner} back-to-back "
                    f"calls (the previous method: one call, {a.ref_reps} samples after the checking pass).  Host clock, MI355X.  The three evaluations are "
                    "checked identical, every box and every counts string, before anything is timed.  Speed is recorded, not gated.\n")
            for key in ("spheroidite", "powder"):
                r = out[key]
                f.write(f"\n## {key}: {r['image'][0]} x {r['image'][1]}, kind '{r['kind']}', {r['instances']} instances, {r['counts']} counts\n\n")
                f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
                for k, label in names.items():
                    if k in r:
                        f.write(f"| {label} | {r[k]['median_ms']} | {r[k]['min_ms']} | {r[k]['max_ms']} | {r[k]['samples']} |\n")


if __name__ == "__main__":
    main()
