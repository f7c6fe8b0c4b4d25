"""Times the powder analysis on the project's own fixture: the five 1024 x 1536 micrographs that 'particle-results' and 'satellite-results' of
tests/golden/rle_pickles.json.gz share (193 - 257 particles and 139 - 150 satellites an image), as a sample of 5 images and, repeated, of 50.
Evaluations alternate inside one process, after a warm-up of each:

  measure-cuda / measure-cpu   ampis_amd.applications.powder.satellite_measurements(device='cuda' / 'cpu') on images without matches: string
                               decoding, ONE amp_rle_overlap_groups call for all images, the matching rule, the summary -- what a user waits for
  measure-pairs                the same summary with the matches made by a restatement of the reference's method (ampis/applications/powder.py:
                               80-83): a Python loop of rle.merge(intersect=True) + rle.area for every satellite against every particle
  call-device / call-host      the bare amp_rle_overlap_groups call on arrays pooled once, with a context (csrc/rle_overlap.hip: upload, one
                               launch, download, stream synchronise -- all in the window) and with a NULL context (csrc/mask_analysis_host.hip)

The three ways are checked to give the same matches, and device and host the same bytes, before anything is timed.  A call-* sample is the mean
over --inner back-to-back calls; the per-pair method takes seconds to minutes and is sampled --pair-reps times (once at 50 images).  Prints one
JSON line; --md PATH also writes the figures as a markdown table.  Needs a HIP device: there is no figure without one.

    python tools/bench_powder.py [--reps 7] [--warmup 2] [--inner 10] [--pair-reps 2] [--md profiles/r11/powder.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from ampis_amd import _lib, rle
from ampis_amd.applications import powder


def sample(n_images):
    """n_images PowderSatelliteImage objects without matches: the five fixture images, repeated"""
    from test_powder import fixture_images
    out = []
    while len(out) < n_images:
        out += fixture_images()
    return out[:n_images]


def per_pair_match(particles, satellites, match_thresh=0.5):
    """The reference's loop (ampis/applications/powder.py:80-94) on the C-ABI codec: one merge and one area per pair"""
    ps, ss = powder._to_rle(particles), powder._to_rle(satellites)
    inter = np.array([[rle.area(rle.merge([s, p], intersect=True)) for p in ps] for s in ss], dtype=np.int64).reshape(len(ss), len(ps))
    return powder._match_from_overlap(inter, np.asarray(rle.area(ss), dtype=np.int64), len(ps), match_thresh)


def measure(psis, how):
    for p in psis:
        p.matches = per_pair_match(p.particles, p.satellites) if how == "pairs" else None
    return powder.satellite_measurements(psis, print_summary=False, output_dict=True, device=how if how != "pairs" else "cpu")


class Call:
    """amp_rle_overlap_groups on arrays pooled once: what is timed is the C call alone."""

    def __init__(self, psis):
        a, b = [powder._to_rle(p.satellites) for p in psis], [powder._to_rle(p.particles) for p in psis]
        self.ng = len(psis)
        self.ap, self.bp = rle._pool([rle._counts(x) for g in a for x in g]), rle._pool([rle._counts(x) for g in b for x in g])
        na, nb = [len(g) for g in a], [len(g) for g in b]
        self.af, self.bf = np.zeros(self.ng + 1, np.int32), np.zeros(self.ng + 1, np.int32)
        self.af[1:], self.bf[1:] = np.cumsum(na), np.cumsum(nb)
        self.gh = np.array([g[0]["size"][0] for g in b], np.int32)
        self.gw = np.array([g[0]["size"][1] for g in b], np.int32)
        self.total = int(np.dot(na, nb))
        self.inter = np.zeros(self.total, np.uint32)
        self.aa, self.ab = np.zeros(int(self.af[-1]), np.uint64), np.zeros(int(self.bf[-1]), np.uint64)
        self.runs = int(len(self.ap[0]) + len(self.bp[0]))

    def __call__(self, ctx):
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.lib().amp_rle_overlap_groups(ctx.handle if ctx is not None else None, *(vp(x) for x in self.ap), *(vp(x) for x in self.bp),
                                                     vp(self.af), vp(self.bf), vp(self.gh), vp(self.gw), self.ng, vp(self.inter), self.total,
                                                     vp(self.aa), vp(self.ab)), "amp_rle_overlap_groups")
        return self.inter.copy(), self.aa.copy(), self.ab.copy()


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a) and list(a) == list(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--pair-reps", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise _lib.AmpError("tools/bench_powder.py measures on a HIP device and none is visible: not measured")
    ctx = _lib.Context(0)
    out = {"metric": "powder satellite analysis of a sample of 1024 x 1536 micrographs, ms per evaluation (host clock around synchronised calls)",
           "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "pair_reps": a.pair_reps, "sizes": {}}
    for n in (5, 50):
        psis = sample(n)
        call = Call(psis)
        dev, host = call(ctx), call(None)
        assert all(d.tobytes() == h.tobytes() for d, h in zip(dev, host)), "device and host paths disagree"
        m_dev, m_cpu = measure(psis, "cuda"), measure(psis, "cpu")
        assert same(m_dev, m_cpu), "satellite_measurements differs between the paths"
        pair_ms = []
        if n == 5:                                                       # the checking pass is the per-pair method's warm-up
            assert same(measure(psis, "pairs"), m_cpu), "the per-pair method disagrees"
        runs = {"measure-cuda": (lambda: measure(psis, "cuda"), 1), "measure-cpu": (lambda: measure(psis, "cpu"), 1),
                "call-device": (lambda: call(ctx), a.inner), "call-host": (lambda: call(None), a.inner)}
        ms = {k: [] for k in runs}
        for i in range(a.warmup + a.reps):
            for name, (fn, inner) in runs.items():
                ctx.sync(); torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(inner):
                    fn()
                ctx.sync()
                if i >= a.warmup:
                    ms[name].append((time.perf_counter() - t) * 1e3 / inner)
        for _ in range(a.pair_reps if n == 5 else 1):
            t = time.perf_counter()
            got = measure(psis, "pairs")
            pair_ms.append((time.perf_counter() - t) * 1e3)
            assert same(got, m_cpu), "the per-pair method disagrees"
        ms["measure-pairs"] = pair_ms
        rec = {"images": n, "satellites": int(call.af[-1]), "particles": int(call.bf[-1]), "pairs": call.total, "runs": call.runs,
               "pairs_with_common_pixels": int((dev[0] > 0).sum()), "matched_satellites": int(m_cpu["n_satellites"])}
        for name, t in ms.items():
            t = np.sort(np.asarray(t))
            rec[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "samples": len(t)}
        out["sizes"][str(n)] = rec
    ctx.close()
    print(json.dumps(out))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        names = {"measure-cuda": "satellite_measurements(device='cuda'), from RLE dicts", "measure-cpu": "satellite_measurements(device='cpu'), from RLE dicts",
                 "measure-pairs": "the reference's method: rle.merge(intersect=True) + rle.area per pair in Python, then the same summary",
                 "call-device": "amp_rle_overlap_groups, context (upload + 1 launch + download)", "call-host": "amp_rle_overlap_groups, NULL context"}
        with open(a.md, "w") as f:
            f.write("# Powder satellite analysis of a sample (tools/bench_powder.py)\n\n")
            f.write(f"The five 1024 x 1536 fixture micrographs (tests/golden/rle_pickles.json.gz, particle-results x satellite-results) as a sample of 5 "
                    f"images and, repeated, of 50; all images of a sample in ONE amp_rle_overlap_groups call.  {a.reps} timed samples after {a.warmup} "
                    f"warm-ups, the evaluations alternating in one process; a bare-call sample is the mean of {a.inner} back-to-back calls, each ending "
                    f"in a stream synchronise; the per-pair method is sampled {a.pair_reps} times at 5 images and once at 50, after its checking pass.  "
                    f"Host clock, MI355X.\n\n")
            for n, rec in out["sizes"].items():
                f.write(f"## {n} images: {rec['satellites']} satellites x {rec['particles']} particles, {rec['pairs']} pairs in {rec['runs']} runs; "
                        f"{rec['pairs_with_common_pixels']} pairs share a pixel, {rec['matched_satellites']} satellites match\n\n")
                f.write("| evaluation | median ms | min ms | max ms | samples |\n|---|---|---|---|---|\n")
                for k in ("measure-cuda", "measure-cpu", "measure-pairs", "call-device", "call-host"):
                    f.write(f"| {names[k]} | {rec[k]['median_ms']} | {rec[k]['min_ms']} | {rec[k]['max_ms']} | {rec[k]['samples']} |\n")
                f.write("\n")
            f.write("The three ways give the same matches and summary, device and host the same bytes (checked before timing).  Speed is recorded, "
                    "not gated; 'auto' means the device when one is visible, whichever is faster at a size.\n")


if __name__ == "__main__":
    main()
