"""Times the optimizer step alone (R50-FPN, K = 2: 44 M trainable floats) with device events: the plain step (amp_model_sgd_step, which is
also what the general entry runs for options that ask for nothing new), the general kernels with clipping off, and the general kernels
with norm-2 clipping.  Every timed step follows a real backward pass at a small image size (the arenas do not depend on it), as in
training; the modes alternate inside one run so that they see the same machine.  Prints one JSON line.

    python tools/bench_sgd.py [--steps 50] [--warmup 5] [--modes plain,general,norm2]
"""
import argparse
import inspect
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ampis_amd import _lib, params as P, synth
from ampis_amd.model import MaskRCNN

MODES = {
    "plain": {},                                                        # sgd_chunks_kernel
    "general": dict(nesterov=True),                                     # finish + update launches
    "norm2": dict(nesterov=True, clip=("norm", 1.0, 2.0)),              # statistics + finish + update launches
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="plain,general,norm2")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if "nesterov" not in inspect.signature(MaskRCNN.sgd_step).parameters:
        modes = [m for m in modes if m == "plain"]                      # a build without the general step: the reference point only
    K, B, H, W = 2, 2, 192, 256
    ctx = _lib.Context(0)
    model = MaskRCNN(ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), train=True, max_gt=2048, max_poly_doubles=2048 * 64)
    model.load_params(P.init_params(K, seed=0, style="spread"))
    imgs, gts = synth.batch(B, H, W, seed=9)
    gts = [dict(boxes=g["boxes"][:40], classes=g["classes"][:40], polygons=g["polygons"][:40]) for g in gts]
    ms = {m: [] for m in modes}
    for i in range(a.warmup + a.steps):
        for m in modes:
            model.forward_losses(imgs, gts, seed=i, backward=True)
            ctx.sync()
            ctx.timer_start()
            model.sgd_step(1e-6, 0.9, 1e-4, **MODES[m])
            dt = ctx.timer_stop()
            if i >= a.warmup:
                ms[m].append(dt)
    floats = sum(int(np.prod(s)) for k, s in P.param_shapes(K).items() if k in set(model.trainable_names()))
    out = {"metric": "optimizer step alone, R50-FPN K=2, ms per step (device events around one step, after a backward pass)",
           "steps": a.steps, "warmup": a.warmup, "trainable_floats": floats}
    for m in modes:
        t = np.sort(np.asarray(ms[m]))
        out[m] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "p90_ms": round(float(t[int(0.9 * (len(t) - 1))]), 4)}
    if "plain" in out:
        for m in modes:
            if m != "plain":
                out[m]["median_over_plain"] = round(out[m]["median_ms"] / out["plain"]["median_ms"], 3)
    model.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
