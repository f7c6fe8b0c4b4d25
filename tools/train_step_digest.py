"""Bit-level digest of training steps over the paths a step can take (csrc/train_plan.h): one JSON record per configuration.

python tools/train_step_digest.py [--only a,b,...] [--out FILE]

A record holds the five losses as bit patterns (forward-only and with backward), sha256 of the gradient arena after forward_backward, sha256 of
every parameter read through get_tensor after one sgd_step and after a second step, workspace_bytes, amp_debug_last_backward_chain,
amp_debug_last_rpn_sparse, N (foreground RoIs), and -- where the library has amp_debug_train_plan -- the plan of the step.  The forward-only
pass and each forward_backward are run twice; `repeatable` says whether the two runs agree in every bit.  Two trees whose records are equal take
the same decisions and compute the same bits; run it on both and compare the files (the `plan` field is the newer tree's alone).

Synthetic micrographs (ampis_amd.synth), weights from a fixed seed.  Switches with an amp_debug_set_* entry are set in this process; the
environment-only ones run in a child process each, one at a time (the switches are read once per process).  A child that ends with a
fault, an abort or its time limit ends the tool at once, with that status."""
import argparse
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 2
SMALL = dict(arch="R50", mode="f16x3", B=2, H=256, W=320, roi_batch=512, gt="first40")
BIG = dict(arch="R50", mode="f16x3", B=4, H=1024, W=1024, roi_batch=512, gt="all")      # p2: 4 * 256 * 256 = 262 144 rows >= 200 000
X = dict(SMALL, arch="X101")
CONFIGS = {
    "a_small": SMALL,
    "b_big": BIG,
    "c_small_f32": dict(SMALL, mode="f32"),
    "d_x101": X,
    "d_x101_gx0": dict(X, set=dict(gx=0)),
    "e_big_rpn_sparse0": dict(BIG, set=dict(rpn_sparse=0)),
    "e_big_rpn_train_fuse0": dict(BIG, set=dict(rpn_train_fuse=0)),
    "e_big_mask_tail_split0": dict(BIG, set=dict(mask_tail_split=0)),
    "e_big_split_chain0": dict(BIG, set=dict(split_chain=0)),
    "f_small_one_image_without_gt": dict(SMALL, gt="second_empty"),
    "f_small_no_gt": dict(SMALL, gt="none"),
    "f_small_bitmask": dict(SMALL, gt="bitmask"),
    "g_big_AMP_NO_SPLIT_GRADS": dict(BIG, env=dict(AMP_NO_SPLIT_GRADS="1")),
    "g_big_AMP_NO_DGRAD_BATCH": dict(BIG, env=dict(AMP_NO_DGRAD_BATCH="1")),
    "g_big_AMP_ASYNC_REDUCE_0": dict(BIG, env=dict(AMP_ASYNC_REDUCE="0")),
    "g_big_AMP_NO_FUSED_BIAS": dict(BIG, env=dict(AMP_NO_FUSED_BIAS="1")),
    "g_big_AMP_NO_DY_CONVERT": dict(BIG, env=dict(AMP_NO_DY_CONVERT="1")),
    "g_big_AMP_NO_DY_REUSE": dict(BIG, env=dict(AMP_NO_DY_REUSE="1")),
    "g_big_AMP_NO_DECONV_SPLIT": dict(BIG, env=dict(AMP_NO_DECONV_SPLIT="1")),
    "g_big_AMP_NO_RPN_SPLIT": dict(BIG, env=dict(AMP_NO_RPN_SPLIT="1"), set=dict(rpn_sparse=0, rpn_train_fuse=0)),      # (the rule sits in the dense pass)
    "g_x101_AMP_GX_DY_INKERNEL": dict(X, env=dict(AMP_GX_DY_INKERNEL="1")),
    "g_small_AMP_NO_TRAIN_NATIVE": dict(SMALL, env=dict(AMP_NO_TRAIN_NATIVE="1")),
}
CHILD_TIMEOUT = 240      # seconds; a configuration takes 10 - 40


def ground_truth(cfg):
    from ampis_amd import rle, synth
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    imgs, gts = synth.batch(B, H, W, seed=77)
    keep = None if cfg["gt"] == "all" else 40
    gts = [dict(boxes=g["boxes"][:keep], classes=g["classes"][:keep], polygons=g["polygons"][:keep]) for g in gts]
    empty = dict(boxes=np.zeros((0, 4), np.float32), classes=np.zeros(0, np.int64), polygons=[])
    if cfg["gt"] == "second_empty":
        gts[1] = empty
    elif cfg["gt"] == "none":
        gts = [empty for _ in gts]
    elif cfg["gt"] == "bitmask":      # every instance as the run lengths of a disc inside its box, no polygon
        yy, xx = np.mgrid[0:H, 0:W]
        for g in gts:
            discs = [((xx - (x0 + x1) / 2) ** 2 + (yy - (y0 + y1) / 2) ** 2 <= (min(x1 - x0, y1 - y0) / 2) ** 2) for x0, y0, x1, y1 in g["boxes"]]
            g["masks_rle"] = [rle.encode(d) for d in discs]
            g["polygons"] = [None] * len(discs)
    return imgs, gts


def bits(losses, names):
    return [struct.unpack("<I", struct.pack("<f", losses[n]))[0] for n in names]


def tap_info(L, m, name):
    ptr, dt, nd, shape = C.c_void_p(), C.c_int(), C.c_int(), (C.c_longlong * 5)()
    if L.amp_model_get_tap(m._h, name.encode(), C.byref(ptr), C.byref(dt), C.byref(nd), shape) != 0:
        return None, ()
    return dt.value, tuple(int(shape[i]) for i in range(nd.value))


def plan_of(L, m, cfg, stale, N):
    """The step's plan as amp_debug_train_plan gives it for what this tool knows of the step (the taps tell the trunk's format)."""
    if not hasattr(L, "amp_debug_train_plan"):
        return None
    f16x3 = 1 if cfg["mode"] == "f16x3" else 0
    acts_split = int(tap_info(L, m, "p2")[0] == 5)
    x = cfg["arch"] == "X101"
    ld = 16
    inputs = [1, 0, f16x3, int(stale), 256, ld, ld, 256, 0, 256, 256, 3, 3, acts_split, int(acts_split and not x), 32 if x else 1, 0 if x else 1, ld, 1,
              N, (K + 3) // 4 * 4, 1, 1, 1] + [0] * 12
    out = (C.c_int * 21)()
    assert L.amp_debug_train_plan((C.c_int * 36)(*inputs), None, out) == 0
    names = "refresh_fwd dgrad_batch sr_ok rpn_train_fused HS AS GSW GS GX last_chain SR async_on MS MT DS".split()
    return dict(zip(names, list(out)[:15]))


def run_config(name):
    from ampis_amd import _lib, params as P
    from ampis_amd.model import MaskRCNN
    cfg = CONFIGS[name]
    L = _lib.lib()
    imgs, gts = ground_truth(cfg)
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    ctx = _lib.Context(0)
    ctx.conv_mode = cfg["mode"]
    m = MaskRCNN(ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), train=True, arch=cfg["arch"], roi_batch=cfg["roi_batch"],
                 max_gt=4096, max_poly_doubles=4096 * 64)
    m.load_params(P.init_params(K, seed=11, style="spread", arch=cfg["arch"]))
    names = m.LOSS_NAMES
    gp, gn = m.grad_arena()

    def grads():
        a = np.empty(gn, np.float32)
        ctx.sync()
        ctx.d2h(a, gp)
        return hashlib.sha256(a.tobytes()).hexdigest()

    def params():
        h = hashlib.sha256()
        for k in m.tensor_names():
            if ".norm." not in k:      # (FrozenBN statistics never change)
                h.update(m.get_tensor(k).tobytes())
        return h.hexdigest()

    for k, v in cfg.get("set", {}).items():
        getattr(L, "amp_debug_set_" + k)(v)
    rec = dict(config=name, workspace_bytes=int(m.workspace_bytes))
    try:
        f1, f2 = (bits(m.forward_losses(imgs, gts, seed=5), names) for _ in range(2))
        rec["losses_forward"] = f1
        steps, same = [], f1 == f2
        for step in range(2):
            r = []
            for _ in range(2):
                lo = bits(m.forward_losses(imgs, gts, seed=5 + step, backward=True), names)
                r.append(dict(losses=lo, grads=grads(), chain=L.amp_debug_last_backward_chain(m._h), rpn_sparse=L.amp_debug_last_rpn_sparse(m._h)))
            same = same and r[0] == r[1]
            N = tap_info(L, m, "train_mask_logits")[1]
            r[0]["N"] = int(N[0]) if N else 0
            plan = plan_of(L, m, cfg, step > 0, r[0]["N"])
            if plan is not None:
                r[0]["plan"] = plan
                r[0]["plan_agrees"] = plan["last_chain"] == r[0]["chain"] and plan["SR"] == r[0]["rpn_sparse"]
            m.sgd_step(0.01)
            r[0]["params_after_sgd"] = params()
            steps.append(r[0])
        rec["steps"], rec["repeatable"], rec["f32_reruns"] = steps, same, m.f32_reruns
    finally:
        for k in cfg.get("set", {}):
            getattr(L, "amp_debug_set_" + k)(-1)
        m.close()
        ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="comma-separated configuration names or their first letters (a, b, ...)")
    ap.add_argument("--out", default=None, help="append the records to this file as well")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RECORD " + json.dumps(run_config(a.child), sort_keys=True), flush=True)
        return 0
    want = [w for w in a.only.split(",") if w]
    todo = [n for n in CONFIGS if not want or n in want or n.split("_")[0] in want]
    for name in todo:
        if CONFIGS[name].get("env"):      # a fresh process: the library reads its switches once
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=dict(os.environ, **CONFIGS[name]["env"]),
                                   capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                print(f"{name}: the child ran into its time limit of {CHILD_TIMEOUT} s; stopping", flush=True)
                return 124
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RECORD ")]
            if p.returncode != 0 or not line:
                print(f"{name}: the child ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                return p.returncode if p.returncode > 0 else 128 - p.returncode if p.returncode < 0 else 1
            rec = json.loads(line[0][7:])
        else:
            rec = run_config(name)
        text = json.dumps(rec, sort_keys=True)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
