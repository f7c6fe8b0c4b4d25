"""One rank of tests/test_solver_world2_gpu.py: a norm-clipped general SGD step behind the overlapped gradient exchange, two ranks sharing
cuda:0 through the librccl stand-in (see rank_main.py).  Writes a JSON report; the parent test asserts on it."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def main(out_path):
    import torch.distributed as dist
    from ampis_amd import _lib, params as P, synth
    from ampis_amd.model import MaskRCNN
    from ampis_amd.utils import comm

    dist.init_process_group("gloo")
    rank = dist.get_rank()
    rep = {"rank": rank}
    ctx = _lib.Context(0)
    comm.attach_rccl(ctx)
    K, B, H, W = 2, 2, 192, 256
    imgs, gts = synth.batch(B, H, W, seed=9 + rank)                  # different data per rank, the same weights
    gts = [dict(boxes=g["boxes"][:40], classes=g["classes"][:40], polygons=g["polygons"][:40]) for g in gts]
    npp = P.init_params(K, seed=2, style="spread")

    def make(c):
        m = MaskRCNN(c, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), train=True, max_gt=2048, max_poly_doubles=2048 * 64)
        m.load_params(npp)
        return m

    model = make(ctx)
    names = model.trainable_names()
    # the summed gradients of this batch, read after an explicit exchange (no update yet)
    model.set_grad_overlap(False)
    model.forward_losses(imgs, gts, seed=3, backward=True)
    rep["scale"] = scale = comm.all_reduce_gradients(model, ctx)
    ptr, nf = model.grad_arena()
    g_sum = np.empty(nf, dtype=np.float32)
    ctx.comm_wait(); ctx.sync(); ctx.d2h(g_sum, ptr)
    norms = [float(np.sqrt(np.sum((model.get_tensor(k, grad=True).astype(np.float64) * scale) ** 2))) for k in names]
    c = float(np.median(norms))                                      # the same on both ranks: about half of the tensors clip
    step = dict(grad_scale=scale, nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip=("norm", c, 2.0))
    # the same batch with the exchange issued from inside the backward pass; the step follows at once and waits on the device
    model.set_grad_overlap(True)
    model.forward_losses(imgs, gts, seed=3, backward=True)
    rep["exchanged"] = model.grads_exchanged()
    model.sgd_step(0.01, 0.9, 1e-4, **step)
    stats = model.clip_stats()
    rep["clipped"], rep["unclipped"] = sum(1 for n_, k in stats.values() if k < 1), sum(1 for n_, k in stats.values() if k == 1)
    rep["params"] = {k: sha(model.get_tensor(k)) for k in names}
    rep["momentum"] = sha(model.momentum())
    rep["stats"] = sha(np.array([v for v in stats.values()], dtype=np.float32))
    # a single process (a context without a communicator) stepping on those summed gradients with grad_scale = 1 / world
    solo_ctx = _lib.Context(0)
    solo = make(solo_ctx)
    solo.forward_losses(imgs, gts, seed=3, backward=True)
    sptr, snf = solo.grad_arena()
    assert snf == nf
    solo_ctx.sync(); solo_ctx.h2d(sptr, g_sum); solo_ctx.sync()
    solo.sgd_step(0.01, 0.9, 1e-4, **step)
    rep["solo_params"] = {k: sha(solo.get_tensor(k)) for k in names}
    rep["solo_momentum"] = sha(solo.momentum())
    solo.close(); solo_ctx.close()
    ctx.barrier()
    model.close()
    comm.detach_rccl()
    ctx.close()
    dist.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(rep, f)


if __name__ == "__main__":
    main(sys.argv[1])
