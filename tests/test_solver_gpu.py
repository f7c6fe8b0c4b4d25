"""The general SGD step on the device (amp_sgd_step_tensors / amp_model_sgd_step_ex: per-tensor learning rate and weight decay, Nesterov,
value and norm clipping) against the fp32 restatement of tests/test_solver_cfg.py, bit for bit; the fast-path rule; and DefaultTrainer
passing cfg.SOLVER through to it."""
import math

import numpy as np
import pytest

from test_solver_cfg import F, clip_coef, group_scalars, norm64, restate_step

pytestmark = pytest.mark.gpu


def fp32_neighbours(x64):
    """The two float32 values that enclose the fp64 value x64 (equal when x64 is a float32)."""
    n = F(x64)
    if float(n) == x64:
        return n, n
    return (n, np.nextafter(n, F(np.inf))) if float(n) < x64 else (np.nextafter(n, F(-np.inf)), n)


def assert_norm_within_one_ulp(N, g, grad_scale, norm_type, what):
    """N is one of the two fp32 neighbours of the norm numpy accumulates in fp64 from fl32(g * grad_scale): an fp64 sum of <= 1.3e7
    non-negative terms is good to ~1e-9 relative, far inside half an fp32 ulp, so the device and numpy can only disagree on the neighbour."""
    lo, hi = fp32_neighbours(norm64(g, grad_scale, norm_type))
    assert N == lo or N == hi, (what, float(N), float(lo), float(hi))


SIZES = [1, 3, 4, 64, 16384, 16385, 50001, 12845056]      # the last one is roi_heads.box_head.fc1.weight
IS_BIAS = [1, 0, 0, 1, 0, 1, 0, 0]
ZERO_GRAD = 2                                             # this tensor's gradient is all zero in every step


@pytest.fixture(scope="module")
def arena():
    """Three steps of gradients over one arena: tensors 64-float aligned with an extra gap of 4 .. 60 floats behind each (the gaps hold
    sentinels in p / v and noise in g)."""
    off, o = [], 8
    for i, n in enumerate(SIZES):
        off.append(o)
        o = (o + n + 63) // 64 * 64 + 4 * (i % 3)
    total = o + 64
    rng = np.random.default_rng(11)
    p0 = rng.uniform(-0.25, 0.25, total).astype(F)
    G = []
    for step in range(3):
        g = rng.standard_normal(total).astype(F) * F(0.02)
        g[off[ZERO_GRAD]:off[ZERO_GRAD] + SIZES[ZERO_GRAD]] = 0
        G.append(g)
    inside = np.zeros(total, bool)
    for o_, n in zip(off, SIZES):
        inside[o_:o_ + n] = True
    return dict(off=off, total=total, p0=p0, G=G, inside=inside)


def _run_device(gpu_ctx, a, p, v, g, **kw):
    import torch
    from ampis_amd import ops
    pd, vd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(g).cuda()
    norms, coefs = ops.sgd_step_tensors(gpu_ctx, pd, gd, vd, a["off"], SIZES, IS_BIAS, **kw)
    return pd.cpu().numpy(), vd.cpu().numpy(), norms, coefs


def _check_steps(gpu_ctx, a, nesterov, clip, blf, wdb, grad_scale, steps=3, twice=True):
    lr, mu, wd = 0.02, 0.9, 1e-4
    kw = dict(lr=lr, momentum=mu, weight_decay=wd, grad_scale=grad_scale, nesterov=nesterov, bias_lr_factor=blf, weight_decay_bias=wdb, clip=clip)
    p, v = a["p0"].copy(), np.full(a["total"], 0, F)
    v[~a["inside"]] = F(7.5)                     # sentinels in the gaps of the momentum arena
    ks = []
    for step in range(steps):
        g = a["G"][step]
        pd, vd, norms, coefs = _run_device(gpu_ctx, a, p, v, g, **kw)
        if twice and step == 0:                    # (c) the same state again: the same bits
            pd2, vd2, norms2, coefs2 = _run_device(gpu_ctx, a, p, v, g, **kw)
            assert np.array_equal(pd, pd2) and np.array_equal(vd, vd2) and np.array_equal(norms, norms2) and np.array_equal(coefs, coefs2)
        # (d) nothing outside the tensors moved
        assert np.array_equal(pd[~a["inside"]], p[~a["inside"]]) and np.array_equal(vd[~a["inside"]], v[~a["inside"]])
        for t, (o, n) in enumerate(zip(a["off"], SIZES)):
            sl = slice(o, o + n)
            lr_t, wd_t = group_scalars(lr, wd, blf, wdb, IS_BIAS[t])
            N = None
            if clip is not None and clip[0] == "norm":
                N = norms[t]
                assert_norm_within_one_ulp(N, g[sl], grad_scale, clip[2], (step, t))                    # (a)
                assert coefs[t] == clip_coef(N, clip[1]), (step, t, coefs[t], N)
            else:
                assert norms[t] == 0 and coefs[t] == 1
            pe, ve, _, k = restate_step(p[sl], v[sl], g[sl], lr_t, wd_t, mu, grad_scale, nesterov, clip, N=N)     # (b) with the device's N
            bad_p, bad_v = int((pe != pd[sl]).sum()), int((ve != vd[sl]).sum())
            assert bad_p == 0 and bad_v == 0, f"step {step} tensor {t} ({n} floats): {bad_p} parameters, {bad_v} momenta differ from the restatement"
            ks.append((t, float(k)))
        p, v = pd, vd
    # the all-zero gradient: k == 1, and the parameter still took the decay (a bias-free tensor with wd > 0)
    z = slice(a["off"][ZERO_GRAD], a["off"][ZERO_GRAD] + SIZES[ZERO_GRAD])
    assert all(k == 1.0 for t, k in ks if t == ZERO_GRAD)
    assert not np.array_equal(p[z], a["p0"][z])
    return ks


CLIPS = [None, ("value", 0.01), ("norm", 30.0, 1.0), ("norm", 0.5, 2.0), ("norm", 0.03, float("inf"))]


@pytest.mark.parametrize("groups", [(1.0, None, 1.0), (2.0, 0.0, 0.5)], ids=["one-group", "bias-lr2-wd0-scale0.5"])
@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: "none" if c is None else "-".join(str(x) for x in c))
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_step_tensors_matches_the_restatement_bitwise(gpu_ctx, arena, nesterov, clip, groups):
    """3 steps over tensors of 1 .. 12 845 056 floats: (a) every reported norm within one ulp of the fp64 norm, (b) with that norm
    substituted, parameters and momentum equal the numpy restatement bit for bit after every step, (c) a second run from the same state
    gives the same bits, (d) the alignment gaps are untouched.  The norm thresholds are chosen so that small tensors pass (k == 1) and
    large ones clip (k < 1)."""
    blf, wdb, gscale = groups
    ks = _check_steps(gpu_ctx, arena, nesterov, clip, blf, wdb, gscale)
    if clip is not None and clip[0] == "norm":
        assert any(k < 1.0 for _, k in ks) and any(k == 1.0 for t, k in ks if t != ZERO_GRAD), sorted(set(ks))


def test_step_tensors_every_tensor_clipped_and_none_clipped(gpu_ctx, arena):
    sub = dict(arena)
    sub["G"] = [g.copy() for g in arena["G"][:1]]
    z = slice(arena["off"][ZERO_GRAD], arena["off"][ZERO_GRAD] + SIZES[ZERO_GRAD])
    sub["G"][0][z] = F(0.01)                      # no zero gradient here, so that every tensor can clip
    lr, mu, wd = 0.02, 0.9, 1e-4
    for c, want in ((1e-4, lambda k: k < 1.0), (1e6, lambda k: k == 1.0)):
        kw = dict(lr=lr, momentum=mu, weight_decay=wd, nesterov=True, clip=("norm", c, 2.0))
        p, v = sub["p0"].copy(), np.zeros(sub["total"], F)
        pd, vd, norms, coefs = _run_device(gpu_ctx, sub, p, v, sub["G"][0], **kw)
        assert all(want(k) for k in coefs), coefs
        for t, (o, n) in enumerate(zip(sub["off"], SIZES)):
            sl = slice(o, o + n)
            pe, ve, _, k = restate_step(p[sl], v[sl], sub["G"][0][sl], F(lr), F(wd), mu, 1.0, True, ("norm", c, 2.0), N=norms[t])
            assert k == coefs[t] and np.array_equal(pe, pd[sl]) and np.array_equal(ve, vd[sl]), t


def test_step_tensors_refuses_bad_options_naming_the_field(gpu_ctx):
    import torch
    from ampis_amd import _lib, ops
    p, g, v = (torch.zeros(64, device="cuda") for _ in range(3))
    call = lambda **kw: ops.sgd_step_tensors(gpu_ctx, p, g, v, [0], [64], [0], 0.01, **kw)
    for kw, field in ((dict(clip=("norm", 1.0, 3.0)), "norm_type"), (dict(clip=("norm", 0.0, 2.0)), "clip_value"), (dict(clip=("value", -1.0)), "clip_value"),
                      (dict(momentum=float("nan")), "momentum"), (dict(bias_lr_factor=float("inf")), "bias_lr_factor"),
                      (dict(clip=("norm", 1.0, -float("inf"))), "norm_type")):
        with pytest.raises(_lib.AmpError, match=field):
            call(**kw)
    with pytest.raises(_lib.AmpError, match="multiple of 4"):
        ops.sgd_step_tensors(gpu_ctx, p, g, v, [2], [8], [0], 0.01)
    assert float(p.abs().max()) == 0.0


K_, B_, H_, W_ = 2, 2, 192, 256


def _model_and_batch(gpu_ctx):
    from ampis_amd import params as P, synth
    from ampis_amd.model import MaskRCNN
    imgs, gts = synth.batch(B_, H_, W_, seed=9)
    gts = [dict(boxes=g["boxes"][:40], classes=g["classes"][:40], polygons=g["polygons"][:40]) for g in gts]
    npp = P.init_params(K_, seed=2, style="spread")
    m = MaskRCNN(gpu_ctx, K_, max_batch=B_, max_h=H_, max_w=W_, max_out_hw=max(H_, W_), train=True, max_gt=2048, max_poly_doubles=2048 * 64)
    m.load_params(npp)
    return m, imgs, gts, npp


def test_default_options_take_the_existing_kernel_bit_for_bit(gpu_ctx):
    """amp_model_sgd_step_ex with options that ask for nothing new runs sgd_chunks_kernel (amp_debug_last_sgd_path == 1) and leaves
    parameters and momentum bitwise equal to amp_model_sgd_step from the same state; any new option takes the general kernels (== 2)."""
    import ctypes as C
    from ampis_amd import _lib
    L = _lib.lib()
    lr, mu, wd = 0.01, 0.9, 1e-4
    out = []
    for which in ("positional", "ex-default"):
        m, imgs, gts, npp = _model_and_batch(gpu_ctx)
        assert L.amp_debug_last_sgd_path(m._h) == 0
        for seed in (3, 4):                        # the second step exercises mu * v
            m.forward_losses(imgs, gts, seed=seed, backward=True)
            if which == "positional":
                m.sgd_step(lr, mu, wd)
            else:
                o = _lib.sgd_opts(lr, mu, wd)
                _lib.check(L.amp_model_sgd_step_ex(m._h, C.byref(o)), "amp_model_sgd_step_ex")
            assert L.amp_debug_last_sgd_path(m._h) == 1
        names = m.trainable_names()
        out.append(({k: m.get_tensor(k) for k in names}, {k: m.get_tensor(k, momentum=True) for k in names}))
        if which == "ex-default":
            # weight_decay_bias spelled out but equal, bias factor 1, clipping off: still the existing kernel; each new option: the general ones
            for kw, path in ((dict(weight_decay_bias=wd), 1), (dict(nesterov=True), 2), (dict(bias_lr_factor=2.0), 2), (dict(weight_decay_bias=0.0), 2),
                             (dict(clip=("value", 1.0)), 2), (dict(clip=("norm", 1.0, 2.0)), 2)):
                m.forward_losses(imgs, gts, seed=5, backward=True)
                m.sgd_step(lr, mu, wd, grad_scale=1.0, **kw)
                assert L.amp_debug_last_sgd_path(m._h) == path, kw
        m.close()
    (pa, va), (pb, vb) = out
    for k in pa:
        assert np.array_equal(pa[k], pb[k]) and np.array_equal(va[k], vb[k]), k
        assert np.abs(va[k]).max() > 0, k


def test_model_step_with_every_option_matches_the_restatement_bitwise(gpu_ctx):
    """Small R50, K = 2, 192 x 256: norm clipping at the median of the tensors' norms (so that some clip and some do not), Nesterov,
    bias_lr_factor 2, weight_decay_bias 0, grad_scale 0.5.  Every trainable tensor and its momentum against the restatement fed the
    norms clip_stats() reports, bit for bit, those norms within one ulp of the fp64 norm of the gradients read back; two steps."""
    m, imgs, gts, npp = _model_and_batch(gpu_ctx)
    names = m.trainable_names()
    lr, mu, wd, blf, wdb, gscale = 0.01, 0.9, 1e-4, 2.0, 0.0, 0.5
    p = {k: m.get_tensor(k) for k in names}
    v = {k: np.zeros_like(p[k]) for k in names}
    for step, seed in enumerate((3, 4)):
        m.forward_losses(imgs, gts, seed=seed, backward=True)
        g = {k: m.get_tensor(k, grad=True) for k in names}
        norms = np.array([norm64(g[k], gscale, 2.0) for k in names])
        c = float(np.median(norms))
        clip = ("norm", c, 2.0)
        m.sgd_step(lr, mu, wd, grad_scale=gscale, nesterov=True, bias_lr_factor=blf, weight_decay_bias=wdb, clip=clip)
        stats = m.clip_stats()
        assert list(stats) == names
        ks = []
        for k in names:
            N, coef = stats[k]
            assert_norm_within_one_ulp(N, g[k], gscale, 2.0, (step, k))
            assert coef == clip_coef(N, c), (step, k)
            lr_t, wd_t = group_scalars(lr, wd, blf, wdb, k.endswith(".bias"))
            pe, ve, _, _ = restate_step(p[k], v[k], g[k], lr_t, wd_t, mu, gscale, True, clip, N=N)
            got_p, got_v = m.get_tensor(k), m.get_tensor(k, momentum=True)
            assert np.array_equal(pe, got_p) and np.array_equal(ve, got_v), \
                f"step {step} {k}: {int((pe != got_p).sum())} parameters, {int((ve != got_v).sum())} momenta of {pe.size} differ"
            p[k], v[k] = got_p, got_v
            ks.append(float(coef))
        assert sum(k < 1.0 for k in ks) >= len(ks) // 4 and sum(k == 1.0 for k in ks) >= len(ks) // 4, sorted(ks)
    for k in ("backbone.bottom_up.stem.conv1.weight", "backbone.bottom_up.res2.0.conv1.weight", "backbone.bottom_up.res2.2.conv3.weight"):
        assert np.array_equal(m.get_tensor(k), npp[k]), k
    m.close()


def test_x101_grouped_weights_clip_as_their_state_dict_tensors(gpu_ctx):
    """X-101-32x8d stores a grouped 3x3 weight as block-diagonal windows (structural zeros) and fuses the predictors; the statistics are
    those of the state_dict tensors all the same: norms within one ulp of the gradients read back in torch layout, every tensor and its
    momentum bit for bit against the restatement."""
    from ampis_amd import params as P, synth
    from ampis_amd.model import MaskRCNN
    K, B, H, W = 2, 1, 128, 160
    imgs, gts = synth.batch(B, H, W, seed=31)
    gts = [dict(boxes=g["boxes"][:25], classes=g["classes"][:25], polygons=g["polygons"][:25]) for g in gts]
    m = MaskRCNN(gpu_ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), arch="X101", train=True, max_gt=512, max_poly_doubles=512 * 64)
    m.load_params(P.init_params(K, seed=4, style="spread", arch="X101"))
    names = m.trainable_names()
    assert sum(n.endswith(".conv2.weight") for n in names) == 4 + 23 + 3
    lr, mu, wd = 0.01, 0.9, 1e-4
    p = {k: m.get_tensor(k) for k in names}
    m.forward_losses(imgs, gts, seed=3, backward=True)
    g = {k: m.get_tensor(k, grad=True) for k in names}
    c = float(np.median([norm64(g[k], 1.0, 2.0) for k in names]))
    clip = ("norm", c, 2.0)
    m.sgd_step(lr, mu, wd, nesterov=True, clip=clip)
    stats = m.clip_stats()
    assert list(stats) == names
    for k in names:
        N, coef = stats[k]
        assert_norm_within_one_ulp(N, g[k], 1.0, 2.0, k)
        pe, ve, _, kk = restate_step(p[k], np.zeros_like(p[k]), g[k], F(lr), F(wd), mu, 1.0, True, clip, N=N)
        assert kk == coef and np.array_equal(pe, m.get_tensor(k)) and np.array_equal(ve, m.get_tensor(k, momentum=True)), k
    m.close()


def _ddicts(n, h, w, seed):
    from ampis_amd import synth
    out = []
    for i in range(n):
        img, gt = synth.micrograph(i, h, w, seed=seed)
        annos = [{"bbox": b.tolist(), "bbox_mode": 0, "segmentation": [p.tolist()], "category_id": 0}
                 for b, p in list(zip(gt["boxes"], gt["polygons"]))[:50]]
        out.append({"file_name": f"synthetic_{i}.png", "image_bgr": img, "height": h, "width": w, "image_id": i, "annotations": annos,
                    "mask_format": "polygonmask", "num_instances": len(annos)})
    return out


NEW_KEYS = ("NESTEROV", "BIAS_LR_FACTOR", "WEIGHT_DECAY_BIAS", "LR_SCHEDULER_NAME", "WARMUP_METHOD", "CLIP_GRADIENTS")


def _train(tmp_path, tag, monkeypatch, edit):
    """4 iterations of DefaultTrainer on a registered synthetic dataset; returns (recorded sgd_step calls, losses, final weights, trainer lr_at, cfg)."""
    from ampis_amd import checkpoint, model_zoo, params as P
    from ampis_amd.config import get_cfg
    from ampis_amd.data import DatasetCatalog, MetadataCatalog
    from ampis_amd.engine import DefaultTrainer
    from ampis_amd.model import MaskRCNN
    DatasetCatalog.clear()
    train = _ddicts(4, 192, 256, 50)
    DatasetCatalog.register("particle_Train", lambda: train)
    MetadataCatalog.get("particle_Train").set(thing_classes=["particle"])
    cfg = get_cfg()
    cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_3x.yaml"))
    cfg.DATASETS.TRAIN, cfg.DATASETS.TEST = ("particle_Train",), ("particle_Train",)
    cfg.SOLVER.IMS_PER_BATCH, cfg.SOLVER.MAX_ITER, cfg.SOLVER.CHECKPOINT_PERIOD = 2, 4, 100
    cfg.SOLVER.BASE_LR, cfg.SOLVER.WARMUP_ITERS, cfg.SOLVER.WARMUP_FACTOR = 0.002, 2, 0.1
    cfg.SEED = 7
    cfg.DATALOADER.NUM_WORKERS = 0
    init = tmp_path / "init.pth"
    if not init.exists():
        checkpoint.save_checkpoint(init, P.init_params(1, seed=4, style="spread"))
    cfg.MODEL.WEIGHTS, cfg.MODEL.ROI_HEADS.NUM_CLASSES = str(init), 1
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (192,), 256
    cfg.OUTPUT_DIR = str(tmp_path / tag)
    edit(cfg)
    calls = []
    orig = MaskRCNN.sgd_step

    def recording(self, *a, **kw):
        calls.append((a, dict(kw)))
        return orig(self, *a, **kw)

    monkeypatch.setattr(MaskRCNN, "sgd_step", recording)
    trainer = DefaultTrainer(cfg)
    trainer.resume_or_load(resume=False)
    trainer.train()
    monkeypatch.setattr(MaskRCNN, "sgd_step", orig)
    losses = [val for val, _ in trainer.storage.history("total_loss")]
    weights = trainer._net.state_dict()
    lrs = [trainer.lr_at(it) for it in range(4)]
    trainer.close()
    DatasetCatalog.clear()
    return calls, losses, weights, lrs, cfg


def test_trainer_passes_the_solver_settings_to_every_step(tmp_path, monkeypatch):
    from ampis_amd.engine.defaults import solver_kwargs

    def solver(clip_on):
        def edit(cfg):
            s = cfg.SOLVER
            s.LR_SCHEDULER_NAME, s.WARMUP_METHOD = "WarmupCosineLR", "constant"
            s.NESTEROV, s.BIAS_LR_FACTOR, s.WEIGHT_DECAY_BIAS = True, 2.0, 0.0
            s.CLIP_GRADIENTS.ENABLED, s.CLIP_GRADIENTS.CLIP_TYPE, s.CLIP_GRADIENTS.CLIP_VALUE = clip_on, "norm", 0.05
        return edit

    calls, losses, w_clip, lrs, cfg = _train(tmp_path, "clip", monkeypatch, solver(True))
    want = solver_kwargs(cfg)
    assert want == dict(nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip=("norm", 0.05, 2.0))
    assert len(calls) == 4 and len(losses) == 4 and all(np.isfinite(losses))
    s = cfg.SOLVER
    for it, (a, kw) in enumerate(calls):
        cosine = 0.5 * (1.0 + math.cos(math.pi * it / 4))
        assert a[0] == lrs[it] == pytest.approx(s.BASE_LR * (0.1 if it < 2 else 1.0) * cosine, rel=1e-14)
        assert a[1:] == (s.MOMENTUM, s.WEIGHT_DECAY) and kw.pop("grad_scale") == 1.0
        assert kw == want, (it, kw)
    # clipping off, everything else the same: other weights
    calls2, losses2, w_noclip, _, cfg2 = _train(tmp_path, "noclip", monkeypatch, solver(False))
    assert all(kw["clip"] is None for _, kw in calls2) and all(np.isfinite(losses2))
    assert any(not np.array_equal(w_clip[k], w_noclip[k]) for k in w_clip)


def test_trainer_default_cfg_equals_a_cfg_without_the_new_keys(tmp_path, monkeypatch):
    def strip(cfg):
        for k in NEW_KEYS:
            del cfg.SOLVER[k]

    calls_a, losses_a, w_a, lrs_a, _ = _train(tmp_path, "default", monkeypatch, lambda cfg: None)
    calls_b, losses_b, w_b, lrs_b, cfg_b = _train(tmp_path, "stripped", monkeypatch, strip)
    assert not any(k in cfg_b.SOLVER for k in NEW_KEYS)
    assert calls_a == calls_b and lrs_a == lrs_b and losses_a == losses_b
    assert all(kw == dict(grad_scale=1.0, nesterov=False, bias_lr_factor=1.0, weight_decay_bias=None, clip=None) for _, kw in calls_a)
    for k in w_a:
        assert np.array_equal(w_a[k], w_b[k]), k
