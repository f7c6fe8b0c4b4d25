"""CPU tests of the optimizer and schedule settings: the fp32 restatement of the general SGD step (include/ampis_hip.h amp_sgd_opts) held
to torch.optim.SGD + torch.nn.utils.clip_grad_*, cfg.SOLVER -> MaskRCNN.sgd_step keyword arguments (engine/defaults.py solver_kwargs),
the warm-up / cosine schedules, and the ctypes mirror of amp_sgd_opts.  The restatement (`restate_step`) is also what the GPU tests
(tests/test_solver_gpu.py) compare the kernels with, bit for bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def norm64(g, grad_scale, norm_type):
    """The norm of gs = fl32(g * grad_scale) accumulated in fp64 (not yet narrowed): sqrt(sum gs^2), sum |gs| or max |gs|."""
    gs = np.abs((np.asarray(g, F).ravel() * F(grad_scale)).astype(F)).astype(np.float64)
    if norm_type == 2:
        return math.sqrt(float(np.sum(gs * gs)))
    if norm_type == 1:
        return float(np.sum(gs))
    assert math.isinf(norm_type)
    return float(gs.max())


def clip_coef(N, c):
    """k = min(fl32(c / fl32(N + 1e-6f)), 1)"""
    k = F(c) / (F(N) + F(1e-6))
    return F(min(k, F(1.0)))


def restate_step(p, v, g, lr_t, wd_t, mu, grad_scale=1.0, nesterov=False, clip=None, N=None):
    """One step of the formula on one tensor, every operation a separately rounded fp32 operation (numpy float32 arrays do not contract).
    lr_t / wd_t are the tensor's own (already narrowed) learning rate and decay; clip = None | ("value", c) | ("norm", c, norm_type);
    N: the fp32 norm to use for ("norm", ...) (default: the fp64 restatement narrowed).  Returns (p, v, N, k)."""
    p, v, g = np.asarray(p, F), np.asarray(v, F), np.asarray(g, F)
    lr_t, wd_t, mu = F(lr_t), F(wd_t), F(mu)
    gs = g * F(grad_scale)
    k = F(1.0)
    if clip is None:
        gc = gs
    elif clip[0] == "value":
        c = F(clip[1])
        gc = np.minimum(np.maximum(gs, -c), c)
    else:
        if N is None:
            N = F(norm64(g, grad_scale, clip[2]))
        k = clip_coef(N, clip[1])
        gc = gs * k
    ge = gc + wd_t * p
    v = mu * v + ge
    u = ge + mu * v if nesterov else v
    p = p - lr_t * u
    assert p.dtype == F and v.dtype == F
    return p, v, N, k


def group_scalars(lr, wd, bias_lr_factor, weight_decay_bias, is_bias):
    """(lr_t, wd_t) as the host forms them: the product in double, narrowed once."""
    wdb = wd if weight_decay_bias is None else weight_decay_bias
    return (F(float(F(lr)) * float(F(bias_lr_factor))), F(wdb)) if is_bias else (F(lr), F(wd))


def ulp_distance(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


CLIPS = [None, ("value", 0.01), ("norm", 0.5, 1.0), ("norm", 0.5, 2.0), ("norm", 0.01, float("inf"))]


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: "none" if c is None else "-".join(str(x) for x in c))
def test_restatement_matches_torch_sgd_and_clip(clip, nesterov):
    """3 steps of torch.optim.SGD (two parameter groups: weights, and biases with lr * 2 and weight decay 0) after
    torch.nn.utils.clip_grad_value_ / clip_grad_norm_ per parameter (detectron2's per-parameter clipping), on the CPU, against the
    restatement fed the norm clip_grad_norm_ returned.  Allowed difference: steps * 2^-22 * max|p| absolute -- four half-ulp roundings per
    element and step at parameter magnitude (torch's CPU kernels contract a*b + c into one FMA where the formula rounds twice); derived,
    not measured.  The restatement's own fp64 norm is compared with torch's returned fp32 norm for the record (torch sums in fp32)."""
    import torch
    sizes = [1, 7, 1000, 16385, 2400000]
    is_bias = [True, False, True, False, False]
    lr, mu, wd, blf, wdb, steps = 0.02, 0.9, 1e-4, 2.0, 0.0, 3
    rng = np.random.default_rng(5)
    P0 = [rng.uniform(-0.2, 0.2, n).astype(F) for n in sizes]
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in P0]
    opt = torch.optim.SGD([{"params": [t for t, b in zip(tp, is_bias) if not b]},
                           {"params": [t for t, b in zip(tp, is_bias) if b], "lr": lr * blf, "weight_decay": wdb}],
                          lr=lr, momentum=mu, weight_decay=wd, nesterov=nesterov)
    p = [a.copy() for a in P0]
    v = [np.zeros_like(a) for a in P0]
    worst_ulp = 0
    for step in range(steps):
        G = [(rng.standard_normal(n) * 0.05).astype(F) for n in sizes]
        if step == 1:
            G[1][:] = 0            # an all-zero gradient: k = 1, the decay still applies
        norms = [None] * len(sizes)
        for i, t in enumerate(tp):
            t.grad = torch.from_numpy(G[i].copy())
            if clip is not None and clip[0] == "value":
                torch.nn.utils.clip_grad_value_([t], clip[1])
            elif clip is not None:
                norms[i] = F(torch.nn.utils.clip_grad_norm_([t], clip[1], norm_type=clip[2]).item())
                worst_ulp = max(worst_ulp, ulp_distance(norms[i], F(norm64(G[i], 1.0, clip[2]))))
        opt.step()
        for i in range(len(sizes)):
            lr_t, wd_t = group_scalars(lr, wd, blf, wdb, is_bias[i])
            p[i], v[i], _, _ = restate_step(p[i], v[i], G[i], lr_t, wd_t, mu, 1.0, nesterov, clip, N=norms[i])
            bound = (step + 1) * 2.0 ** -22 * float(np.abs(p[i]).max())
            diff = float(np.abs(p[i].astype(np.float64) - tp[i].detach().numpy().astype(np.float64)).max())
            print(f"step {step} size {sizes[i]}: max |p - torch| = {diff:.3e} (bound {bound:.3e}); torch norm vs fp64 norm: {worst_ulp} ulp so far")
            assert diff <= bound, (step, sizes[i], diff, bound, f"torch's fp32 norm is up to {worst_ulp} ulp from the fp64 norm")


def _cfg():
    from ampis_amd import model_zoo
    from ampis_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_3x.yaml"))
    return cfg


def test_solver_defaults_are_detectron2s_and_map_to_the_plain_step():
    from ampis_amd.engine.defaults import solver_kwargs
    s = _cfg().SOLVER
    assert (s.NESTEROV, s.BIAS_LR_FACTOR, s.WEIGHT_DECAY_BIAS, s.LR_SCHEDULER_NAME, s.WARMUP_METHOD) == (False, 1.0, None, "WarmupMultiStepLR", "linear")
    c = s.CLIP_GRADIENTS
    assert (c.ENABLED, c.CLIP_TYPE, c.CLIP_VALUE, c.NORM_TYPE) == (False, "value", 1.0, 2.0)
    assert solver_kwargs(_cfg()) == dict(nesterov=False, bias_lr_factor=1.0, weight_decay_bias=None, clip=None)


def test_every_solver_key_reaches_sgd_step():
    from ampis_amd.engine.defaults import solver_kwargs
    cfg = _cfg()
    cfg.SOLVER.NESTEROV, cfg.SOLVER.BIAS_LR_FACTOR, cfg.SOLVER.WEIGHT_DECAY_BIAS = True, 2.0, 0.0
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
    assert solver_kwargs(cfg) == dict(nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip=("value", 1.0))
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = "norm", 0.25
    assert solver_kwargs(cfg)["clip"] == ("norm", 0.25, 2.0)
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "NORM"               # detectron2 looks the type up case-insensitively in effect
    for nt, want in ((1, 1.0), (1.0, 1.0), (2, 2.0), ("inf", float("inf")), (float("inf"), float("inf"))):
        cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = nt
        assert solver_kwargs(cfg)["clip"] == ("norm", 0.25, want)
    # clipping switched off: the other CLIP_GRADIENTS keys are not looked at
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED, cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = False, "full_model"
    assert solver_kwargs(cfg)["clip"] is None
    # WEIGHT_DECAY_NORM is accepted and changes nothing (every norm layer is FrozenBN)
    before = solver_kwargs(cfg)
    cfg.SOLVER.WEIGHT_DECAY_NORM = 0.05
    assert solver_kwargs(cfg) == before


def test_cfg_without_the_new_keys_gets_the_defaults():
    from ampis_amd.config import CfgNode
    from ampis_amd.engine.defaults import solver_kwargs
    cfg = CfgNode({"SOLVER": {"BASE_LR": 0.01, "MOMENTUM": 0.9, "WEIGHT_DECAY": 1e-4}})
    assert solver_kwargs(cfg) == dict(nesterov=False, bias_lr_factor=1.0, weight_decay_bias=None, clip=None)
    cfg = CfgNode({"SOLVER": {"WEIGHT_DECAY": 1e-4, "CLIP_GRADIENTS": {"ENABLED": True}}})
    assert solver_kwargs(cfg)["clip"] == ("value", 1.0)


@pytest.mark.parametrize("key,value", [
    ("CLIP_GRADIENTS.CLIP_TYPE", "full_model"), ("CLIP_GRADIENTS.CLIP_TYPE", 2), ("CLIP_GRADIENTS.CLIP_TYPE", None),
    ("CLIP_GRADIENTS.NORM_TYPE", 3.0), ("CLIP_GRADIENTS.NORM_TYPE", 0), ("CLIP_GRADIENTS.NORM_TYPE", "two"), ("CLIP_GRADIENTS.NORM_TYPE", -float("inf")),
    ("CLIP_GRADIENTS.CLIP_VALUE", 0.0), ("CLIP_GRADIENTS.CLIP_VALUE", -1.0), ("CLIP_GRADIENTS.CLIP_VALUE", "1.0"), ("CLIP_GRADIENTS.CLIP_VALUE", float("nan")),
    ("CLIP_GRADIENTS.ENABLED", "yes"),
    ("BIAS_LR_FACTOR", -1.0), ("BIAS_LR_FACTOR", "2"), ("WEIGHT_DECAY_BIAS", "0"), ("WEIGHT_DECAY_BIAS", float("inf")),
    ("NESTEROV", 1), ("NESTEROV", "True"), ("NESTEROV", None),
])
def test_unrepresentable_solver_settings_are_refused_naming_the_key(key, value):
    from ampis_amd.engine.defaults import solver_kwargs
    cfg = _cfg()
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "norm"
    node = cfg.SOLVER
    parts = key.split(".")
    for part in parts[:-1]:
        node = node[part]
    node[parts[-1]] = value
    with pytest.raises(ValueError, match=re.escape(f"SOLVER.{key}")):
        solver_kwargs(cfg)


class _Sched:
    """DefaultTrainer.lr_at without a trainer: the method reads self.cfg only."""

    def __init__(self, cfg):
        self.cfg = cfg

    def lr_at(self, it):
        from ampis_amd.engine.defaults import DefaultTrainer
        return DefaultTrainer.lr_at(self, it)


def test_warmup_factor_and_cosine_schedule_closed_form():
    from ampis_amd.engine.train_loop import warmup_cosine_lr, warmup_factor_at
    base, max_iter, iters, factor = 0.02, 1000, 100, 0.001
    for it in (0, 50, 100, max_iter // 2, max_iter - 1):
        cos = 0.5 * (1.0 + math.cos(math.pi * it / max_iter))
        lin = factor * (1 - it / iters) + it / iters if it < iters else 1.0
        con = factor if it < iters else 1.0
        assert warmup_factor_at(it, "linear", iters, factor) == pytest.approx(lin, rel=1e-15)
        assert warmup_factor_at(it, "constant", iters, factor) == pytest.approx(con, rel=1e-15)
        assert warmup_cosine_lr(it, base, max_iter, iters, factor, "linear") == pytest.approx(base * lin * cos, rel=1e-14)
        assert warmup_cosine_lr(it, base, max_iter, iters, factor, "constant") == pytest.approx(base * con * cos, rel=1e-14)
    assert warmup_factor_at(0, "linear", iters, factor) == factor and warmup_factor_at(iters, "linear", iters, factor) == 1.0
    assert warmup_cosine_lr(0, base, max_iter, 0, factor) == base                      # WARMUP_ITERS = 0: no warm-up at all
    assert warmup_factor_at(0, "constant", 0, factor) == 1.0 and warmup_factor_at(0, "linear", 0, factor) == 1.0
    assert warmup_cosine_lr(max_iter // 2, base, max_iter, iters, factor) == pytest.approx(base / 2, rel=1e-14)
    with pytest.raises(ValueError, match="Unknown warmup method"):
        warmup_factor_at(0, "exp", iters, factor)
    with pytest.raises(ValueError, match="Unknown warmup method"):
        warmup_factor_at(0, "exp", 0, factor)


def test_lr_at_picks_the_schedule_by_name():
    import bisect
    cfg = _cfg()
    s = cfg.SOLVER
    s.BASE_LR, s.MAX_ITER, s.STEPS, s.GAMMA, s.WARMUP_ITERS, s.WARMUP_FACTOR = 0.02, 1000, (600, 800), 0.1, 100, 0.001
    sched = _Sched(cfg)

    def todays(it):          # the expression DefaultTrainer.lr_at evaluated before the schedule became selectable
        w = s.WARMUP_FACTOR * (1 - it / s.WARMUP_ITERS) + it / s.WARMUP_ITERS if it < s.WARMUP_ITERS else 1.0
        return s.BASE_LR * w * s.GAMMA ** bisect.bisect_right(list(s.STEPS), it)

    for it in (0, 1, 50, 99, 100, 599, 600, 799, 800, 999):
        assert sched.lr_at(it) == todays(it), it                                       # exactly, not approximately
    s.WARMUP_METHOD = "constant"
    assert sched.lr_at(10) == s.BASE_LR * s.WARMUP_FACTOR and sched.lr_at(100) == s.BASE_LR
    s.LR_SCHEDULER_NAME = "WarmupCosineLR"
    assert sched.lr_at(10) == pytest.approx(s.BASE_LR * s.WARMUP_FACTOR * 0.5 * (1 + math.cos(math.pi * 10 / 1000)), rel=1e-14)
    assert sched.lr_at(500) == pytest.approx(s.BASE_LR / 2, rel=1e-14)
    s.LR_SCHEDULER_NAME = "WarmupPolyLR"
    with pytest.raises(ValueError, match="Unknown LR scheduler: WarmupPolyLR"):
        sched.lr_at(0)
    s.LR_SCHEDULER_NAME, s.WARMUP_METHOD = "WarmupCosineLR", "exp"
    with pytest.raises(ValueError, match="Unknown warmup method"):
        sched.lr_at(0)
    # a cfg that lacks the new keys schedules as before
    from ampis_amd.config import CfgNode
    old = CfgNode({"SOLVER": {"BASE_LR": 0.02, "MAX_ITER": 1000, "STEPS": (600, 800), "GAMMA": 0.1, "WARMUP_ITERS": 100, "WARMUP_FACTOR": 0.001}})
    assert [_Sched(old).lr_at(it) for it in (0, 50, 700)] == [todays(it) for it in (0, 50, 700)]


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "ampis_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_ctypes_sgd_opts_mirrors_the_header():
    from ampis_amd._lib import SgdOpts
    hdr = _header_struct_fields("amp_sgd_opts")
    assert [n for n, _ in SgdOpts._fields_] == [n for n, _ in hdr]
    assert [t for _, t in SgdOpts._fields_] == [{"int": C.c_int, "float": C.c_float}[t] for _, t in hdr]
    assert C.sizeof(SgdOpts) == 4 * len(hdr) == 40
    assert [getattr(SgdOpts, n).offset for n, _ in SgdOpts._fields_] == [4 * i for i in range(len(hdr))]
    src = open(os.path.join(ROOT, "include", "ampis_hip.h")).read()
    vals = dict(re.findall(r"(AMP_CLIP_[A-Z]+) = (\d)", src))
    from ampis_amd import _lib
    assert (int(vals["AMP_CLIP_NONE"]), int(vals["AMP_CLIP_VALUE"]), int(vals["AMP_CLIP_NORM"])) == (_lib.CLIP_NONE, _lib.CLIP_VALUE, _lib.CLIP_NORM)


def test_sgd_opts_default_and_the_bound_symbols():
    """amp_sgd_opts_default writes every field and nothing past the struct; the header declares every new function _lib.py binds, and the
    library exports it (no device call here)."""
    from ampis_amd import _lib
    pad = 32
    size = C.sizeof(_lib.SgdOpts)
    buf = (C.c_ubyte * (size + pad))(*([0xA5] * (size + pad)))
    o = _lib.SgdOpts.from_buffer(buf)
    _lib.check(_lib.lib().amp_sgd_opts_default(C.byref(o)), "amp_sgd_opts_default")
    assert bytes(buf[size:]) == b"\xa5" * pad
    got = {n: getattr(o, n) for n, _ in _lib.SgdOpts._fields_}
    want = dict(lr=0.0, momentum=F(0.9), weight_decay=F(1e-4), grad_scale=1.0, nesterov=0, bias_lr_factor=1.0, weight_decay_bias=F(1e-4),
                clip_type=0, clip_value=1.0, norm_type=2.0)
    assert got == want
    src = open(os.path.join(ROOT, "include", "ampis_hip.h")).read()
    for name in ("amp_sgd_opts_default", "amp_sgd_step_tensors", "amp_model_sgd_step_ex", "amp_model_clip_stats"):
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), name
        assert name in _lib.lib()._amp_sig and hasattr(_lib.lib(), name), name
    # sgd_opts(): the keyword arguments of MaskRCNN.sgd_step -> the struct
    o = _lib.sgd_opts(0.02, 0.9, 1e-4, 0.5, nesterov=True, bias_lr_factor=2.0, weight_decay_bias=None, clip=("norm", 0.25, float("inf")))
    assert (o.nesterov, o.clip_type, o.clip_value, o.weight_decay_bias, o.grad_scale) == (1, _lib.CLIP_NORM, 0.25, F(1e-4), 0.5) and math.isinf(o.norm_type)
    assert _lib.sgd_opts(0.02, clip=("value", 3.0)).clip_type == _lib.CLIP_VALUE
    with pytest.raises(ValueError):
        _lib.sgd_opts(0.02, clip=("full_model", 1.0))
