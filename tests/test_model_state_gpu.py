"""A used model against a freshly loaded one, across every state change of amp_model (ampis_amd/csrc/model.hip).

The contract: the result of a model call is a function of the current parameters, momentum, options and inputs -- not of the calls that came
before.  The model keeps derived copies of its parameters (the f16x3 split copies and their job tables, the split data-gradient copies, the
folded FrozenBN scale / shift, the two fused predictor matrices, w_absmax, the SGD chunk table and plan) and sticky settings (img_hw, the
loss options, the context's conv mode); a stale copy faults nothing and moves no loss by much.  So every case of tests/model_state_cases.py
is applied to a model M that has already trained, and then M's next call is compared with the same call on F: a new model with the same
constructor arguments on a new context in the same conv mode, loaded with M.state_dict() (plus the FrozenBN tensors M was loaded with),
M.momentum_dict(), M's loss options and image sizes.  Steps and inference are bitwise repeatable, so every comparison is byte equality:
  infer     boxes, scores, classes, RLE counts and sizes (same_bytes of test_range_guard_model_gpu);
  forward   the five losses of forward_losses(backward=False);
  step      the five losses, every trainable tensor's gradient and the whole gradient arena of forward_losses(backward=True); then, after the
            same sgd_step on both, state_dict() and the whole momentum arena (padding rows included).
Each (case, probe) pair is a test of its own: the transition is applied, then the one probe, so every probe meets the state the transition
left and not what an earlier probe made of it.  M is created once per module and size and keeps training from test to test; F and its
context are new for every comparison and closed after it.

Sizes: (a) K = 2, 128 x 160, B = 2 for inference and 1 for training (the constants of test_range_guard_model_gpu) for the whole table;
(b) 448 x 448 with B = 2, the smallest frame at which p2 has the 24576 rows of RPN_FUSE_MIN_PIXELS (2 * 112 * 112 = 25088), for the cases
around sgd_step and forward-only calls: the paths gated on fresh split copies (fused RPN head, split chain, fused res2 tail, stem + pool)
only run there or differ most there.  test_size_b_reaches_the_fused_rpn_head shows that the head really is fused at (b)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import model_state_cases as T
from test_range_guard_model_gpu import same_bytes, step_differences

pytestmark = pytest.mark.gpu

SIZES = {"a": dict(BI=2, BT=1, H=128, W=160), "b": dict(BI=2, BT=2, H=448, W=448)}
D = 40
PROBE_SEED = 7


def read_grad_arena(model):
    """the whole gradient arena of a model, as it stands"""
    p, n = model.grad_arena()
    out = np.empty(n, dtype=np.float32)
    model.ctx.sync()
    model.ctx.d2h(out, p)
    return out


class Rig:
    """M, its context, its batches and the Python-side record of what a fresh model has to be given (FrozenBN tensors, image sizes)"""

    def __init__(self, size, comm=False, K=2, arch="R50", anchors=None):
        from ampis_amd import _lib, params as P, synth
        from ampis_amd.model import MaskRCNN
        self.size, self.K, self.arch = size, K, arch
        for k, v in SIZES[size].items():
            setattr(self, k, v)
        n = max(self.BI, self.BT)
        imgs, gts = synth.batch(n, self.H, self.W, seed=31)
        self.imgs_inf, self.imgs_tr = imgs[:self.BI], imgs[:self.BT]
        self.gts = [dict(boxes=g["boxes"][:25], classes=np.minimum(g["classes"][:25], K - 1), polygons=g["polygons"][:25]) for g in gts[:self.BT]]
        # score_thresh 0: a few steps of training on 25 instances push every foreground score of these random weights below the default
        # 0.05, and a comparison of two empty detection lists shows nothing; this way every image keeps its D best boxes and their masks
        self.kw = dict(max_batch=n, max_h=self.H, max_w=self.W, max_out_hw=max(self.H, self.W), detections_per_image=D, train=True, max_gt=512,
                       max_poly_doubles=512 * 64, arch=arch, score_thresh=0.0, **(anchors or {}))
        self.ctx = _lib.Context(0)
        if comm:
            self.ctx.comm_init(0, 1, _lib.Context.comm_unique_id())
        self.M = MaskRCNN(self.ctx, K, **self.kw)
        self.sizes, self.seed, self.base = None, 100, None
        self.load(P.init_params(K, seed=3, style="spread", arch=arch, num_anchors=self.M.num_anchors))
        self.step()                       # every transition meets a model that has trained
        self.sgd(**T.PLAIN)

    # ---- what the cases call ----
    def load(self, params):
        self.M.load_params(params)
        self.base = params

    def step(self):
        self.seed += 1
        return self.M.forward_losses(self.imgs_tr, self.gts, seed=self.seed, backward=True)

    def sgd(self, lr, momentum=0.9, weight_decay=1e-4, **kw):
        self.M.sgd_step(lr, momentum, weight_decay, **kw)

    def infer(self):
        return self.M.infer(self.imgs_inf)

    def forward(self):
        return self.M.forward_losses(self.imgs_tr, self.gts, seed=self.seed, backward=False)

    def set_sizes(self, sizes):
        self.M.set_image_sizes(sizes)
        self.sizes = sizes

    def current_params(self):
        p = {k: v for k, v in self.base.items() if ".norm." in k}
        p.update(self.M.state_dict())
        return p

    def stem_peak(self, params):
        """the largest value the stem + pool leaves on an AMP_CONV_F32 context (it places the power of two of the "stem" scaling)"""
        F, ctx = self.fresh(mode="f32", params=params)
        try:
            F.infer(self.imgs_inf)
            return float(F.tap("stem_pool").max())
        finally:
            F.close()
            ctx.close()

    # ---- the reference ----
    def fresh(self, mode=None, momentum=False, params=None):
        """F: a new context in the conv mode of M's (or `mode`), a new model with M's constructor arguments, M's parameters, options and sizes"""
        from ampis_amd import _lib
        from ampis_amd.model import MaskRCNN
        ctx = _lib.Context(0)
        ctx.conv_mode = self.ctx.conv_mode if mode is None else mode
        F = MaskRCNN(ctx, self.K, **self.kw)
        F.load_params(self.current_params() if params is None else params)
        if momentum:
            assert F.load_momentum_dict(self.M.momentum_dict()) == []
        F.set_loss_opts(self.M.loss_opts())
        F.set_image_sizes(self.sizes)
        return F, ctx

    def train(self, m):
        losses = m.forward_losses(self.imgs_tr, self.gts, seed=PROBE_SEED, backward=True)
        return losses, {n: m.get_tensor(n, grad=True) for n in m.trainable_names()}

    def close(self):
        self.M.close()
        self.ctx.close()


def probe(rig, which):
    """M's next call against F's, byte for byte"""
    M = rig.M
    F, fctx = rig.fresh(momentum=which == "step")
    n0 = M.f32_reruns
    try:
        if which == "infer":
            got, ref = M.infer(rig.imgs_inf), F.infer(rig.imgs_inf)
            assert all(np.isfinite(o["boxes"]).all() and np.isfinite(o["scores"]).all() for o in ref)
            assert sum(len(o["scores"]) for o in ref) > 0, "no detections: the comparison would be empty"
            assert same_bytes(got, ref), "infer() of the used model differs from a freshly loaded model's"
        elif which == "forward":
            got = M.forward_losses(rig.imgs_tr, rig.gts, seed=PROBE_SEED, backward=False)
            ref = F.forward_losses(rig.imgs_tr, rig.gts, seed=PROBE_SEED, backward=False)
            assert all(np.isfinite(v) for v in ref.values()), ref
            bad = [n for n in ref if np.float32(got[n]).tobytes() != np.float32(ref[n]).tobytes()]
            assert not bad, f"forward-only losses of the used model differ from a freshly loaded model's: {[(n, got[n], ref[n]) for n in bad]}"
        else:
            got, ref = rig.train(M), rig.train(F)
            assert all(np.isfinite(v) for v in ref[0].values()), ref[0]
            assert any(np.abs(g).max() > 0 for g in ref[1].values())
            bad = step_differences(got, ref)
            assert not bad, f"{len(bad)} losses / gradients of the used model's step differ from a freshly loaded model's: {bad[:6]}"
            assert read_grad_arena(M).tobytes() == read_grad_arena(F).tobytes(), "the gradient arenas differ outside the tensors (padding rows)"
            M.sgd_step(**T.PLAIN)
            F.sgd_step(**T.PLAIN)
            a, b = M.state_dict(), F.state_dict()
            bad = [k for k in a if a[k].tobytes() != b[k].tobytes()]
            assert not bad, f"{len(bad)} tensors differ after the same sgd_step: {bad[:6]}"
            assert M.momentum().tobytes() == F.momentum().tobytes(), "the momentum arenas differ after the same sgd_step (padding rows included)"
        # every transition of the table ends in range: both calls ran on the split copies the comparison is about, not on the fp32 re-run
        assert (M.f32_reruns - n0, F.f32_reruns) == (0, 0), "the probe was re-run in fp32"
    finally:
        F.close()
        fctx.close()


@pytest.fixture(scope="module")
def rig_a():
    r = Rig("a")
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig_b():
    r = Rig("b")
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig_comm():
    """M on a context with a communicator of size one, built the way test_comm_gpu.py builds rccl_ctx"""
    r = Rig("a", comm=True)
    yield r
    r.close()


TABLE = [(s, c["name"], p) for s in "ab" for c in T.CASES if s in c["sizes"] for p in T.PROBES]


@pytest.mark.parametrize("size,name,which", TABLE, ids=["-".join(t) for t in TABLE])
def test_used_model_equals_a_fresh_one(request, size, name, which):
    c = T.case(name)
    rig = request.getfixturevalue("rig_comm" if c.get("comm") else "rig_" + size)
    try:
        c["apply"](rig)
        probe(rig, which)
    finally:
        rig.set_sizes(None)               # a case that leaves per-image sizes in force leaves them to its own probe only


def test_size_b_reaches_the_fused_rpn_head(rig_b):
    """at size (b) a training step with fresh split copies runs the RPN head fused on p2: the predictor map differs in bytes from the one of
    the two-convolution form (amp_debug_set_rpn_train_fuse(0)), as test_training_forward_with_the_fused_rpn_head_and_recomputed_hidden_rows
    establishes it"""
    from ampis_amd import _lib
    r = rig_b
    assert r.BT * (r.H // 4) * (r.W // 4) >= 24576 and r.BI * (r.H // 4) * (r.W // 4) >= 24576
    r.infer()                             # fresh split copies
    taps = {}
    try:
        for fuse in (0, -1):
            _lib.lib().amp_debug_set_rpn_train_fuse(fuse)
            r.M.forward_losses(r.imgs_tr, r.gts, seed=PROBE_SEED, backward=True)
            taps[fuse] = r.M.tap("rpn_pred2")
    finally:
        _lib.lib().amp_debug_set_rpn_train_fuse(-1)
    assert taps[0].shape == taps[-1].shape and np.isfinite(taps[0]).all()
    assert taps[0].tobytes() != taps[-1].tobytes(), "p2 did not take the fused RPN head at size (b)"


# ---- state_dict() is the inverse of load_params() ----------------------------------------------------------------------------------------------
A9 = dict(anchor_sizes=[[32, 40, 50], [64, 80, 101], [128, 161, 203], [256, 322, 406], [512, 645, 812]], aspect_ratios=[[0.5, 1.0, 2.0]])
ROUND_TRIP = {"R50-K1": ("R50", 1, {}), "R50-K2": ("R50", 2, {}), "R50-K3": ("R50", 3, {}), "R50-K2-A9": ("R50", 2, A9), "X101-K1": ("X101", 1, {})}


@pytest.mark.parametrize("cfg", list(ROUND_TRIP))
def test_state_dict_returns_the_bytes_that_were_loaded(cfg):
    """K = 1, 2, 3: the mask predictor's padding to 4 rows and the (K + 1) + 4 K fused rows; A = 9: 48 fused RPN rows; X101: the grouped
    conv2 in its block-diagonal window layout"""
    from ampis_amd import _lib, params as P
    from ampis_amd.model import MaskRCNN
    arch, K, akw = ROUND_TRIP[cfg]
    ctx = _lib.Context(0)
    m = MaskRCNN(ctx, K, max_batch=1, max_h=128, max_w=160, max_out_hw=160, detections_per_image=D, arch=arch, **akw)
    try:
        assert m.num_anchors == (9 if akw else 3)
        p = P.init_params(K, seed=8, style="spread", arch=arch, num_anchors=m.num_anchors)
        m.load_params(p)
        sd = m.state_dict()
        assert set(sd) == {k for k in p if ".norm." not in k}
        bad = [k for k in sd if sd[k].tobytes() != p[k].tobytes() or sd[k].shape != p[k].shape]
        assert not bad, bad[:6]
    finally:
        m.close()
        ctx.close()


def test_grouped_backbone_keeps_its_padding_through_a_step():
    """X101 after a step with weight decay: the off-diagonal window slots of the grouped weights (and every other padding row) hold what a
    fresh load of state_dict() holds: the same step, the same gradient arena and, after another sgd_step, the same momentum arena -- zeros
    there.  (A slot of the parameter arena can only leave zero through a momentum that is not zero: p -= lr * v.)"""
    r = Rig("a", K=1, arch="X101")
    try:
        probe(r, "step")
    finally:
        r.close()


@pytest.mark.parametrize("cfg", ["R50-K3", "R50-K2-A9"])
def test_padded_rows_keep_their_zeros_through_a_step(cfg):
    """K = 3 (mask predictor rows 3..4, 16 fused box rows) and A = 9 (45 fused RPN rows of 48) after a step with weight decay: the same
    step, gradient arena, state_dict() and momentum arena as a fresh load of state_dict() -- whose padding rows are zeros"""
    arch, K, akw = ROUND_TRIP[cfg]
    r = Rig("a", K=K, arch=arch, anchors=akw)
    try:
        assert r.M.num_anchors == (9 if akw else 3)
        probe(r, "step")
    finally:
        r.close()


# ---- a weight that crosses the range of the split copy after load ----------------------------------------------------------------------------
def test_weight_pushed_beyond_the_split_range_by_a_step(rig_a):
    """w_absmax is the largest |w| seen at LOAD: a step that lifts a weight of a split-eligible trunk layer beyond 65504 leaves the model with
    a split copy a fresh model would not make.  What is promised: the next infer() is finite and equals, byte for byte, a fresh model on an
    AMP_CONV_F32 context (the split copy's overflow raised the range flag and the batch was run again in fp32: f32_reruns + 1) or a fresh
    model on an AMP_CONV_F16X3 context (no re-run).  Equality with the fresh F16X3 model is NOT required: that one keeps the one layer on fp32
    and runs the rest split, the used model re-runs the whole batch in fp32.
    What the library gives (MI355X): the first of the two -- f32_reruns goes up by one and the bytes are those of the fresh AMP_CONV_F32
    model, not those of the fresh AMP_CONV_F16X3 model.  amp_model_sgd_step does not have to update w_absmax for this to hold."""
    r, M = rig_a, rig_a.M
    name = T.BB + "res3.0.conv1.weight"
    r.step()
    buf = np.zeros_like(M.get_tensor(name))
    buf[0, 0, 0, 0] = 1e7
    assert M.load_momentum_dict({name: buf}) == []
    r.sgd(lr=0.01, momentum=0.9, weight_decay=0.0)          # w -= 0.01 * (0.9e7 + g)
    try:
        assert 65504.0 < float(np.abs(M.get_tensor(name)).max()) < 1e6
        n0 = M.f32_reruns
        got = M.infer(r.imgs_inf)
        reran = M.f32_reruns - n0
        assert all(np.isfinite(o["boxes"]).all() and np.isfinite(o["scores"]).all() for o in got), "non-finite detections"
        eq = {}
        for mode in ("f16x3", "f32"):
            F, fctx = r.fresh(mode=mode)
            try:
                eq[mode] = same_bytes(got, F.infer(r.imgs_inf))
            finally:
                F.close()
                fctx.close()
        print(f"f32_reruns + {reran}; equals the fresh model on f16x3: {eq['f16x3']}, on f32: {eq['f32']}")
        assert eq["f16x3"] or eq["f32"], "infer() after the weight left the range matches neither fresh reference"
        assert (reran == 1 and eq["f32"]) or (reran == 0 and eq["f16x3"]), (reran, eq)
    finally:      # the module's model goes on with the weight and its momentum back in range
        p = r.current_params()
        w = p[name].copy()
        w[0, 0, 0, 0] = 0.0
        p[name] = w
        r.load(p)
        v = M.get_tensor(name, momentum=True)
        v[0, 0, 0, 0] = 0.0
        M.load_momentum_dict({name: v})
