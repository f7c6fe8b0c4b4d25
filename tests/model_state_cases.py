"""The table of state transitions of amp_model (ampis_amd/csrc/model.hip) that tests/test_model_state_gpu.py applies to a used model before
it compares the model's next call with a freshly loaded one's, byte for byte.

A case is dict(name, calls, sizes, what, apply):
  calls   the extern "C" entry points of model.hip the transition goes through.  tests/test_model_state_cases.py (no GPU) holds the table
          to the source: every entry point that marks the split copies stale, clears `finalized` or writes `img_hw` must be named here.
  sizes   the sizes of the GPU file the case runs at: "a" (128 x 160) for every case, "b" (448 x 448, where the paths gated on fresh
          split copies run: the fused RPN head from 24576 rows at a level) for the cases around sgd_step and forward-only calls.
  what    the derived state the transition could leave behind.
  apply   apply(rig): the transition itself on rig.M.  `rig` is the Rig of the GPU file: M, ctx, base (the parameters last loaded), step()
          (one forward_backward on the training batch), sgd(**kw), infer(), forward(), load(params), set_sizes(sizes).

This module imports nothing that needs a GPU."""
import ctypes as C

import numpy as np

BB = "backbone.bottom_up."
PLAIN = dict(lr=0.002, momentum=0.9, weight_decay=1e-4)
GENERAL = dict(lr=0.002, momentum=0.9, weight_decay=1e-4, nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip=("norm", 1.0, 2.0))
BIG_LAYER = BB + "res3.1.conv2"            # split-eligible (Cin 128); the layer of test_weights_beyond_the_range_leave_the_split_path_without_a_rerun
REFINALIZE_TENSOR = "roi_heads.box_predictor.cls_score.weight"      # one half of a fused matrix: the other half and both biases must come from the device


def last_sgd_path(rig):
    from ampis_amd import _lib
    return _lib.lib().amp_debug_last_sgd_path(rig.M._h)


def sgd_plain(rig):
    rig.step()
    rig.sgd(**PLAIN)
    assert last_sgd_path(rig) == 1


def sgd_general(rig):
    rig.step()
    rig.sgd(**GENERAL)
    assert last_sgd_path(rig) == 2
    stats = rig.M.clip_stats()
    assert len(stats) == len(rig.M.trainable_names())
    assert all(np.isfinite(n) and 0.0 < k <= 1.0 for n, k in stats.values()), "clip_stats of a norm-clipped step"


def two_steps_no_infer(rig):
    for _ in range(2):
        rig.step()
        rig.sgd(**PLAIN)


def infer_between_steps(rig):
    rig.step()
    rig.sgd(**PLAIN)
    rig.infer()
    rig.step()
    rig.sgd(**PLAIN)


def forward_only_after_step(rig):
    rig.step()
    rig.sgd(**PLAIN)
    rig.forward()


def with_big_weight(params):
    """one weight of 61000 in BIG_LAYER, undone by 2^-16 in the layer's FrozenBN scale: amp_model_finalize gives the layer no split copy"""
    q = dict(params)
    w = q[BIG_LAYER + ".weight"].copy()
    w[0, 0, 0, 0] = 61000.0
    q[BIG_LAYER + ".weight"] = w
    q[BIG_LAYER + ".norm.weight"] = params[BIG_LAYER + ".norm.weight"] * np.float32(2.0 ** -16)
    return q


def reload_params(rig):
    """other weights on the same model: first with one layer beyond the range of a split copy (a smaller split arena, other job tables),
    used for an inference and a step, then weights that are all in range again (the arena grows back).  The momentum stays."""
    from ampis_amd import params as P
    n0 = rig.M.f32_reruns
    rig.load(with_big_weight(P.init_params(rig.K, seed=5, style="spread")))
    rig.infer()
    rig.step()
    rig.sgd(**PLAIN)
    assert rig.M.f32_reruns == n0, "a layer without a split copy is no reason for a re-run"
    rig.load(P.init_params(rig.K, seed=4, style="spread"))


def momentum_round_trip(rig):
    """momentum(value) and load_momentum_dict are inverses of momentum() and momentum_dict(), and the dict covers everything that is not zero:
    the padding rows of the arena hold zeros and stay untouched"""
    M = rig.M
    rig.step()
    rig.sgd(**PLAIN)
    v0 = M.momentum()
    d = M.momentum_dict()
    assert any(np.abs(a).max() > 0 for a in d.values())
    M.momentum(np.zeros_like(v0))
    assert not M.momentum().any()
    assert M.load_momentum_dict(d) == []
    assert M.momentum().tobytes() == v0.tobytes(), "momentum_dict -> load_momentum_dict does not restore the arena (padding rows not zero?)"
    M.momentum(v0 * np.float32(0.5))
    assert M.momentum().tobytes() == (v0 * np.float32(0.5)).tobytes()


def conv_mode_round_trip(rig):
    """f16x3 -> f32, a step and an inference there (amp_model_infer refreshes nothing in fp32: the copies stay stale), f32 -> f16x3"""
    rig.step()
    rig.sgd(**PLAIN)
    rig.ctx.conv_mode = "f32"
    try:
        rig.step()
        rig.sgd(**PLAIN)
        rig.infer()
    finally:
        rig.ctx.conv_mode = "f16x3"


def rerun_then_in_range(rig):
    """the "stem" scaling of test_range_guard_model_gpu.SITES: the stem's output leaves the fp16 range, the inference and the step are run
    again in fp32; then the unscaled parameters, in range"""
    import test_range_guard_model_gpu as G
    rig.step()
    rig.sgd(**PLAIN)
    cur = rig.current_params()
    k = G.pow2_for(rig.stem_peak(cur))
    n0 = rig.M.f32_reruns
    rig.load(G.scaled(cur, "stem", k))
    rig.infer()
    assert rig.M.f32_reruns == n0 + 1, "the scaled stem did not trigger the fp32 re-run of the inference"
    rig.step()
    assert rig.M.f32_reruns == n0 + 2, "the scaled stem did not trigger the fp32 re-run of the step"
    rig.sgd(**PLAIN)
    back = dict(cur)                         # the unscaled FrozenBN and frozen layers (the scaling touched nothing else) ...
    back.update({n: rig.M.get_tensor(n) for n in rig.M.trainable_names()})      # ... under the stepped weights
    rig.load(back)
    rig.infer()
    assert rig.M.f32_reruns == n0 + 2, "an in-range call after a re-run was re-run too"


def ragged_sizes(rig):
    """per-image sizes for a ragged batch, calls, then none again"""
    H, W = rig.H, rig.W
    rig.step()
    rig.sgd(**PLAIN)
    rig.set_sizes([(H - 28, W), (H, W - 30)][:rig.BI])
    rig.infer()
    rig.set_sizes([(H - 28, W - 30), (H - 1, W - 2)][:rig.BT])
    rig.step()
    rig.sgd(**PLAIN)
    rig.set_sizes(None)
    rig.infer()


def ragged_sizes_kept(rig):
    """per-image sizes set and left in force: the fresh model is given the same"""
    rig.step()
    rig.sgd(**PLAIN)
    rig.set_sizes([(rig.H - 28, rig.W), (rig.H, rig.W - 30)][:rig.BI])
    rig.infer()


def loss_opts_round_trip(rig):
    rig.step()
    rig.sgd(**PLAIN)
    rig.M.set_loss_opts(rpn_loss_type="giou", box_smooth_l1_beta=0.5, rpn_loss_weight=2.0, box_bbox_reg_loss_weight=0.5)
    rig.step()
    rig.sgd(**PLAIN)
    rig.M.set_loss_opts()
    assert rig.M.loss_opts()["rpn_loss_type"] == "smooth_l1"


def broadcast(rig):
    """broadcast_params(0) on a communicator of size one: the arenas are overwritten with themselves, the copies marked stale"""
    assert rig.ctx.comm_info()[1] == 1
    rig.step()
    rig.sgd(**PLAIN)
    v0 = rig.M.momentum()
    rig.M.broadcast_params(0)
    rig.ctx.comm_wait()
    assert rig.M.momentum().tobytes() == v0.tobytes()


def load_tensor(model, name, a):
    """amp_model_load_tensor of one tensor (the Python surface only ever reloads all of them)"""
    from ampis_amd import _lib
    a = np.ascontiguousarray(a, dtype=np.float32)
    shape = (C.c_longlong * a.ndim)(*a.shape)
    _lib.check(_lib.lib().amp_model_load_tensor(model._h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim), f"amp_model_load_tensor({name})")


def refinalize(rig):
    """C API only: after a step, one tensor loaded again with its own current value, then amp_model_finalize.  Nothing may change."""
    from ampis_amd import _lib
    M = rig.M
    rig.step()
    rig.sgd(**PLAIN)
    before = M.state_dict()
    load_tensor(M, REFINALIZE_TENSOR, before[REFINALIZE_TENSOR])
    _lib.check(_lib.lib().amp_model_finalize(M._h), "amp_model_finalize")
    after = M.state_dict()
    changed = [k for k in before if before[k].tobytes() != after[k].tobytes()]
    assert not changed, f"reloading {REFINALIZE_TENSOR} with its own value and finalizing again changed {changed}"


TRAIN = ("amp_model_forward_backward",)
STEP = TRAIN + ("amp_model_sgd_step",)
LOAD = ("amp_model_load_tensor", "amp_model_finalize")

CASES = [
    dict(name="sgd_plain", sizes="ab", calls=STEP, apply=sgd_plain,
         what="forward and dgrad split copies, fused predictor split"),
    dict(name="sgd_general", sizes="ab", calls=TRAIN + ("amp_model_sgd_step_ex", "amp_model_clip_stats"), apply=sgd_general,
         what="the same through sgd_general_run, and sgd_plan"),
    dict(name="two_steps_no_infer", sizes="ab", calls=STEP, apply=two_steps_no_infer,
         what="the refresh in amp_model_infer"),
    dict(name="infer_between_steps", sizes="ab", calls=STEP + ("amp_model_infer",), apply=infer_between_steps,
         what="a refresh that the next step must not trust"),
    dict(name="forward_only_after_step", sizes="ab", calls=STEP + ("amp_model_forward_losses",), apply=forward_only_after_step,
         what="the refresh of a forward-only call, or its absence"),
    dict(name="reload_params", sizes="a", calls=LOAD + STEP + ("amp_model_infer",), apply=reload_params,
         what="w_absmax, need and reallocation of split_arena, fwd_jobs_dirty / dgrad_jobs_dirty, sgd_chunks / sgd_plan rebuilt, momentum kept"),
    dict(name="momentum_round_trip", sizes="a", calls=STEP + ("amp_model_momentum_arena", "amp_model_set_momentum_tensor", "amp_model_get_tensor"),
         apply=momentum_round_trip, what="layout inverses, padding rows untouched"),
    dict(name="conv_mode_round_trip", sizes="a", calls=STEP + ("amp_model_infer",), apply=conv_mode_round_trip,
         what="amp_model_infer refreshes only in F16X3 mode: the stale flag must survive the fp32 interval"),
    dict(name="rerun_then_in_range", sizes="a", calls=LOAD + STEP + ("amp_model_infer", "amp_model_f32_reruns"), apply=rerun_then_in_range,
         what="workspace and flags after an fp32 re-run"),
    dict(name="ragged_sizes", sizes="a", calls=STEP + ("amp_model_set_image_sizes", "amp_model_infer"), apply=ragged_sizes,
         what="sticky img_hw, cleared"),
    dict(name="ragged_sizes_kept", sizes="a", calls=STEP + ("amp_model_set_image_sizes", "amp_model_infer"), apply=ragged_sizes_kept,
         what="sticky img_hw, in force"),
    dict(name="loss_opts_round_trip", sizes="a", calls=STEP + ("amp_model_set_loss_opts", "amp_model_get_loss_opts"), apply=loss_opts_round_trip,
         what="sticky loss options"),
    dict(name="broadcast", sizes="a", comm=True, calls=STEP + ("amp_model_broadcast_params", "amp_model_momentum_arena"), apply=broadcast,
         what="split_stale after the arena is overwritten, momentum arena"),
    dict(name="refinalize", sizes="a", calls=STEP + LOAD + ("amp_model_get_tensor",), apply=refinalize,
         what="the fused predictor matrices rebuilt from host copies older than the device's rows"),
]

PROBES = ("infer", "forward", "step")


def case(name):
    return next(c for c in CASES if c["name"] == name)
