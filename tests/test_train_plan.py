"""The training step's plan (csrc/train_plan.h, shown by amp_debug_train_plan) against a transcription of the expressions run_train held before
the plan existed: ampis_amd/csrc/model.hip at commit ba05c34, cited by line.  No GPU.

The reference below is that commit's source, not the header: a rule that changes in train_plan.h fails here until the change is meant and
the transcription is edited with it.  Boolean inputs are covered by their full product, under the default switches and under every single
switch flipped; every numeric input at each threshold and its two neighbours."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from ampis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ("backward dry conv_mode split_stale rpn_batch rpn_ld pred_cout pred_cin pred_scale conv_cout conv_cin conv_kh conv_kw "
          "acts_split gs_chain_ok num_groups stride_in_1x1 lv_ld fc1_split N Kp fcn_split deconv_split predictor_split "
          "bias xfmt cout cin kh kw rows dys_floats has_wt_split same_dy copy_rows reserved").split()
SWITCHES = ("train_native dgrad_batch rpn_sparse rpn_train_fuse mask_tail_split deconv_split async_reduce split_grads fused_bias dy_convert "
            "dy_convert_min_rows dy_reuse gx rpn_split gx_dy_inkernel split_chain").split()
OUT = ("refresh_fwd dgrad_batch sr_ok rpn_train_fused HS AS GSW GS GX last_chain SR async_on MS MT DS "
       "wgrad_convert wgrad_fused dgrad_wsplit dy_reuse rpn_level_split gx_dy_pass").split()
BOOLS = ("backward dry conv_mode split_stale pred_scale acts_split gs_chain_ok stride_in_1x1 fc1_split fcn_split deconv_split predictor_split "
         "bias has_wt_split same_dy").split()
# a step on which every path can be on: R50 head shapes, 512 foreground RoIs, and as the layer of the per-layer rules the FPN output conv at p2 of B = 4, 1024 x 1024
BASE = dict(backward=1, dry=0, conv_mode=1, split_stale=0, rpn_batch=256, rpn_ld=16, pred_cout=16, pred_cin=256, pred_scale=0, conv_cout=256, conv_cin=256,
            conv_kh=3, conv_kw=3, acts_split=1, gs_chain_ok=1, num_groups=1, stride_in_1x1=1, lv_ld=16, fc1_split=1, N=512, Kp=4, fcn_split=1, deconv_split=1,
            predictor_split=1, bias=1, xfmt=1, cout=256, cin=256, kh=3, kw=3, rows=262144, dys_floats=262144 * 256, has_wt_split=1, same_dy=1, copy_rows=262144, reserved=0)
DEFAULTS = dict(train_native=1, dgrad_batch=1, rpn_sparse=1, rpn_train_fuse=1, mask_tail_split=1, deconv_split=1, async_reduce=1, split_grads=1, fused_bias=1,
                dy_convert=1, dy_convert_min_rows=200000, dy_reuse=1, gx=1, rpn_split=1, gx_dy_inkernel=0, split_chain=1)


def env_switches():
    """The switches as the library reads them from this process's environment (TrainSwitches' initialisers; the variables of model.hip ba05c34)."""
    e = os.environ
    off = lambda name: 0 if name in e else 1
    return dict(train_native=off("AMP_NO_TRAIN_NATIVE"), dgrad_batch=off("AMP_NO_DGRAD_BATCH"), rpn_sparse=off("AMP_NO_RPN_SPARSE"),
                rpn_train_fuse=off("AMP_NO_RPN_TRAIN_FUSE"), mask_tail_split=off("AMP_NO_MASK_TAIL_SPLIT"), deconv_split=off("AMP_NO_DECONV_SPLIT"),
                async_reduce=int(int(e["AMP_ASYNC_REDUCE"]) != 0) if "AMP_ASYNC_REDUCE" in e else 1, split_grads=off("AMP_NO_SPLIT_GRADS"),
                fused_bias=off("AMP_NO_FUSED_BIAS"), dy_convert=off("AMP_NO_DY_CONVERT"),
                dy_convert_min_rows=int(e.get("AMP_DY_CONVERT_MIN_ROWS", 200000)), dy_reuse=off("AMP_NO_DY_REUSE"), gx=off("AMP_NO_GX"),
                rpn_split=off("AMP_NO_RPN_SPLIT"), gx_dy_inkernel=1 - off("AMP_GX_DY_INKERNEL"), split_chain=off("AMP_NO_SPLIT_CHAIN"))


def parent(rows_, sw):
    """What model.hip at ba05c34 decides: rows_ is an [n, 36] integer matrix in the order of INPUTS, sw a dict of SWITCHES; returns [n, 21] in the order of OUT."""
    i = {k: rows_[:, j].astype(np.int64) for j, k in enumerate(INPUTS)}
    b = lambda k: i[k] != 0
    s = lambda k: bool(sw[k])
    f16 = i["conv_mode"] == 1                                                                                      # AMP_CONV_F16X3
    dry, backward = b("dry"), b("backward")
    o = {}
    # l. 891: if (!dry && m->split_stale && m->ctx->conv_mode == AMP_CONV_F16X3 && getenv("AMP_NO_TRAIN_NATIVE") == nullptr) refresh_split_weights
    o["refresh_fwd"] = ~dry & b("split_stale") & f16 & s("train_native")
    # l. 892-893: dgrad_batch = !dry && backward && !no_dgrad_batch && conv_mode == AMP_CONV_F16X3
    o["dgrad_batch"] = ~dry & backward & s("dgrad_batch") & f16
    # l. 897-905: sr_ok stays false in the plan run; else backward && rpn_sparse && cpred.cout == T_ld && cpred.cin == 256 && cpred.scale == nullptr &&
    #             c.rpn_batch <= 512 && cconv.cout == 256 && cconv.cin == 256 && cconv.kh == 3 && cconv.kw == 3
    o["sr_ok"] = (~dry & backward & s("rpn_sparse") & (i["pred_cout"] == i["rpn_ld"]) & (i["pred_cin"] == 256) & ~b("pred_scale") & (i["rpn_batch"] <= 512) &
                  (i["conv_cout"] == 256) & (i["conv_cin"] == 256) & (i["conv_kh"] == 3) & (i["conv_kw"] == 3))
    # l. 906: m->rpn_train_fused = !dry && sr_ok && rpn_train_fuse && conv_mode == AMP_CONV_F16X3
    o["rpn_train_fused"] = ~dry & o["sr_ok"] & s("rpn_train_fuse") & f16
    # l. 1000: HS = backward && m->acts_split && CONV("roi_heads.box_head.fc1").w_split != nullptr
    o["HS"] = backward & b("acts_split") & b("fc1_split")
    # l. 1166: AS = m->acts_split
    o["AS"] = b("acts_split")
    # l. 1156: GSW = m->acts_split && getenv("AMP_NO_SPLIT_GRADS") == nullptr && ctx->conv_mode == AMP_CONV_F16X3
    o["GSW"] = b("acts_split") & s("split_grads") & f16
    # l. 1224: GS = AS && !no_gs && ctx->conv_mode == AMP_CONV_F16X3 && m->gs_chain_ok
    o["GS"] = o["AS"] & s("split_grads") & f16 & b("gs_chain_ok")
    # l. 1226: GX = AS && !GS && !no_gs && gx && ctx->conv_mode == AMP_CONV_F16X3 && c.num_groups > 1 && !c.stride_in_1x1
    o["GX"] = o["AS"] & ~o["GS"] & s("split_grads") & s("gx") & f16 & (i["num_groups"] > 1) & ~b("stride_in_1x1")
    # l. 1227: m->last_chain = !AS ? 0 : (GS ? 2 : (GX ? 3 : 1))
    o["last_chain"] = np.where(~o["AS"], 0, np.where(o["GS"], 2, np.where(o["GX"], 3, 1)))
    # l. 1359: SR = sr_ok && T.lv.ld == cpred.cout
    o["SR"] = o["sr_ok"] & (i["lv_ld"] == i["pred_cout"])
    # l. 1146: async_on = getenv("AMP_ASYNC_REDUCE") ? atoi(...) != 0 : true
    o["async_on"] = np.full(len(rows_), s("async_reduce"))
    # l. 235-244, split_chain(): false if off || m->ws.dry || conv_mode != AMP_CONV_F16X3 || m->split_stale, or if a named layer has no split copy.
    # By the time the mask head asks, refresh_split_weights (l. 2039) has cleared split_stale if l. 891 called it.
    stale = b("split_stale") & ~o["refresh_fwd"]
    chain = lambda has: ~(~np.bool_(s("split_chain")) | dry | ~f16 | stale) & has
    # l. 1064-1065: MS = backward && m->acts_split && split_chain(m, {mask_fcn1 .. mask_fcn4})
    o["MS"] = backward & b("acts_split") & chain(b("fcn_split"))
    # l. 1071: MT = MS && mask_tail_split && Kp <= 16 && (size_t)N * 784 * 256 * 4 < 0x80000000ull && ((long long)N * 196 + 127) / 128 >= 512 && split_chain(m, {deconv})
    #  (l. 1257 derives it again in the backward half as m->mask_tail_split && conv_mode == AMP_CONV_F16X3: the same value, split_chain has asked for the mode)
    o["MT"] = (o["MS"] & s("mask_tail_split") & (i["Kp"] <= 16) & (i["N"] * 784 * 256 * 4 < 0x80000000) & ((i["N"] * 196 + 127) // 128 >= 512) &
               chain(b("deconv_split")))
    assert np.array_equal(o["MT"], o["MT"] & f16)
    # l. 1082: DS = MT && !no_ds && split_chain(m, {predictor})
    o["DS"] = o["MT"] & s("deconv_split") & chain(b("predictor_split"))
    # ---- the layer ----
    bias, xfmt, cout, cin, rows = b("bias"), i["xfmt"], i["cout"], i["cin"], i["rows"]
    kk = i["kh"] * i["kw"] * cin
    # l. 1180-1181: bias && xfmt == 1 && GSW && !no_conv && cw.cout % 128 == 0 && cw.cin % 128 == 0 && kh * kw * cin >= 256 &&
    #               (Mo >= dyc_min_rows || (kh * kw * cin >= 4096 && Mo >= 4096)) && (size_t)Mo * cw.cout <= DYS_SCRATCH
    o["wgrad_convert"] = (bias & (xfmt == 1) & o["GSW"] & s("dy_convert") & (cout % 128 == 0) & (cin % 128 == 0) & (kk >= 256) &
                          ((rows >= sw["dy_convert_min_rows"]) | ((kk >= 4096) & (rows >= 4096))) & (rows * cout <= i["dys_floats"]))
    # l. 1174: fused = bias && ctx->conv_mode == AMP_CONV_F16X3 && !no_fused_bias && !(xfmt & 2)
    o["wgrad_fused"] = bias & f16 & s("fused_bias") & ((xfmt & 2) == 0)
    # l. 1196-1200: dgrad_wsplit: null if !dgrad_batch || !cw.wt_split; else xb = B_*Hy*Wy*cout*4 < 0x80000000 && wb = cout*kh*kw*cin*4 < 0x80000000
    o["dgrad_wsplit"] = o["dgrad_batch"] & b("has_wt_split") & (rows * cout * 4 < 0x80000000) & (cout * kk * 4 < 0x80000000)
    # l. 1215: dy == dys_of && !no_reuse && dys_rows == (long long)B_ * Hy * Wy
    o["dy_reuse"] = b("same_dy") & s("dy_reuse") & (i["copy_rows"] == rows)
    # l. 1392: GSW && !no_rpn_split && Ml >= 200000 && (size_t)Ml * 256 <= DYS_SCRATCH && cpred.scale == nullptr && T.lv.ld == 16 && cpred.cout <= 16 && cconv.cout == 256
    o["rpn_level_split"] = (o["GSW"] & s("rpn_split") & (rows >= 200000) & (rows * 256 <= i["dys_floats"]) & ~b("pred_scale") & (i["lv_ld"] == 16) &
                            (i["pred_cout"] <= 16) & (i["conv_cout"] == 256))
    # l. 1579: dy_pass = getenv("AMP_GX_DY_INKERNEL") == nullptr
    o["gx_dy_pass"] = np.full(len(rows_), not s("gx_dy_inkernel"))
    return np.stack([np.asarray(o[k]).astype(np.int32) for k in OUT], axis=1)


def library(rows_, sw=None):
    """amp_debug_train_plan for every row; sw: a dict of SWITCHES, or None for the process's state"""
    fn = _lib.lib().amp_debug_train_plan
    rows_ = np.ascontiguousarray(rows_, dtype=np.int32)
    out = np.full((len(rows_), len(OUT)), -1, dtype=np.int32)
    swa = np.array([sw[k] for k in SWITCHES], dtype=np.int32) if sw is not None else None
    p_in, p_out, p_sw = rows_.ctypes.data, out.ctypes.data, (swa.ctypes.data if swa is not None else None)
    si, so = rows_.strides[0], out.strides[0]
    for r in range(len(rows_)):
        assert fn(p_in + r * si, p_sw, p_out + r * so) == 0
    return out


def matrix(cases):
    return np.array([[dict(BASE, **c)[k] for k in INPUTS] for c in cases], dtype=np.int32)


def product_rows(names=BOOLS, xfmts=(0, 1, 2, 3)):
    base = np.array([BASE[k] for k in INPUTS], dtype=np.int32)
    combos = np.array(list(itertools.product((0, 1), repeat=len(names))), dtype=np.int32)
    rows_ = np.tile(base, (len(combos) * len(xfmts), 1))
    for j, k in enumerate(names):
        rows_[:, INPUTS.index(k)] = np.repeat(combos[:, j], len(xfmts))
    rows_[:, INPUTS.index("xfmt")] = np.tile(np.array(xfmts, dtype=np.int32), len(combos))
    return rows_


def explain(rows_, got, ref):
    r, c = np.argwhere(got != ref)[0]
    return f"{OUT[c]}: library {got[r, c]}, ba05c34 {ref[r, c]} for {dict(zip(INPUTS, rows_[r].tolist()))}"


def check(rows_, sw):
    got, ref = library(rows_, sw), parent(rows_, sw)
    assert np.array_equal(got, ref), explain(rows_, got, ref)


def test_the_tables_have_the_sizes_the_entry_point_documents():
    assert len(INPUTS) == 36 and len(SWITCHES) == 16 and len(OUT) == 21 and set(BASE) == set(INPUTS) and set(DEFAULTS) == set(SWITCHES)


def test_full_product_of_the_boolean_inputs_under_the_default_switches():
    rows_ = product_rows()
    assert len(rows_) == 2 ** len(BOOLS) * 4
    check(rows_, DEFAULTS)
    ref = parent(rows_, DEFAULTS)
    for j, k in enumerate(OUT):          # the product reaches both answers of every decision (last_chain: all four chains)
        assert set(np.unique(ref[:, j])) >= ({0, 1, 2} if k == "last_chain" else {0, 1}) or k in ("async_on", "gx_dy_pass", "GX"), k
    x = product_rows()
    x[:, INPUTS.index("num_groups")] = 32      # ResNeXt: chain 3
    check(x, DEFAULTS)
    assert 3 in parent(x, DEFAULTS)[:, OUT.index("last_chain")] and parent(x, DEFAULTS)[:, OUT.index("GX")].any()


@pytest.mark.parametrize("switch", SWITCHES)
def test_full_product_of_the_boolean_inputs_with_one_switch_flipped(switch):
    sw = dict(DEFAULTS)
    sw[switch] = 300000 if switch == "dy_convert_min_rows" else 1 - DEFAULTS[switch]      # (BASE's layer has 262 144 rows)
    groups = 32 if switch == "gx" else 1
    rows_ = product_rows()
    rows_[:, INPUTS.index("num_groups")] = groups
    check(rows_, sw)
    assert not np.array_equal(parent(rows_, sw), parent(rows_, DEFAULTS)), "the switch decides nothing on these rows"


def _around(key, threshold, **fixed):
    return [dict(fixed, **{key: v}) for v in (threshold - 1, threshold, threshold + 1)]


NUMERIC = (
    _around("rpn_batch", 512) + _around("rpn_ld", 16) + _around("pred_cout", 16) + _around("pred_cin", 256) + _around("conv_cout", 256) + _around("conv_cin", 256) +
    _around("conv_kh", 3) + _around("conv_kw", 3) + _around("lv_ld", 16) + _around("pred_cout", 16, rpn_ld=17, lv_ld=17) +
    _around("num_groups", 1, gs_chain_ok=0, stride_in_1x1=0) + _around("conv_mode", 1) +
    _around("N", 334) +                         # ceil(N * 196 / 128) >= 512 from N = 334 on
    _around("N", 2675) + _around("N", 0) +      # N * 784 * 256 * 4 < 2^31 up to N = 2674
    _around("Kp", 16) +
    _around("cout", 128) + _around("cout", 256) + _around("cin", 128) + _around("cin", 256) +
    [dict(kh=1, kw=1, cin=c) for c in (128, 256, 384)] +                                       # K = kh * kw * cin >= 256
    _around("rows", 200000, dys_floats=2 ** 31 - 1) +
    [dict(kh=1, kw=1, cin=c, rows=r, dys_floats=2 ** 31 - 1) for c in (3968, 4096, 4224) for r in (4095, 4096, 4097)] +      # the deep rule: K >= 4096 and rows >= 4096
    _around("dys_floats", 262144 * 256) +
    _around("rows", 2097152, dys_floats=2 ** 31 - 1) +                                         # rows * cout * 4 < 2^31
    _around("cin", 8192, cout=8192, kh=2, kw=4) + _around("cin", 8192, cout=8192, kh=2, kw=2) +      # cout * kh * kw * cin * 4 < 2^31
    _around("copy_rows", 262144) + _around("xfmt", 1) + _around("xfmt", 2)
)


def test_every_numeric_input_at_its_thresholds_and_their_neighbours():
    rows_ = matrix(NUMERIC)
    check(rows_, DEFAULTS)
    check(rows_, dict(DEFAULTS, rpn_sparse=0, fused_bias=0))
    low = matrix(_around("rows", 1000, dys_floats=2 ** 31 - 1))
    check(low, dict(DEFAULTS, dy_convert_min_rows=1000))                 # AMP_DY_CONVERT_MIN_ROWS moves the threshold
    ref = parent(low, dict(DEFAULTS, dy_convert_min_rows=1000))[:, OUT.index("wgrad_convert")]
    assert ref.tolist() == [0, 1, 1]
    ref = parent(rows_, DEFAULTS)
    for j, k in enumerate(OUT):
        assert len(np.unique(ref[:, j])) > 1 or k in ("refresh_fwd", "dgrad_batch", "HS", "AS", "GSW", "async_on", "MS", "gx_dy_pass"), k


@pytest.mark.parametrize("setter, switch", [("amp_debug_set_split_chain", "split_chain"), ("amp_debug_set_rpn_train_fuse", "rpn_train_fuse"),
                                            ("amp_debug_set_rpn_sparse", "rpn_sparse"), ("amp_debug_set_mask_tail_split", "mask_tail_split"),
                                            ("amp_debug_set_gx", "gx")])
def test_a_setter_overrides_the_environment_and_minus_one_returns_to_it(setter, switch):
    env = env_switches()
    rows_ = product_rows(("backward", "dry", "conv_mode", "split_stale", "acts_split", "gs_chain_ok", "stride_in_1x1", "fcn_split", "deconv_split"), xfmts=(1,))
    rows_[:, INPUTS.index("num_groups")] = 32
    fn = getattr(_lib.lib(), setter)
    fn.argtypes, fn.restype = [C.c_int], None
    try:
        for v in (0, 1):
            fn(v)
            got, ref = library(rows_), parent(rows_, dict(env, **{switch: v}))
            assert np.array_equal(got, ref), (v, explain(rows_, got, ref))
        assert not np.array_equal(parent(rows_, dict(env, **{switch: 0})), parent(rows_, dict(env, **{switch: 1})))
    finally:
        fn(-1)
    got, ref = library(rows_), parent(rows_, env)
    assert np.array_equal(got, ref), explain(rows_, got, ref)


def test_the_step_reads_no_environment_variable():
    src = os.path.join(ROOT, "ampis_amd", "csrc")
    assert "getenv" not in open(os.path.join(src, "model_train.h")).read()
    plan = open(os.path.join(src, "train_plan.h")).read()
    body = plan[plan.index("constexpr int TRAIN_SWITCH_COUNT"):]
    assert "getenv" not in body and "amp_model*" not in body and "amp_ctx*" not in body          # only TrainSwitches' initialisers read it; the functions are pure
