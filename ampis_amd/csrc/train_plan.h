// Which path a training step takes: the switches, the thresholds and the pure functions that decide.  Host code only: nothing here knows
// amp_model or amp_ctx, reads the environment after the switches' construction, or calls HIP.  model_train.h asks these functions and launches
// what they say; amp_debug_train_plan (model.hip) shows the same answers to tests/test_train_plan.py without a GPU.
// For model.hip alone (one translation unit): everything sits in the anonymous namespace.
#pragma once
#include <stdlib.h>

#include "../../include/ampis_hip.h"      // AMP_CONV_F16X3

namespace {

// The switches a training step reads, 1 = the path is on.  One instance (g_tsw, model.hip); the environment the process was started with gives the
// initial values, the amp_debug_set_* entries of model.hip overwrite five of them (tests).
struct TrainSwitches {
    int train_native = getenv("AMP_NO_TRAIN_NATIVE") ? 0 : 1;      // EXPERIMENT switch: 0 = a training step's trunk keeps fp32 activations and does not refresh the weights' split copies
    int dgrad_batch = getenv("AMP_NO_DGRAD_BATCH") ? 0 : 1;      // EXPERIMENT switch: 0 = transpose + split in front of every data-gradient conv
    int rpn_sparse = getenv("AMP_NO_RPN_SPARSE") ? 0 : 1;          // EXPERIMENT switch: 0 = the dense backward of the RPN head (amp_debug_set_rpn_sparse)
    int rpn_train_fuse = getenv("AMP_NO_RPN_TRAIN_FUSE") ? 0 : 1;  // EXPERIMENT switch: 0 = the head's hidden tensor saved by the forward pass (amp_debug_set_rpn_train_fuse)
    int mask_tail_split = getenv("AMP_NO_MASK_TAIL_SPLIT") ? 0 : 1;      // EXPERIMENT switch: 0 = fp32 macts[4] and d_mtb (amp_debug_set_mask_tail_split)
    int deconv_split = getenv("AMP_NO_DECONV_SPLIT") ? 0 : 1;      // EXPERIMENT switch: 0 = the deconv's output in fp32
    int async_reduce = getenv("AMP_ASYNC_REDUCE") ? (atoi(getenv("AMP_ASYNC_REDUCE")) != 0 ? 1 : 0) : 1;      // AMP_ASYNC_REDUCE=0: the slab reductions on the main stream
    int split_grads = getenv("AMP_NO_SPLIT_GRADS") ? 0 : 1;      // EXPERIMENT switch: 0 = no scaled split gradients anywhere (chains GS / GX, dy-convert, the RPN split route)
    int fused_bias = getenv("AMP_NO_FUSED_BIAS") ? 0 : 1;      // EXPERIMENT switch: 0 = every bias gradient by amp_colsum
    int dy_convert = getenv("AMP_NO_DY_CONVERT") ? 0 : 1;      // EXPERIMENT switch: 0 = no amp_colsum_split + wgrad_split_kernel route
    long long dy_convert_min_rows = getenv("AMP_DY_CONVERT_MIN_ROWS") ? atoll(getenv("AMP_DY_CONVERT_MIN_ROWS")) : 200000;      // EXPERIMENT switch
    int dy_reuse = getenv("AMP_NO_DY_REUSE") ? 0 : 1;      // EXPERIMENT switch: 0 = the data gradient splits dy itself
    int gx = getenv("AMP_NO_GX") ? 0 : 1;      // EXPERIMENT switch: 0 = ResNeXt blocks on fp32 gradients (split activations only) (amp_debug_set_gx)
    int rpn_split = getenv("AMP_NO_RPN_SPLIT") ? 0 : 1;      // EXPERIMENT switch: 0 = the dense RPN backward's big levels like the small ones
    int gx_dy_inkernel = getenv("AMP_GX_DY_INKERNEL") ? 1 : 0;      // 1 = chain GX decodes conv2's dy on the load (fmt 2) instead of by a pass of its own
    int split_chain = getenv("AMP_NO_SPLIT_CHAIN") ? 0 : 1;      // 0 = split_chain() answers no: fp32 tensors between the heads' convolutions (amp_debug_set_split_chain)
};
constexpr int TRAIN_SWITCH_COUNT = 16;

// ---- thresholds ----
// the LDS-DMA kernels address an operand with 32-bit byte offsets: a tensor they stage stays below 2 GiB
constexpr unsigned long long LDS_DMA_MAX_BYTES = 0x80000000ull;
// the sparse RPN backward's row lists are sized for RPN.BATCH_SIZE_PER_IMAGE <= 512
constexpr int RPN_SPARSE_MAX_BATCH = 512;
// the mask tail keeps fcn4's output split only where the ring kernel takes the deconv's data gradient: from 512 tiles of 128 rows on
constexpr long long MASK_TAIL_MIN_RING_TILES = 512;
// dy-convert: a layer with K = kh * kw * cin >= 4096 pays from 4096 output rows on, any other from TrainSwitches::dy_convert_min_rows (200000) on
constexpr long long DY_CONVERT_DEEP_K = 4096;
constexpr long long DY_CONVERT_DEEP_MIN_ROWS = 4096;
// the dense RPN backward takes the split route on levels of at least this many pixels (p2 at B = 4, 1024 x 1024)
constexpr long long RPN_SPLIT_MIN_ROWS = 200000;

// What the step's decisions depend on.  The three groups become known one after the other; each train_plan_* function reads its own group and
// the groups before it.
struct TrainPlanIn {
    // ---- known at entry ----
    bool backward = false, dry = false;
    int conv_mode = AMP_CONV_F16X3;     // amp_ctx::conv_mode
    bool split_stale = false;           // amp_model::split_stale at entry (the weights' split copies are older than the weights)
    int rpn_batch = 0;                  // RPN.BATCH_SIZE_PER_IMAGE
    int rpn_ld = 0;                     // amp::rpn_ld(A): the row length the sparse backward expects of the fused predictor
    int pred_cout = 0, pred_cin = 0;    // proposal_generator.rpn_head.pred (dry: no layer table yet, all zero)
    bool pred_scale = false;            // ... has a FrozenBN scale
    int conv_cout = 0, conv_cin = 0, conv_kh = 0, conv_kw = 0;      // proposal_generator.rpn_head.conv
    // ---- known after the trunk ----
    bool acts_split = false, gs_chain_ok = false;      // amp_model::acts_split, ::gs_chain_ok as run_trunk left them
    int num_groups = 1;
    bool stride_in_1x1 = true;
    int lv_ld = 0;                      // amp_rpn_levels::ld of the trunk's predictor maps
    bool fc1_split = false;             // roi_heads.box_head.fc1 has a split copy
    // ---- known after the RoI counts are on the host ----
    int N = 0;                          // foreground RoIs of the batch
    int Kp = 0;                         // mask predictor columns, padded to 4
    bool fcn_split = false;             // mask_fcn1..4 all have a split copy
    bool deconv_split = false, predictor_split = false;      // roi_heads.mask_head.deconv / .predictor have one
};

struct TrainPlan {
    // entry
    bool refresh_fwd = false;       // refresh the weights' split copies before the trunk
    bool dgrad_batch = false;       // refresh_dgrad_weights: every data-gradient weight split once per step
    bool sr_ok = false;             // the sparse RPN backward applies as far as the head's shapes say
    bool rpn_train_fused = false;   // run_trunk runs the RPN predictors in the conv's epilogue and saves no hidden tensor
    // after the trunk
    bool HS = false;                // box head: pooled tensor and fc1's input in the split row format
    bool AS = false;                // the trunk's saved activations are in the split row format
    bool GSW = false;               // weight gradients may take dy as a scaled split copy (dy-convert, the RPN split route)
    bool GS = false, GX = false;    // the backbone's chain on scaled split gradients: R50 / R101, ResNeXt
    int last_chain = 0;             // amp_debug_last_backward_chain: 0 fp32 storage, 1 split activations + fp32 gradients, 2 GS, 3 GX
    bool SR = false;                // the RPN head's gradients over the sampled pixels only
    bool async_on = false;          // slab reductions on the side stream
    // after the counts
    bool MS = false;                // mask head: pooled input and fcn1..3 outputs split
    bool MT = false;                // ... and fcn4's output (the deconv's input)
    bool DS = false;                // ... and the deconv's output
};

// split_chain() of model_types.h without the layers: fp32 tensors between convolutions in the plan run, off AMP_CONV_F16X3, and while the split copies are stale
bool split_chain_allowed(const TrainSwitches& sw, bool dry, int conv_mode, bool split_stale) {
    return sw.split_chain != 0 && !dry && conv_mode == AMP_CONV_F16X3 && !split_stale;
}

// What is known at entry decides the two weight refreshes and how the RPN head runs.
void train_plan_entry(const TrainPlanIn& in, const TrainSwitches& sw, TrainPlan* p) {
    const bool f16x3 = in.conv_mode == AMP_CONV_F16X3;
    // the forward trunk of a training step runs on pre-split operands like inference: refresh the weights' split copies (stale since the
    // last SGD step) once here instead of splitting every layer's weights inside its own launch
    // (a forward-only call too: the losses of the same weights must not depend on whether an inference came in between)
    p->refresh_fwd = !in.dry && in.split_stale && f16x3 && sw.train_native != 0;
    p->dgrad_batch = !in.dry && in.backward && sw.dgrad_batch != 0 && f16x3;
    // the RPN head's backward pass runs over the sampled anchors' pixels only (rpn_sparse.hip) -- and then the forward pass need not save the head's hidden
    // tensor: the predictors run in the conv's epilogue as in inference, the backward pass recomputes the rows it needs from the gathered patches
    // (the plan run comes before the parameters: no layer table yet)
    p->sr_ok = !in.dry && in.backward && sw.rpn_sparse != 0 && in.pred_cout == in.rpn_ld && in.pred_cin == 256 && !in.pred_scale && in.rpn_batch <= RPN_SPARSE_MAX_BATCH &&
               in.conv_cout == 256 && in.conv_cin == 256 && in.conv_kh == 3 && in.conv_kw == 3;
    p->rpn_train_fused = p->sr_ok && sw.rpn_train_fuse != 0 && f16x3;
}

// What the trunk left decides the box head's format, the backbone's backward chain and the RPN head's backward route.
void train_plan_trunk(const TrainPlanIn& in, const TrainSwitches& sw, TrainPlan* p) {
    const bool f16x3 = in.conv_mode == AMP_CONV_F16X3;
    // heads of a training step on the native trunk (HS): the pooled tensors and the mask head's hidden activations are stored in the
    // split row format as well (their convolutions stage pre-split operands; wgrad / the ReLU masks of the backward pass read the format)
    p->HS = in.backward && in.acts_split && in.fc1_split;
    p->AS = in.acts_split;
    p->GSW = in.acts_split && sw.split_grads != 0 && f16x3;
    // The backbone's chain on SCALED SPLIT gradients (GS): a gradient tensor is kept as the split rows of d * 2^16, so its data-gradient
    // convolution stages both operands by LDS-DMA on the ring kernel (no split, no scaling: the scale rides through the linear chain),
    // residual and ReLU mask come in the split format, and the weight-gradient kernel passes the halves through (xfmt 3).
    p->GS = p->AS && sw.split_grads != 0 && f16x3 && in.gs_chain_ok;
    p->GX = p->AS && !p->GS && sw.split_grads != 0 && sw.gx != 0 && f16x3 && in.num_groups > 1 && !in.stride_in_1x1;
    p->last_chain = !p->AS ? 0 : (p->GS ? 2 : (p->GX ? 3 : 1));
    p->SR = p->sr_ok && in.lv_ld == in.pred_cout;
    p->async_on = sw.async_reduce != 0;
}

// The foreground count decides the mask head's formats, forward and backward alike.
void train_plan_counts(const TrainPlanIn& in, const TrainSwitches& sw, TrainPlan* p) {
    // a refresh at entry has made the split copies fresh
    const bool chain = split_chain_allowed(sw, in.dry, in.conv_mode, in.split_stale && !p->refresh_fwd);
    p->MS = in.backward && in.acts_split && chain && in.fcn_split;          // macts[0..3] split
    // macts[4] (the deconv's input, the 'dy' operand of ITS weight gradient and the mask of its data gradient) split as well: the deconv runs on
    // the ring kernel, the predictor's data gradient leaves d(deconv out) * 2^16 as split rows with the deconv's bias sums on the side, and the
    // deconv's weight- and data-gradient launches stage both operands as they are (AMP_NO_MASK_TAIL_SPLIT: fp32 macts[4] and d_mtb as before)
    p->MT = p->MS && sw.mask_tail_split != 0 && in.Kp <= 16 && (unsigned long long)in.N * 784 * 256 * 4 < LDS_DMA_MAX_BYTES &&
            ((long long)in.N * 196 + 127) / 128 >= MASK_TAIL_MIN_RING_TILES /* the ring kernel takes the deconv's data gradient */ && chain && in.deconv_split;
    // MT: the deconv's OUTPUT stays in the split row format too (round 4): the ring kernel scatters split rows straight from its accumulators
    // (conv_epilogue_direct, out_mode 1) instead of sending 1.6 GB of fp32 through the staged epilogue; the predictor reads it as a split
    // operand, its weight gradient takes x split, its data gradient the split activation as the ReLU mask (AMP_NO_DECONV_SPLIT: fp32 as before)
    p->DS = p->MT && sw.deconv_split != 0 && chain && in.predictor_split;
}

// ---- per-layer choices ----

// How a layer's weight gradient runs.  bias: the bias gradient (column sums of dy) is wanted too; xfmt: 1 = x split, 2 = dy split and scaled by 2^16;
// rows: output pixels of the layer; dys_floats: the capacity of the scaled split copy's buffer.
struct WgradRoute {
    bool convert;      // one pass over dy gives the bias gradient AND dy * 2^16 in the split format (amp_colsum_split), the weight gradient runs on wgrad_split_kernel
    bool fused;        // else: the AMP_CONV_F16X3 kernel sums the bias gradient on the side from the dy tiles it stages anyway (false and bias: a separate amp_colsum pass)
};
WgradRoute wgrad_route(const TrainSwitches& sw, int conv_mode, bool GSW, bool bias, int xfmt, int cout, int cin, int kh, int kw, long long rows, unsigned long long dys_floats) {
    WgradRoute r;
    r.fused = bias && conv_mode == AMP_CONV_F16X3 && sw.fused_bias != 0 && !(xfmt & 2);
    // a big biased layer whose activation is already split (FPN output / RPN conv at p2, p3; the mask head): one pass over dy gives the bias
    // gradient AND dy * 2^16 in the split format, and the weight gradient runs on wgrad_split_kernel (+35-45 % on these shapes)
    const long long K = (long long)kh * kw * cin;
    r.convert = bias && xfmt == 1 && GSW && sw.dy_convert != 0 && cout % 128 == 0 && cin % 128 == 0 && K >= 256 &&
                (rows >= sw.dy_convert_min_rows || (K >= DY_CONVERT_DEEP_K && rows >= DY_CONVERT_DEEP_MIN_ROWS)) && (unsigned long long)rows * cout <= dys_floats;
    return r;
}

// the split data-gradient weights of this step (refresh_dgrad_weights) where conv_run would take a split copy: its LDS-DMA kernels,
// i.e. operands below 2 GiB (cout % 32 == 0 by construction); false: transpose and split in front of the launch as before
bool dgrad_takes_wsplit(bool dgrad_batch, bool has_wt_split, long long rows, int cout, int kh, int kw, int cin) {
    if (!dgrad_batch || !has_wt_split) return false;
    const unsigned long long xb = (unsigned long long)rows * cout * 4, wb = (unsigned long long)cout * kh * kw * cin * 4;
    return xb < LDS_DMA_MAX_BYTES && wb < LDS_DMA_MAX_BYTES;
}

// a data gradient may stage the scaled split copy the weight gradient of the same dy has just left (same_dy: dy is the tensor the copy was made of);
// the caller still asks conv_kernel_for: only the ring kernel undoes the 2^16
bool dy_reuse_allowed(const TrainSwitches& sw, bool same_dy, long long copy_rows, long long rows) { return same_dy && sw.dy_reuse != 0 && copy_rows == rows; }

// the dense RPN backward, per level: big levels on the native trunk: the predictor's data gradient (K = 15) is one bandwidth-bound pass that writes
// d_t * 2^16 as split rows and sums the conv's bias gradient on the side; both gradients of the conv then stage that copy on the ring kernels
bool rpn_level_split(const TrainSwitches& sw, bool GSW, long long rows, unsigned long long dys_floats, bool pred_scale, int lv_ld, int pred_cout, int conv_cout) {
    return GSW && sw.rpn_split != 0 && rows >= RPN_SPLIT_MIN_ROWS && (unsigned long long)rows * 256 <= dys_floats && !pred_scale && lv_ld == 16 && pred_cout <= 16 && conv_cout == 256;
}

// chain GX: conv2's dy is decoded by a pass of its own: decoding it on the load (fmt 2) costs the kernel more than the pass (55.1 against 52.8 ms
// per X-101 step, A/B in one call; AMP_GX_DY_INKERNEL=1 for the other)
bool gx_dy_pass(const TrainSwitches& sw) { return sw.gx_dy_inkernel == 0; }

}  // namespace
