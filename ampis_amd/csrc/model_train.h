// The training step of amp_model: forward + the five losses (TrainStep), then the gradients of every trainable parameter (Backward).  run_train at the
// end of the file is the list of stages.  Which path a stage takes is decided in train_plan.h (TrainStep::plan and the per-layer rules); nothing here reads
// the environment.  With ws.dry nothing is launched: the stages only reserve their buffers, in the same order and sizes as a live run.
// For model.hip alone (one translation unit).
#pragma once
#include <algorithm>

#include "model_types.h"

namespace {

// AMP_ALLOC into a member (or any variable that exists already); the message names it like AMP_ALLOC does
#define AMP_ALLOC_TO(var, T, n)                                                               \
    var = ws.get<T>((size_t)(n));                                                             \
    if (!var) { amp::set_error("amp_model: workspace exhausted allocating %s (%zu bytes, cap %zu)", #var, \
                               (size_t)(n) * sizeof(T), ws.cap); return AMP_ERR_NOMEM; }

// One call of run_train: its arguments, the trunk's results, the plan, every workspace buffer of the forward half and the counts the host reads on the way.
struct TrainStep {
    amp_model* m; const uint8_t* imgs_d; int B, H, W; const amp_gt* gt; unsigned int seed; float* losses; bool backward;
    Bump& ws; const bool dry; const amp_model_cfg& c; amp_ctx* ctx;
    Trunk T;
    TrainPlanIn in;
    TrainPlan plan;
    int K, Kp, ld_box, RB, R;
    int A = 0;                          // anchors per image over the five levels
    int total_gt = 0, npoly = 0, n_polys = 0;
    size_t n_runs = 0;
    // ---- ground truth on the device ----
    float* d_gt_boxes = nullptr; int* d_gt_cls = nullptr; int* d_gt_off = nullptr;
    int* d_poly_off = nullptr; int* d_inst_poly_off = nullptr; double* d_poly_xy = nullptr; unsigned long long* d_rle_off = nullptr; int* d_rle_hw = nullptr;
    // ---- RPN labels and samples ----
    float* match_val = nullptr; int* match_idx = nullptr; unsigned int* gt_best = nullptr; signed char* label = nullptr; uint32_t* keys = nullptr;
    int* rpn_sampled = nullptr; int* rpn_counts = nullptr; float* rpn_partial = nullptr;
    float* d_rpn_pred[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // ---- RoIs and the box head ----
    Proposals PR;
    uint32_t* rkeys = nullptr; int* rcls_s = nullptr; int* rgti_s = nullptr;
    float* rois = nullptr; int* roi_cls = nullptr; int* roi_gti = nullptr; int* roi_counts = nullptr; int* roi_batch_idx = nullptr;
    float* pooled = nullptr; float* fc1 = nullptr; float* fc2 = nullptr; float* box_pred = nullptr; float* box_partial = nullptr; float* d_box_pred = nullptr;
    std::vector<int> h_counts, h_cls, h_gti;
    // ---- the counts on the host ----
    int total_rois = 0, N = 0, Nc = 1;
    std::vector<int> fg_off;
    // ---- mask head ----
    float* m_rois = nullptr; int* m_batch = nullptr; int* m_cls = nullptr; int* m_poly = nullptr;
    float* mpooled = nullptr; float* mt_a = nullptr; float* mt_b = nullptr; float* mlogits = nullptr; float* m_partial = nullptr; unsigned char* m_targets = nullptr;
    float* macts[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // input, fcn1..fcn4 outputs (ping-pong in eval mode)
    float* d_mlogits = nullptr;
    std::vector<float> h_mpart;
    int bm_overflow = 0;

    TrainStep(amp_model* m_, const uint8_t* imgs_d_, int B_, int H_, int W_, const amp_gt* gt_, unsigned int seed_, float* losses_, bool backward_)
        : m(m_), imgs_d(imgs_d_), B(B_), H(H_), W(W_), gt(gt_), seed(seed_), losses(losses_), backward(backward_), ws(m_->ws), dry(m_->ws.dry), c(m_->cfg), ctx(m_->ctx),
          K(m_->cfg.num_classes), Kp((m_->cfg.num_classes + 3) / 4 * 4), ld_box((5 * m_->cfg.num_classes + 1 + 3) / 4 * 4), RB(m_->cfg.roi_batch), R(B_ * m_->cfg.roi_batch) {}
    const ConvW& CONV(const char* key) const { return m->conv.at(key); }
    bool has_split(std::initializer_list<const char*> keys) const {
        for (const char* k : keys) {
            auto it = m->conv.find(k);
            if (it == m->conv.end() || !it->second.w_split) return false;
        }
        return true;
    }

    int trunk();
    int rpn_losses();
    int box_head();
    int mask_buffers();
    int mask_targets_bitmask();
    int mask_head();
    int read_losses();
};

// The plan's entry part, the weight refreshes it asks for, the trunk in saving mode, the plan's second part.
int TrainStep::trunk() {
    m->saving = backward;
    in.backward = backward; in.dry = dry; in.conv_mode = ctx->conv_mode; in.split_stale = m->split_stale;
    in.rpn_batch = c.rpn_batch; in.rpn_ld = amp::rpn_ld(m->rpn_A);
    if (!dry) {      // (the plan run comes before the parameters: no layer table yet)
        const ConvW& cpred = CONV("proposal_generator.rpn_head.pred");
        const ConvW& cconv = CONV("proposal_generator.rpn_head.conv");
        in.pred_cout = cpred.cout; in.pred_cin = cpred.cin; in.pred_scale = cpred.scale != nullptr;
        in.conv_cout = cconv.cout; in.conv_cin = cconv.cin; in.conv_kh = cconv.kh; in.conv_kw = cconv.kw;
    }
    train_plan_entry(in, g_tsw, &plan);
    if (plan.refresh_fwd) AMP_TRY(refresh_split_weights(m));
    if (plan.dgrad_batch) AMP_TRY(refresh_dgrad_weights(m));
    if (!dry) m->rpn_train_fused = plan.rpn_train_fused;
    const int trunk_status = run_trunk(m, imgs_d, B, H, W, T);
    m->saving = false;
    m->rpn_train_fused = false;
    AMP_TRY(trunk_status);
    in.acts_split = m->acts_split; in.gs_chain_ok = m->gs_chain_ok; in.num_groups = c.num_groups; in.stride_in_1x1 = c.stride_in_1x1 != 0; in.lv_ld = T.lv.ld;
    in.fc1_split = !dry && has_split({"roi_heads.box_head.fc1"});
    train_plan_trunk(in, g_tsw, &plan);
    return AMP_OK;
}

// Ground truth to the device, anchor labels, the RPN's sample and its two losses (with the gradient maps d_rpn_pred of a backward step).
int TrainStep::rpn_losses() {
    total_gt = dry ? c.max_gt : gt->gt_off[B];
    npoly = dry ? c.max_poly_doubles : gt->poly_off[gt->inst_poly_off ? gt->inst_poly_off[total_gt] : total_gt];
    AMP_REQUIRE(total_gt <= c.max_gt && npoly <= c.max_poly_doubles, "amp_model_forward_losses: %d instances / %d polygon doubles exceed cfg.max_gt / max_poly_doubles", total_gt, npoly);
    for (int l = 0; l < 5; ++l) A += T.fh[l] * T.fw[l] * m->rpn_A;

    AMP_ALLOC_TO(d_gt_boxes, float, (size_t)std::max(total_gt, 1) * 4);
    AMP_ALLOC_TO(d_gt_cls, int, (size_t)std::max(total_gt, 1));
    AMP_ALLOC_TO(d_gt_off, int, (size_t)B + 1);
    // polygons: one per instance (gt->inst_poly_off == NULL) or a range of polygons per instance; bitmask instances carry run lengths
    n_polys = dry ? c.max_gt : (gt->inst_poly_off ? gt->inst_poly_off[total_gt] : total_gt);
    n_runs = (dry || !gt->rle_off) ? 0 : (size_t)gt->rle_off[total_gt];
    AMP_REQUIRE(dry || n_polys <= c.max_gt, "amp_model_forward_losses: %d polygons exceed cfg.max_gt", n_polys);
    AMP_ALLOC_TO(d_poly_off, int, (size_t)std::max(n_polys, total_gt) + 1);
    AMP_ALLOC_TO(d_inst_poly_off, int, (size_t)total_gt + 1);
    AMP_ALLOC_TO(d_poly_xy, double, (size_t)std::max(npoly, 1));
    AMP_ALLOC_TO(d_rle_off, unsigned long long, (size_t)total_gt + 1);
    AMP_ALLOC_TO(d_rle_hw, int, (size_t)std::max(total_gt, 1) * 2);
    AMP_ALLOC_TO(match_val, float, (size_t)B * A);
    AMP_ALLOC_TO(match_idx, int, (size_t)B * A);
    AMP_ALLOC_TO(gt_best, unsigned int, (size_t)std::max(total_gt, 1));
    AMP_ALLOC_TO(label, signed char, (size_t)B * A);
    AMP_ALLOC_TO(keys, uint32_t, (size_t)B * A);
    AMP_ALLOC_TO(rpn_sampled, int, (size_t)B * c.rpn_batch);
    AMP_ALLOC_TO(rpn_counts, int, (size_t)B * 2);
    AMP_ALLOC_TO(rpn_partial, float, (size_t)B * 2);
    if (backward) {
        for (int l = 0; l < 5; ++l) {
            AMP_ALLOC(dp, float, (size_t)B * T.fh[l] * T.fw[l] * T.lv.ld);
            d_rpn_pred[l] = dp;
            if (!dry) AMP_HIP_CHECK(hipMemsetAsync(dp, 0, (size_t)B * T.fh[l] * T.fw[l] * T.lv.ld * 4, ctx->stream));
        }
    }
    if (dry) return AMP_OK;
    AMP_HIP_CHECK(hipMemcpyAsync(d_gt_off, gt->gt_off, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    AMP_HIP_CHECK(hipMemcpyAsync(d_poly_off, gt->poly_off, (size_t)(n_polys + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (gt->inst_poly_off) AMP_HIP_CHECK(hipMemcpyAsync(d_inst_poly_off, gt->inst_poly_off, (size_t)(total_gt + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (gt->rle_off) {
        AMP_REQUIRE(gt->rle_counts && gt->rle_hw, "amp_model_forward_losses: amp_gt.rle_off without rle_counts / rle_hw");
        AMP_HIP_CHECK(hipMemcpyAsync(d_rle_off, gt->rle_off, (size_t)(total_gt + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (total_gt) AMP_HIP_CHECK(hipMemcpyAsync(d_rle_hw, gt->rle_hw, (size_t)total_gt * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    if (total_gt) {
        AMP_HIP_CHECK(hipMemcpyAsync(d_gt_boxes, gt->boxes, (size_t)total_gt * 16, hipMemcpyHostToDevice, ctx->stream));
        AMP_HIP_CHECK(hipMemcpyAsync(d_gt_cls, gt->classes, (size_t)total_gt * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (npoly) AMP_HIP_CHECK(hipMemcpyAsync(d_poly_xy, gt->poly_xy, (size_t)npoly * 8, hipMemcpyHostToDevice, ctx->stream));
    AMP_TRY(amp_anchor_labels(ctx, &T.lv, B, d_gt_boxes, d_gt_off, total_gt, c.rpn_iou_lo, c.rpn_iou_hi, match_val, match_idx, gt_best, label));
    AMP_TRY(amp_rpn_sample_loss_ex(ctx, &T.lv, backward ? d_rpn_pred : nullptr, B, d_gt_boxes, d_gt_off, label, match_idx, keys, c.rpn_batch, c.rpn_pos_max, seed,
                                   rpn_sampled, rpn_counts, rpn_partial, &m->loss_opts));
    tap(m, "rpn_label", label, 3, {B, A});
    tap(m, "rpn_match_idx", match_idx, 1, {B, A});
    tap(m, "rpn_sampled", rpn_sampled, 1, {B, c.rpn_batch});
    tap(m, "rpn_counts", rpn_counts, 1, {B, 2});
    return AMP_OK;
}

// Proposals (training top-k), GT appended, matched and sampled; the box head; the sample's counts to the host; the box losses.
int TrainStep::box_head() {
    AMP_TRY(run_proposals(m, T, B, H, W, c.pre_nms_topk_train, c.post_nms_topk_train, PR));
    const int ncap = c.post_nms_topk_train + c.max_gt;
    AMP_ALLOC_TO(rkeys, uint32_t, (size_t)B * ncap);
    AMP_ALLOC_TO(rcls_s, int, (size_t)B * ncap);
    AMP_ALLOC_TO(rgti_s, int, (size_t)B * ncap);
    AMP_ALLOC_TO(rois, float, (size_t)B * RB * 4);
    AMP_ALLOC_TO(roi_cls, int, (size_t)B * RB);
    AMP_ALLOC_TO(roi_gti, int, (size_t)B * RB);
    AMP_ALLOC_TO(roi_counts, int, (size_t)B * 2);
    AMP_ALLOC_TO(roi_batch_idx, int, (size_t)R);
    AMP_ALLOC_TO(pooled, float, (size_t)R * 49 * 256);
    AMP_ALLOC_TO(fc1, float, (size_t)R * 1024);
    AMP_ALLOC_TO(fc2, float, (size_t)R * 1024);
    AMP_ALLOC_TO(box_pred, float, (size_t)R * ld_box);
    AMP_ALLOC_TO(box_partial, float, (size_t)B * 2);
    if (backward) { AMP_ALLOC(dbp, float, (size_t)R * ld_box); d_box_pred = dbp; }
    h_counts.assign(2 * B, 0);
    fg_off.assign(B + 1, 0);
    N = dry ? B * c.roi_fg_max : 0;       // the plan sizes the mask rows with the sampler's own cap
    if (dry) return AMP_OK;
    AMP_TRY(amp_roi_sample(ctx, B, PR.boxes, PR.count, PR.Rcap, d_gt_boxes, d_gt_cls, d_gt_off, K, RB, c.roi_fg_max, c.roi_iou, seed, rkeys,
                           rcls_s, rgti_s, ncap, rois, roi_cls, roi_gti, roi_counts, PR.anchor, A));
    std::vector<int> iota(R);
    for (int i = 0; i < R; ++i) iota[i] = i / RB;
    AMP_HIP_CHECK(hipMemcpyAsync(roi_batch_idx, iota.data(), (size_t)R * 4, hipMemcpyHostToDevice, ctx->stream));
    AMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // iota is a temporary
    const bool HS = plan.HS;
    AMP_TRY(amp::roi_align_run(ctx, &T.ff, rois, roi_batch_idx, nullptr, R, 7, pooled, nullptr, HS ? 1 : 0, T.feat_split ? 1 : 0));
    AMP_TRY(launch_conv(m, CONV("roi_heads.box_head.fc1"), pooled, 1, 1, R, 1, 0, true, 0, nullptr, 0, fc1, HS ? 1 : 0));
    AMP_TRY(launch_conv(m, CONV("roi_heads.box_head.fc2"), fc1, 1, 1, R, 1, 0, true, 0, nullptr, 0, fc2));
    AMP_TRY(launch_conv(m, CONV("roi_heads.box_predictor"), fc2, 1, 1, R, 1, 0, false, 0, nullptr, 0, box_pred));
    // counts decide the normalisers and the mask-branch sizes
    h_cls.resize(R); h_gti.resize(R);
    AMP_HIP_CHECK(hipMemcpyAsync(h_counts.data(), roi_counts, (size_t)2 * B * 4, hipMemcpyDeviceToHost, ctx->stream));
    AMP_HIP_CHECK(hipMemcpyAsync(h_cls.data(), roi_cls, (size_t)R * 4, hipMemcpyDeviceToHost, ctx->stream));
    AMP_HIP_CHECK(hipMemcpyAsync(h_gti.data(), roi_gti, (size_t)R * 4, hipMemcpyDeviceToHost, ctx->stream));
    AMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    tap(m, "train_rois", rois, 0, {B, RB, 4});
    tap(m, "train_roi_cls", roi_cls, 1, {B, RB});
    tap(m, "train_roi_gti", roi_gti, 1, {B, RB});
    tap(m, "train_roi_counts", roi_counts, 1, {B, 2});
    tap(m, "train_box_pred", box_pred, 0, {R, ld_box});
    for (int b = 0; b < B; ++b) { total_rois += h_counts[2 * b] + h_counts[2 * b + 1]; fg_off[b + 1] = fg_off[b] + h_counts[2 * b]; }
    N = fg_off[B];
    return amp_box_loss_ex(ctx, B, RB, K, box_pred, ld_box, d_box_pred, rois, roi_cls, roi_gti, d_gt_boxes, d_gt_off, c.bbox_reg_weights, total_rois,
                           box_partial, &m->loss_opts);
}

// The mask branch's buffers, on the foreground RoIs (the first nfg of every image's sample).
int TrainStep::mask_buffers() {
    Nc = std::max(N, 1);
    AMP_ALLOC_TO(m_rois, float, (size_t)Nc * 4);
    AMP_ALLOC_TO(m_batch, int, (size_t)Nc);
    AMP_ALLOC_TO(m_cls, int, (size_t)Nc);
    AMP_ALLOC_TO(m_poly, int, (size_t)Nc);
    AMP_ALLOC_TO(mpooled, float, (size_t)Nc * 196 * 256);
    AMP_ALLOC_TO(mt_a, float, (size_t)Nc * 196 * 256);
    AMP_ALLOC_TO(mt_b, float, (size_t)Nc * 784 * 256);
    AMP_ALLOC_TO(mlogits, float, (size_t)Nc * 784 * Kp);
    AMP_ALLOC_TO(m_partial, float, (size_t)Nc);
    AMP_ALLOC_TO(m_targets, unsigned char, (size_t)Nc * 784);
    macts[0] = mpooled; macts[1] = mt_a; macts[2] = mpooled; macts[3] = mt_a; macts[4] = mpooled;
    if (backward) {
        for (int i = 1; i <= 4; ++i) { AMP_ALLOC(ma, float, (size_t)Nc * 196 * 256); macts[i] = ma; }
        AMP_ALLOC(dml, float, (size_t)Nc * 784 * Kp);
        d_mlogits = dml;
    }
    return AMP_OK;
}

// bitmask ground truth: BitMasks.crop_and_resize from the run lengths.  The runs travel in a buffer of their own (their
// size is data-dependent: not part of the workspace plan), the window bit maps in a scratch of <= 256 frame-sized slots.
int TrainStep::mask_targets_bitmask() {
    const int Hp = (H + 31) / 32 * 32, Wp = (W + 31) / 32 * 32;
    for (int i = 0; i < total_gt; ++i)
        AMP_REQUIRE(gt->rle_off[i + 1] == gt->rle_off[i] || (gt->rle_hw[2 * i] >= 1 && gt->rle_hw[2 * i] <= Hp && gt->rle_hw[2 * i + 1] >= 1 && gt->rle_hw[2 * i + 1] <= Wp),
                    "amp_model_forward_losses: the bitmask of instance %d is %dx%d, the frame %dx%d", i, gt->rle_hw[2 * i], gt->rle_hw[2 * i + 1], Hp, Wp);
    const size_t slot = (size_t)Wp * (Hp / 32 + 1);
    const int nslots = std::min(N, 256);
    const size_t need = slot * nslots + (n_runs + 63) / 64 * 64;
    if (m->bm_words < need) {
        AMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (m->bm_scratch) AMP_HIP_CHECK(hipFree(m->bm_scratch));
        m->bm_scratch = nullptr; m->bm_words = 0;
        AMP_HIP_CHECK(hipMalloc(&m->bm_scratch, need * sizeof(unsigned int)));
        m->bm_words = need;
    }
    if (!m->bm_flag) { AMP_HIP_CHECK(hipMalloc(&m->bm_flag, sizeof(int))); AMP_HIP_CHECK(hipMemsetAsync(m->bm_flag, 0, sizeof(int), ctx->stream)); }
    unsigned int* d_runs = m->bm_scratch + slot * nslots;
    AMP_HIP_CHECK(hipMemcpyAsync(d_runs, gt->rle_counts, n_runs * sizeof(unsigned int), hipMemcpyHostToDevice, ctx->stream));
    return amp_mask_targets_bitmask(ctx, N, m_rois, m_poly, d_rle_off, d_runs, d_rle_hw, m->bm_scratch, slot, nslots, m_targets, m->bm_flag);
}

// The foreground RoIs' list, the plan's third part, the mask head and its loss.
int TrainStep::mask_head() {
    h_mpart.assign(N, 0.f);
    if (N <= 0 || dry) return AMP_OK;
    std::vector<int> hb(N), hc(N), hp(N);
    for (int b = 0; b < B; ++b) {
        const int nb = fg_off[b + 1] - fg_off[b];
        if (!nb) continue;
        AMP_HIP_CHECK(hipMemcpyAsync(m_rois + (size_t)fg_off[b] * 4, rois + (size_t)b * RB * 4, (size_t)nb * 16, hipMemcpyDeviceToDevice, ctx->stream));
        for (int i = 0; i < nb; ++i) {
            hb[fg_off[b] + i] = b;
            hc[fg_off[b] + i] = h_cls[b * RB + i];
            hp[fg_off[b] + i] = gt->gt_off[b] + h_gti[b * RB + i];
        }
    }
    AMP_HIP_CHECK(hipMemcpyAsync(m_batch, hb.data(), (size_t)N * 4, hipMemcpyHostToDevice, ctx->stream));
    AMP_HIP_CHECK(hipMemcpyAsync(m_cls, hc.data(), (size_t)N * 4, hipMemcpyHostToDevice, ctx->stream));
    AMP_HIP_CHECK(hipMemcpyAsync(m_poly, hp.data(), (size_t)N * 4, hipMemcpyHostToDevice, ctx->stream));
    AMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // hb/hc/hp are temporaries
    in.N = N; in.Kp = Kp;
    in.fcn_split = has_split({"roi_heads.mask_head.mask_fcn1", "roi_heads.mask_head.mask_fcn2", "roi_heads.mask_head.mask_fcn3", "roi_heads.mask_head.mask_fcn4"});
    in.deconv_split = has_split({"roi_heads.mask_head.deconv"});
    in.predictor_split = has_split({"roi_heads.mask_head.predictor"});
    train_plan_counts(in, g_tsw, &plan);
    const bool MS = plan.MS, MT = plan.MT, DS = plan.DS;
    AMP_TRY(amp::roi_align_run(ctx, &T.ff, m_rois, m_batch, nullptr, N, 14, mpooled, nullptr, MS ? 1 : 0, T.feat_split ? 1 : 0));
    for (int i = 1; i <= 4; ++i) {
        const std::string key = "roi_heads.mask_head.mask_fcn" + std::to_string(i);
        AMP_TRY(launch_conv(m, CONV(key.c_str()), macts[i - 1], N, 14, 14, 1, 1, true, 0, nullptr, 0, macts[i], MS ? ((i < 4 || MT) ? 3 : 1) : 0));
    }
    AMP_TRY(launch_conv(m, CONV("roi_heads.mask_head.deconv"), macts[4], N, 14, 14, 1, 0, true, 0, nullptr, 1, mt_b, MT ? (DS ? 3 : 1) : 0));
    AMP_TRY(launch_conv(m, CONV("roi_heads.mask_head.predictor"), mt_b, N, 28, 28, 1, 0, false, 0, nullptr, 0, mlogits, DS ? 1 : 0));
    if (n_runs) AMP_TRY(mask_targets_bitmask());
    AMP_TRY(amp_mask_target_loss_fmt(ctx, N, Kp, mlogits, d_mlogits, m_rois, m_cls, m_poly, d_poly_xy, d_poly_off, gt->inst_poly_off ? d_inst_poly_off : nullptr,
                                     n_runs ? d_rle_off : nullptr, m_targets, m_partial, m_targets));
    AMP_HIP_CHECK(hipMemcpyAsync(h_mpart.data(), m_partial, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (n_runs) AMP_HIP_CHECK(hipMemcpyAsync(&bm_overflow, m->bm_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    tap(m, "train_mask_targets", m_targets, 4, {N, 28, 28});
    tap(m, "train_mask_logits", mlogits, 0, {N, 28, 28, Kp});
    return AMP_OK;
}

// The partial sums to the host; the five losses, normalised and weighted.
int TrainStep::read_losses() {
    if (dry) return AMP_OK;
    std::vector<float> h_rpn(2 * B), h_box(2 * B);
    AMP_HIP_CHECK(hipMemcpyAsync(h_rpn.data(), rpn_partial, (size_t)2 * B * 4, hipMemcpyDeviceToHost, ctx->stream));
    AMP_HIP_CHECK(hipMemcpyAsync(h_box.data(), box_partial, (size_t)2 * B * 4, hipMemcpyDeviceToHost, ctx->stream));
    AMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    AMP_REQUIRE(!bm_overflow, "amp_model_forward_losses: a bitmask window did not fit its scratch slot (internal sizing error)");
    float s_bce = 0.f, s_loc = 0.f, s_ce = 0.f, s_l1 = 0.f, s_mask = 0.f;
    for (int b = 0; b < B; ++b) { s_bce += h_rpn[2 * b]; s_loc += h_rpn[2 * b + 1]; s_ce += h_box[2 * b]; s_l1 += h_box[2 * b + 1]; }
    for (int i = 0; i < N; ++i) s_mask += h_mpart[i];
    const float rpn_norm = (float)(c.rpn_batch * B);
    losses[0] = total_rois ? s_ce / (float)total_rois : 0.f;
    const amp_loss_opts& lo = m->loss_opts;      // the weights as detectron2 applies them (x 1.0f by default: the same bits)
    losses[1] = s_l1 / (float)std::max(total_rois, 1) * lo.box_bbox_reg_loss_weight;
    losses[2] = N ? s_mask / ((float)N * 784.f) : 0.f;
    losses[3] = s_bce / rpn_norm * lo.rpn_loss_weight;
    losses[4] = s_loc / rpn_norm * (lo.rpn_loss_weight * lo.rpn_bbox_reg_loss_weight);
    return AMP_OK;
}

// =============================================== backward ===============================================
// Gradients of the five losses (weighted as amp_model_set_loss_opts says: the loss kernels' gradients carry the weights) w.r.t. every
// trainable parameter, into m->garena (same offsets as the parameters).  Stem and res2 are frozen (FREEZE_AT = 2), FrozenBN has no parameters; its scale is folded into the weight
// transforms (data gradients) and the wgrad reduce (weight gradients).
struct Backward {
    static constexpr size_t WG_SCRATCH = (size_t)64 << 20;     // floats: split-K slabs of the largest layer
    static constexpr size_t WT_SCRATCH = (size_t)13 << 20;     // floats: transformed weights of the largest layer (fc1: 12.85 M)
    struct AsyncScope {          // every exit from the backward pass joins the side stream and leaves the context in the plain mode
        amp_ctx* c; bool on;
        ~AsyncScope() { if (on) (void)amp::wgrad_async_end(c); }
    };

    TrainStep& s;
    amp_model* m; amp_ctx* ctx; Bump& ws; const bool dry; const amp_model_cfg& c; const TrainPlan& plan; const Trunk& T; const int B;
    const bool AS;                       // the trunk's saved activations are in the split row format
    AsyncScope async_scope;
    float* wg_scratch = nullptr; float* wt_scratch = nullptr; float* wg_scratch1 = nullptr; float* cs_scratch = nullptr; float* dys_scratch = nullptr;
    size_t DYS_SCRATCH = 0;              // floats: the largest dy converted to a scaled split operand (p2 level)
    const float* dys_of = nullptr;       // the dy tensor whose scaled split copy dys_scratch currently holds
    long long dys_rows = 0;
    float* d_feat[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // gradient buffers of the FPN outputs p2..p6
    int dfeat_init = 1;                  // handed to the first RoIAlign backward, 0 afterwards
    int fstr[4] = {4, 8, 16, 32};
    float* d_res[4] = {nullptr, nullptr, nullptr, nullptr};   // gradients w.r.t. res3..res5 outputs (index = stage)
    float* dcur = nullptr;               // the block chain's running gradient (Backward::block)
    bool dcur_masked = false;            // ... already times the ReLU mask of the block it enters

    explicit Backward(TrainStep& s_) : s(s_), m(s_.m), ctx(s_.ctx), ws(s_.ws), dry(s_.dry), c(s_.c), plan(s_.plan), T(s_.T), B(s_.B), AS(s_.plan.AS), async_scope{s_.ctx, false} {}
    const ConvW& CONV(const char* key) const { return m->conv.at(key); }
    float* GW(const ConvW& cw) const { return m->garena + (cw.w - m->parena); }
    float* GB(const ConvW& cw) const { return m->garena + (cw.shift - m->parena); }
    void forget_dys() { dys_of = nullptr; }      // a scaled split copy is only trusted right after the weight gradient that made it

    int bgrad(const ConvW& cw, const float* dy, long long M_, bool acc) { return amp_colsum(ctx, dy, (int)M_, cw.cout, cs_scratch, GB(cw), acc ? 1 : 0); }
    int wgrad(const ConvW& cw, const float* x, int B_, int H_, int W_, int stride, int pad, const float* dy, bool acc, bool bias = false, int xfmt = 0);
    const float* dgrad_wsplit(const ConvW& cw, int B_, int Hy, int Wy) const {
        return dgrad_takes_wsplit(plan.dgrad_batch, cw.wt_split != nullptr, (long long)B_ * Hy * Wy, cw.cout, cw.kh, cw.kw, cw.cin) ? cw.wt_split : nullptr;
    }
    int dgrad(const ConvW& cw, const float* dy, int B_, int Hy, int Wy, int fwd_pad, const float* res, const float* mask, float* dx, bool mask_split = false);
    int dgrad_s(const ConvW& cw, const float* dy_s, int B_, int Hy, int Wy, int fwd_pad, const float* res_s, const float* mask_s, float* dx_s);

    int begin();
    int mask_head();
    int box_head();
    int rpn_head();
    int rpn_level_dense(int l);
    int fpn();
    int reserve_blocks();
    int block(int bi);
    int conv2_plain(const amp_model::BlockAct& ba, const ConvW& c2, int st2, int h1, int w1, float* d_t2, float* d_t2_up, float* d_t1);
    int conv2_gx(const amp_model::BlockAct& ba, const ConvW& c2, int st2, int h1, int w1, float* d_t2, float* d_t2_up, float* d_t1);
    int projection_tail(const amp_model::BlockAct& ba, const ConvW& c1, const ConvW& cs, int st1, int h1, int w1, const float* d_t1);
    int end();
};

// weight gradient; bias = true: the bias gradient (column sums of dy) as well -- summed on the side by the AMP_CONV_F16X3 kernel from the
// dy tiles it stages anyway, by a separate amp_colsum pass over dy on the fp32 MFMA.  xfmt: 1 = x split, 2 = dy split and scaled by 2^16
int Backward::wgrad(const ConvW& cw, const float* x, int B_, int H_, int W_, int stride, int pad, const float* dy, bool acc, bool bias, int xfmt) {
    amp_conv_desc d;
    d.B = B_; d.H = H_; d.W = W_; d.Cin = cw.cin; d.Cout = cw.cout; d.KH = cw.kh; d.KW = cw.kw; d.stride = stride; d.pad = pad;
    d.relu = 0; d.res_mode = 0; d.out_mode = 0;
    AMP_REQUIRE(amp_conv_wgrad_scratch_floats(&d) <= WG_SCRATCH, "backward: wgrad scratch too small");
    forget_dys();
    const long long Mo = (long long)B_ * ((H_ + 2 * pad - cw.kh) / stride + 1) * ((W_ + 2 * pad - cw.kw) / stride + 1);
    const WgradRoute route = wgrad_route(g_tsw, ctx->conv_mode, plan.GSW, bias, xfmt, cw.cout, cw.cin, cw.kh, cw.kw, Mo, DYS_SCRATCH);
    if (route.convert) {
        AMP_TRY(amp_colsum_split(ctx, dy, (int)Mo, cw.cout, cs_scratch, GB(cw), acc ? 1 : 0, dys_scratch, 16));
        dys_of = dy; dys_rows = Mo;                 // the data-gradient convolution of the same dy can stage this copy (dgrad below)
        return amp_conv2d_wgrad_fmt(ctx, &d, x, dys_scratch, cw.scale, wg_scratch, GW(cw), acc ? 1 : 0, 16, 0, 3, nullptr, 0);
    }
    // AMP_CONV_F16X3 splits dy * 2^16 like the data gradients below (ignored on the fp32 MFMA)
    AMP_TRY(amp_conv2d_wgrad_fmt(ctx, &d, x, dy, cw.scale, wg_scratch, GW(cw), acc ? 1 : 0, 16, 0, xfmt, route.fused ? GB(cw) : nullptr, acc ? 1 : 0));
    if (bias && !route.fused) {
        const int Ho_ = (H_ + 2 * pad - cw.kh) / stride + 1, Wo_ = (W_ + 2 * pad - cw.kw) / stride + 1;
        return bgrad(cw, dy, (long long)B_ * Ho_ * Wo_, acc);
    }
    return AMP_OK;
}

// dx = conv(dy, flipped/transposed/scaled w) (+ res) (* mask>0); dy is [B_,Hy,Wy,cw.cout]
int Backward::dgrad(const ConvW& cw, const float* dy, int B_, int Hy, int Wy, int fwd_pad, const float* res, const float* mask, float* dx, bool mask_split) {
    AMP_REQUIRE((size_t)cw.cout * cw.kh * cw.kw * cw.cin <= WT_SCRATCH, "backward: weight-transform scratch too small");
    const float* wsp = dgrad_wsplit(cw, B_, Hy, Wy);
    const float* wt = wsp ? cw.w : wt_scratch;        // with a split copy the fp32 pointer is not read
    if (!wsp) AMP_TRY(amp_dgrad_weights(ctx, cw.w, cw.scale, cw.cout, cw.kh, cw.kw, cw.cin, wt_scratch));
    amp_conv_desc d;
    d.B = B_; d.H = Hy; d.W = Wy; d.Cin = cw.cout; d.Cout = cw.cin; d.KH = cw.kh; d.KW = cw.kw; d.stride = 1; d.pad = cw.kh - 1 - fwd_pad;
    d.relu = 0; d.res_mode = res ? 1 : 0; d.out_mode = 0;
    // data gradient on the context's arithmetic; AMP_CONV_F16X3 splits dy * 2^16 (gradients of 1e-9..1e-4 would sit in the f16
    // subnormals) -- unless the weight gradient of the same dy has just left that very tensor in dys_scratch: then the ring kernel stages
    // it as it is and undoes the 2^16 in its fold
    const int fmt = (mask && mask_split) ? 8 : 0;
    if (dy_reuse_allowed(g_tsw, dy == dys_of, dys_rows, (long long)B_ * Hy * Wy) &&
        amp::conv_kernel_for(ctx->conv_mode, d, 1, 1 | fmt, 16, res != nullptr, mask != nullptr) == amp::ConvKernel::SPLIT_128x256)      // only the ring kernel undoes the 2^16
        return amp::conv_run(ctx, &d, 1, dys_scratch, wt, wsp, 0, nullptr, nullptr, res, mask, dx, 16, 1 | fmt);
    return amp::conv_run(ctx, &d, 1, dy, wt, wsp, 0, nullptr, nullptr, res, mask, dx, 16, fmt);
}

// the same on SCALED SPLIT gradients (chains GS / GX, the mask tail): dy, residual, ReLU mask and dx are split rows, dy and dx times 2^16
int Backward::dgrad_s(const ConvW& cw, const float* dy_s, int B_, int Hy, int Wy, int fwd_pad, const float* res_s, const float* mask_s, float* dx_s) {
    AMP_REQUIRE((size_t)cw.cout * cw.kh * cw.kw * cw.cin <= WT_SCRATCH, "backward: weight-transform scratch too small");
    const float* wsp = dgrad_wsplit(cw, B_, Hy, Wy);
    if (!wsp) AMP_TRY(amp_dgrad_weights(ctx, cw.w, cw.scale, cw.cout, cw.kh, cw.kw, cw.cin, wt_scratch));
    amp_conv_desc d;
    d.B = B_; d.H = Hy; d.W = Wy; d.Cin = cw.cout; d.Cout = cw.cin; d.KH = cw.kh; d.KW = cw.kw; d.stride = 1; d.pad = cw.kh - 1 - fwd_pad;
    d.relu = 0; d.res_mode = res_s ? 1 : 0; d.out_mode = 0;
    return amp::conv_run(ctx, &d, 1, dy_s, wsp ? cw.w : wt_scratch, wsp, 0, nullptr, nullptr, res_s, mask_s, dx_s, 0, 1 | 2 | (res_s ? 4 : 0) | (mask_s ? 8 : 0));
}

// The scratch buffers, the side stream of the slab reductions, the gradient buffers of p2..p6.
int Backward::begin() {
    if (!dry) AMP_TRY(amp::comm_wait_done(ctx));    // a previous exchange of this arena (a step without sgd_step, a re-run) must have finished
    if (!dry) { m->issued_mask = 0; m->grads_valid = false; }
    AMP_ALLOC_TO(wg_scratch, float, WG_SCRATCH);
    AMP_ALLOC_TO(wt_scratch, float, WT_SCRATCH);
    // The slab reductions (69 launches of ~20 us between MFMA kernels) run on a second stream behind an event (amp::wgrad_async_*), with
    // a second scratch so that the next layer's kernel does not wait for the previous layer's reduction.  AMP_ASYNC_REDUCE=0: on the main stream.
    AMP_ALLOC_TO(wg_scratch1, float, plan.async_on ? WG_SCRATCH : 64);
    if (!dry && plan.async_on) { AMP_TRY(amp::wgrad_async_begin(ctx, wg_scratch1)); async_scope.on = true; }
    AMP_ALLOC_TO(cs_scratch, float, (size_t)4 << 20);   // ceil(M/512) * N floats of the largest bias-gradient reduction
    DYS_SCRATCH = (size_t)B * T.fh[0] * T.fw[0] * 256;
    AMP_ALLOC_TO(dys_scratch, float, DYS_SCRATCH);
    if (!dry) m->last_chain = plan.last_chain;      // which backbone chain runs (amp_debug_last_backward_chain)
    for (int l = 0; l < 5; ++l) {
        AMP_ALLOC(df, float, (size_t)B * T.fh[l] * T.fw[l] * 256);
        d_feat[l] = df;
        // p2..p5: the first RoIAlign backward below writes every cell (amp::roi_align_bwd_run, init): no zero fill of 1.3 GB at B = 16; p6 has no pooler
        if (!dry && l == 4) AMP_HIP_CHECK(hipMemsetAsync(df, 0, (size_t)B * T.fh[l] * T.fw[l] * 256 * 4, ctx->stream));
    }
    return AMP_OK;
}

int Backward::mask_head() {
    const int N = s.N, Nc = s.Nc, K = s.K, Kp = s.Kp;
    float* const* macts = s.macts;
    float* mt_b = s.mt_b;
    float* d_mlogits = s.d_mlogits;
    AMP_ALLOC(d_mtb, float, (size_t)Nc * 784 * 256);
    AMP_ALLOC(d_ma, float, (size_t)Nc * 196 * 256);
    AMP_ALLOC(d_mb, float, (size_t)Nc * 196 * 256);
    AMP_ALLOC(dwd_t, float, (size_t)256 * 4 * 256);
    AMP_ALLOC(dbd_t, float, 256);
    if (dry) return AMP_OK;
    if (N <= 0) {      // no foreground RoI: the mask head's gradients are zero
        for (const char* key : {"roi_heads.mask_head.predictor", "roi_heads.mask_head.deconv", "roi_heads.mask_head.mask_fcn1", "roi_heads.mask_head.mask_fcn2",
                                "roi_heads.mask_head.mask_fcn3", "roi_heads.mask_head.mask_fcn4"}) {
            const ConvW& cw = CONV(key);
            AMP_HIP_CHECK(hipMemsetAsync(GW(cw), 0, (size_t)cw.cout * cw.kh * cw.kw * cw.cin * 4, ctx->stream));
            AMP_HIP_CHECK(hipMemsetAsync(GB(cw), 0, (size_t)cw.cout * 4, ctx->stream));
        }
        return AMP_OK;
    }
    const ConvW& cp = CONV("roi_heads.mask_head.predictor");
    const bool MS = plan.MS, MT = plan.MT, DS = plan.DS;
    AMP_TRY(wgrad(cp, mt_b, N, 28, 28, 1, 0, d_mlogits, false, true, DS ? 1 : 0));
    if (DS) AMP_TRY(amp_small_k_dgrad_split_ld(ctx, d_mlogits, Kp, K, cp.w, 256, mt_b, d_mtb, N * 784, 16, cs_scratch, dbd_t, 0));    // + the deconv's bias sums
    else if (MT) AMP_TRY(amp_small_k_dgrad_split_f32act(ctx, d_mlogits, Kp, K, cp.w, 256, mt_b, d_mtb, N * 784, 16, cs_scratch, dbd_t, 0));
    else AMP_TRY(amp_small_k_dgrad(ctx, d_mlogits, Kp, K, cp.w, 256, mt_b, d_mtb, (size_t)N * 784));
    const ConvW& cd = CONV("roi_heads.mask_head.deconv");
    {   // weight gradient in [ci][tap][co] form, then transposed into the forward layout [(tap,co)][ci]
        amp_conv_desc d;
        d.B = N; d.H = 28; d.W = 28; d.Cin = 256; d.Cout = 256; d.KH = 2; d.KW = 2; d.stride = 2; d.pad = 0; d.relu = 0; d.res_mode = 0; d.out_mode = 0;
        AMP_REQUIRE(amp_conv_wgrad_scratch_floats(&d) <= WG_SCRATCH, "backward: wgrad scratch too small");
        // here the gradient is the 'x' operand (MT: both operands split rows, the 2^16 sits in x and is undone like a dy shift)
        if (MT) AMP_TRY(amp_conv2d_wgrad_fmt(ctx, &d, d_mtb, macts[4], nullptr, wg_scratch, dwd_t, 0, 16, 0, 3, nullptr, 0));
        else AMP_TRY(amp_conv2d_wgrad_scaled(ctx, &d, d_mtb, macts[4], nullptr, wg_scratch, dwd_t, 0, 0, 16));
        AMP_TRY(amp::wgrad_async_join(ctx));      // dwd_t is read right away
        AMP_TRY(amp_deconv_grad_transpose(ctx, dwd_t, GW(cd), 256, 4, 256, 0));
        if (!MT) AMP_TRY(amp_colsum(ctx, d_mtb, N * 784, 256, cs_scratch, dbd_t, 0));
        for (int q = 0; q < 4; ++q) AMP_HIP_CHECK(hipMemcpyAsync(GB(cd) + q * 256, dbd_t, 256 * 4, hipMemcpyDeviceToDevice, ctx->stream));
        // data gradient: a 2x2 stride-2 convolution of d_mtb with w[ci][ky][kx][co], masked by fcn4's ReLU
        const float* wsp = (cd.scale == nullptr && cd.cout == 1024 && cd.cin == 256) ? dgrad_wsplit(cd, N, 28, 28) : nullptr;   // [ci][(tap, co)] = the 2x2 window rows
        if (!wsp) AMP_TRY(amp_dgrad_weights(ctx, cd.w, nullptr, 1024, 1, 1, 256, wt_scratch));
        amp_conv_desc g;
        g.B = N; g.H = 28; g.W = 28; g.Cin = 256; g.Cout = 256; g.KH = 2; g.KW = 2; g.stride = 2; g.pad = 0; g.relu = 0; g.res_mode = 0; g.out_mode = 0;
        // MT: the data gradient leaves the mask head's chain in the scaled split domain (the 2^16 rides on): fcn4..fcn1 below take d * 2^16 as
        // split rows straight from the producing convolution's epilogue -- no fp32 tensor, no conversion pass
        if (MT) AMP_TRY(amp::conv_run(ctx, &g, 1, d_mtb, wsp ? cd.w : wt_scratch, wsp, 0, nullptr, nullptr, nullptr, macts[4], d_ma, 0, 1 | 2 | 8));
        else AMP_TRY(amp::conv_run(ctx, &g, 1, d_mtb, wsp ? cd.w : wt_scratch, wsp, 0, nullptr, nullptr, nullptr, macts[4], d_ma, 16, 0));
    }
    float* dcur_m = d_ma;
    float* dnext = d_mb;
    for (int i = 4; i >= 1; --i) {
        const std::string key = "roi_heads.mask_head.mask_fcn" + std::to_string(i);
        const ConvW& cf = CONV(key.c_str());
        if (MT) {
            // bias gradient: column sums of the split rows (read-only: half the bytes of the converting pass); weight gradient on both split
            // operands; data gradient split -> split with fcn(i-1)'s split rows as the ReLU mask, the last one (no mask) back to fp32 for RoIAlign
            AMP_TRY(amp_colsum_of_split(ctx, dcur_m, N * 196, 256, cs_scratch, GB(cf), 0, 16));
            AMP_TRY(wgrad(cf, macts[i - 1], N, 14, 14, 1, 1, dcur_m, false, false, 3));
            if (i > 1) {
                AMP_TRY(dgrad_s(cf, dcur_m, N, 14, 14, 1, nullptr, macts[i - 1], dnext));
            } else {
                AMP_REQUIRE((size_t)cf.cout * cf.kh * cf.kw * cf.cin <= WT_SCRATCH, "backward: weight-transform scratch too small");
                const float* wsp1 = dgrad_wsplit(cf, N, 14, 14);
                if (!wsp1) AMP_TRY(amp_dgrad_weights(ctx, cf.w, cf.scale, cf.cout, cf.kh, cf.kw, cf.cin, wt_scratch));
                amp_conv_desc d1;
                d1.B = N; d1.H = 14; d1.W = 14; d1.Cin = cf.cout; d1.Cout = cf.cin; d1.KH = cf.kh; d1.KW = cf.kw; d1.stride = 1; d1.pad = cf.kh - 1 - 1;
                d1.relu = 0; d1.res_mode = 0; d1.out_mode = 0;
                AMP_TRY(amp::conv_run(ctx, &d1, 1, dcur_m, wsp1 ? cf.w : wt_scratch, wsp1, 0, nullptr, nullptr, nullptr, nullptr, dnext, 16, 1));
            }
        } else {
            AMP_TRY(wgrad(cf, macts[i - 1], N, 14, 14, 1, 1, dcur_m, false, true, MS));
            AMP_TRY(dgrad(cf, dcur_m, N, 14, 14, 1, nullptr, i > 1 ? macts[i - 1] : nullptr, dnext, MS));
        }
        std::swap(dcur_m, dnext);
    }
    AMP_TRY(amp::roi_align_bwd_run(ctx, d_feat, T.fh, T.fw, fstr, 256, s.m_rois, s.m_batch, N, 14, dcur_m, B, dfeat_init));
    dfeat_init = 0;
    return AMP_OK;
}

int Backward::box_head() {
    const int R = s.R;
    AMP_ALLOC(d_fc2, float, (size_t)R * 1024);
    AMP_ALLOC(d_fc1, float, (size_t)R * 1024);
    AMP_ALLOC(d_pooled, float, (size_t)R * 49 * 256);
    if (dry) return AMP_OK;
    const ConvW& cb = CONV("roi_heads.box_predictor");
    AMP_TRY(wgrad(cb, s.fc2, 1, 1, R, 1, 0, s.d_box_pred, false, true));
    AMP_TRY(dgrad(cb, s.d_box_pred, 1, 1, R, 0, nullptr, s.fc2, d_fc2));
    const ConvW& c2 = CONV("roi_heads.box_head.fc2");
    AMP_TRY(wgrad(c2, s.fc1, 1, 1, R, 1, 0, d_fc2, false, true));
    AMP_TRY(dgrad(c2, d_fc2, 1, 1, R, 0, nullptr, s.fc1, d_fc1));
    const ConvW& c1 = CONV("roi_heads.box_head.fc1");
    AMP_TRY(wgrad(c1, s.pooled, 1, 1, R, 1, 0, d_fc1, false, true, plan.HS));      // (HS: the pooled tensor is split)
    AMP_TRY(dgrad(c1, d_fc1, 1, 1, R, 0, nullptr, nullptr, d_pooled));
    AMP_TRY(amp::roi_align_bwd_run(ctx, d_feat, T.fh, T.fw, fstr, 256, s.rois, s.roi_batch_idx, R, 7, d_pooled, B, dfeat_init));
    dfeat_init = 0;
    return AMP_OK;
}

// RPN head (shared weights: gradients accumulate over the 5 levels).
// The losses touch <= RPN.BATCH_SIZE_PER_IMAGE anchors per image: the head's gradients over those pixels only (rpn_sparse.hip), all levels in one list --
// or (plan.SR false) the dense pass, level by level.
int Backward::rpn_head() {
    const int SRR = B * c.rpn_batch;
    AMP_ALLOC(sr_rows, unsigned int, (size_t)SRR);
    AMP_ALLOC(sr_nrows, int, (size_t)B);
    AMP_ALLOC(sr_dpred, float, (size_t)SRR * amp::rpn_ld(m->rpn_A));
    AMP_ALLOC(sr_act, float, (size_t)SRR * 256);
    AMP_ALLOC(sr_dt, float, (size_t)SRR * 256);
    AMP_ALLOC(sr_xg, float, (size_t)SRR * 2304);
    const size_t sr_G_floats = std::max((size_t)SRR * 2304, amp::rpn_sparse_sums_floats(amp::rpn_ld(m->rpn_A)));      // G, and the head sums' partials before it
    AMP_ALLOC(sr_G, float, sr_G_floats);
    AMP_ALLOC(sr_wt, float, (size_t)2304 * 256);
    const bool SR = !dry && plan.SR;
    if (!dry) {
        const ConvW& cpred = CONV("proposal_generator.rpn_head.pred");
        const ConvW& cconv = CONV("proposal_generator.rpn_head.conv");
        bool rpn_fused_lvl = false;
        for (int l = 0; l < 5; ++l) rpn_fused_lvl = rpn_fused_lvl || m->rpn_t[l] == nullptr;
        AMP_REQUIRE(SR || !rpn_fused_lvl, "%s", "backward: the RPN head's hidden tensor was not saved and the sparse backward pass does not apply");
        if (SR) {
            amp::RpnSparseArgs sa;
            sa.B = B; sa.batch = c.rpn_batch; sa.ld = T.lv.ld; sa.K = cpred.cout; sa.C = 256; sa.A = T.lv.A;
            for (int l = 0; l < 5; ++l) {
                sa.fh[l] = T.fh[l]; sa.fw[l] = T.fw[l];
                sa.dpred[l] = s.d_rpn_pred[l]; sa.t[l] = m->rpn_t[l]; sa.feat[l] = T.feat[l]; sa.dfeat[l] = d_feat[l];
            }
            sa.sampled = s.rpn_sampled; sa.counts = s.rpn_counts;
            sa.t_split = AS ? 1 : 0; sa.feat_split = AS ? 1 : 0;
            // recompute the hidden rows only when run_trunk really fused the head (it saved no t for some level), from split weights only while they
            // are fresh (AMP_NO_TRAIN_NATIVE does not refresh them after an SGD step: null = split per call)
            sa.recompute_t = rpn_fused_lvl ? 1 : 0; sa.w_conv_split = m->split_stale ? nullptr : cconv.w_split; sa.conv_shift = cconv.shift;
            sa.w_pred = cpred.w; sa.w_conv = cconv.w; sa.conv_scale = cconv.scale;
            sa.gw_pred = GW(cpred); sa.gb_pred = GB(cpred); sa.gw_conv = GW(cconv); sa.gb_conv = GB(cconv);
            sa.rows = sr_rows; sa.nrows = sr_nrows; sa.dpred_rows = sr_dpred; sa.act_rows = sr_act; sa.dt_rows = sr_dt; sa.xg = sr_xg; sa.G = sr_G; sa.G_floats = sr_G_floats; sa.wt = sr_wt;
            sa.wg_scratch = wg_scratch; sa.wg_scratch_floats = WG_SCRATCH;
            AMP_TRY(amp::rpn_sparse_backward(ctx, sa));
            forget_dys();
        }
        m->last_rpn_sparse = SR ? 1 : 0;
    }
    for (int l = 0; l < 5; ++l) AMP_TRY(rpn_level_dense(l));
    return AMP_OK;
}

// one level of the dense pass (its d_t buffer is reserved on the sparse route too: one workspace plan for both)
int Backward::rpn_level_dense(int l) {
    AMP_ALLOC(d_t, float, (size_t)B * T.fh[l] * T.fw[l] * 256);
    if (dry || plan.SR) return AMP_OK;
    const ConvW& cpred = CONV("proposal_generator.rpn_head.pred");
    const ConvW& cconv = CONV("proposal_generator.rpn_head.conv");
    AMP_TRY(wgrad(cpred, m->rpn_t[l], B, T.fh[l], T.fw[l], 1, 0, s.d_rpn_pred[l], l > 0, true, AS));
    const long long Ml = (long long)B * T.fh[l] * T.fw[l];
    if (rpn_level_split(g_tsw, plan.GSW, Ml, DYS_SCRATCH, cpred.scale != nullptr, T.lv.ld, cpred.cout, cconv.cout)) {
        AMP_TRY(amp_small_k_dgrad_split(ctx, s.d_rpn_pred[l], cpred.cout, cpred.w, 256, m->rpn_t[l], dys_scratch, (int)Ml, 16, cs_scratch, GB(cconv), l > 0 ? 1 : 0));
        amp_conv_desc dd;
        dd.B = B; dd.H = T.fh[l]; dd.W = T.fw[l]; dd.Cin = cconv.cin; dd.Cout = cconv.cout; dd.KH = cconv.kh; dd.KW = cconv.kw; dd.stride = 1; dd.pad = 1;
        dd.relu = 0; dd.res_mode = 0; dd.out_mode = 0;
        AMP_REQUIRE(amp_conv_wgrad_scratch_floats(&dd) <= WG_SCRATCH, "backward: wgrad scratch too small");
        AMP_TRY(amp_conv2d_wgrad_fmt(ctx, &dd, T.feat[l], dys_scratch, cconv.scale, wg_scratch, GW(cconv), l > 0 ? 1 : 0, 16, 0, 3, nullptr, 0));
        dys_of = d_t; dys_rows = Ml;             // (d_t itself stays unwritten: its only reader below takes the split copy)
    } else {
        AMP_TRY(dgrad(cpred, s.d_rpn_pred[l], B, T.fh[l], T.fw[l], 0, nullptr, m->rpn_t[l], d_t, AS));
        AMP_TRY(wgrad(cconv, T.feat[l], B, T.fh[l], T.fw[l], 1, 1, d_t, l > 0, true, AS));
    }
    return dgrad(cconv, d_t, B, T.fh[l], T.fw[l], 1, d_feat[l], nullptr, d_feat[l]);   // accumulate in place
}

int Backward::fpn() {
    if (!dry) AMP_TRY(amp_subsample2_bwd(ctx, d_feat[4], d_feat[3], B, T.fh[3], T.fw[3], 256));    // p6 = p5[::2, ::2]
    float* d_lat_prev = nullptr;                              // 2x2 sums of the finer level's lateral gradient
    for (int l = 2; l <= 5; ++l) {
        const int s_ = l - 2;
        const int fh_ = T.fh[s_], fw_ = T.fw[s_];
        AMP_ALLOC(d_lat, float, (size_t)B * fh_ * fw_ * 256);
        float* d_lat_next = nullptr;
        if (l < 5) { AMP_ALLOC(dln, float, (size_t)B * T.fh[s_ + 1] * T.fw[s_ + 1] * 256); d_lat_next = dln; }
        if (l >= 3) { AMP_ALLOC(dr, float, (size_t)B * fh_ * fw_ * kOut[s_]); d_res[s_] = dr; }
        if (dry) { d_lat_prev = d_lat_next; continue; }
        const std::string ln = "backbone.fpn_lateral" + std::to_string(l), on = "backbone.fpn_output" + std::to_string(l);
        const ConvW& co = CONV(on.c_str());
        const ConvW& cl = CONV(ln.c_str());
        AMP_TRY(wgrad(co, m->lat[s_], B, fh_, fw_, 1, 1, d_feat[s_], false, true, AS));
        AMP_TRY(dgrad(co, d_feat[s_], B, fh_, fw_, 1, d_lat_prev, nullptr, d_lat));      // + top-down share from the finer level
        if (l < 5) {
            AMP_TRY(amp::upsample2_bwd_run(ctx, d_lat, d_lat_next, B, T.fh[s_ + 1], T.fw[s_ + 1], 256, 1));      // first writer: no zero fill
        }
        const float* res_in = nullptr;   // input of the lateral conv = output of stage s_
        for (auto& ba : m->blocks) if (ba.stage == s_) res_in = ba.out;
        AMP_TRY(wgrad(cl, res_in, B, fh_, fw_, 1, 0, d_lat, false, true, AS));
        if (l >= 3) AMP_TRY(dgrad(cl, d_lat, B, fh_, fw_, 0, nullptr, nullptr, d_res[s_]));
        d_lat_prev = d_lat_next;
    }
    return AMP_OK;
}

// dry run: reserve the worst-case gradient buffers of every trainable block (kept by hand in step with Backward::block)
int Backward::reserve_blocks() {
    int hh = ((s.H + 31) / 32 * 32) / 4, ww = ((s.W + 31) / 32 * 32) / 4;
    for (int s_ = 1; s_ < 4; ++s_) {
        hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1;
        { AMP_ALLOC(r0, float, (size_t)B * hh * ww * kOut[s_]); (void)r0; }     // the stage's entry gradient as a scaled split tensor
        for (int b_ = 0; b_ < m->nblk[s_]; ++b_) {
            AMP_ALLOC(r1, float, (size_t)B * hh * ww * m->mid[s_]);
            AMP_ALLOC(r2, float, (size_t)B * hh * ww * m->mid[s_]);
            AMP_ALLOC(r3, float, (size_t)B * hh * ww * kOut[s_]);
            AMP_ALLOC(r4, float, (size_t)B * hh * ww * kOut[s_]);
            (void)r1; (void)r2; (void)r3; (void)r4;
            if (m->cfg.num_groups > 1) {     // ResNeXt on the split trunk: conv2's input decoded to fp32 for the grouped weight gradient (at the block's INPUT resolution in its first block)
                const int up = (b_ == 0 && !c.stride_in_1x1) ? 2 : 1;
                AMP_ALLOC(r5, float, (size_t)B * (hh * up) * (ww * up) * m->mid[s_]);
                AMP_ALLOC(r6, float, (size_t)B * hh * ww * m->mid[s_]);          // ... and its output gradient (the scaled split chain)
                (void)r5; (void)r6;
            }
        }
    }
    return AMP_OK;
}

// conv2's two gradients on fp32 gradients (chains 0 and 1): dense, or grouped (ResNeXt: window layout, grouped_bwd.hip)
int Backward::conv2_plain(const amp_model::BlockAct& ba, const ConvW& c2, int st2, int h1, int w1, float* d_t2, float* d_t2_up, float* d_t1) {
    const float* dy2 = d_t2;
    if (st2 == 2) {
        AMP_HIP_CHECK(hipMemsetAsync(d_t2_up, 0, (size_t)B * h1 * w1 * ba.mid * 4, ctx->stream));
        AMP_TRY(amp_subsample2_bwd(ctx, d_t2, d_t2_up, B, h1, w1, ba.mid));
        dy2 = d_t2_up;
    } else {
        AMP_REQUIRE(st2 == 1, "backward: conv2 with stride %d", st2);
    }
    if (c2.groups > 1) {
        amp_conv_desc dw;
        dw.B = B; dw.H = h1; dw.W = w1; dw.Cin = ba.mid; dw.Cout = ba.mid; dw.KH = 3; dw.KW = 3; dw.stride = st2; dw.pad = 1; dw.relu = 0; dw.res_mode = 0; dw.out_mode = 0;
        AMP_REQUIRE(amp_grouped_wgrad_scratch_floats(&dw) <= WG_SCRATCH && (size_t)ba.mid * 9 * 64 <= WT_SCRATCH, "backward: grouped scratch too small");
        AMP_TRY(amp::wgrad_async_join(ctx));      // the grouped kernels use wg_scratch on the main stream: no reduction may still be reading it
        // t1 is split on the native trunk.  grouped_wgrad_kernel can decode it on the load (amp_conv2d_grouped_wgrad_fmt, fmt 1), but its
        // loop is bound by load issue and the two 2-byte loads + converts per value DOUBLE its time (6.6 -> 13.0 ms per X-101 step at
        // B = 4 / 1024^2, measured); one decoding pass into a scratch (read 4 B, write 4 B per value: ~0.05 ms per layer) and the fp32 form is cheaper
        const float* t1f = ba.t1;
        if (AS) {
            AMP_ALLOC(t1_dec, float, (size_t)B * h1 * w1 * ba.mid);
            AMP_TRY(amp_unsplit_rows(ctx, ba.t1, (long long)B * h1 * w1, ba.mid, t1_dec));
            t1f = t1_dec;
        }
        AMP_TRY(amp_conv2d_grouped_wgrad(ctx, &dw, c2.groups, t1f, d_t2, c2.scale, wg_scratch, GW(c2)));
        AMP_TRY(amp_group_dgrad_weights(ctx, c2.w, c2.scale, ba.mid, 3, 3, wt_scratch));
        amp_conv_desc dd = dw;
        dd.stride = 1;
        forget_dys();
        return amp::conv_run(ctx, &dd, c2.groups, dy2, wt_scratch, nullptr, 0, nullptr, nullptr, nullptr, ba.t1, d_t1, 16, AS ? 8 : 0);      // (the ReLU mask t1 likewise)
    }
    AMP_TRY(wgrad(c2, ba.t1, B, h1, w1, st2, 1, d_t2, false, false, AS));
    return dgrad(c2, dy2, B, h1, w1, 1, nullptr, ba.t1, d_t1, AS);
}

// conv2's two gradients on chain GX (ResNeXt: grouped, the block's stride in it): the weight gradient on decoded operands (the 2^16 undone by its
// reduce pass), the data gradient = the grouped FORWARD kernel on transposed windows, split in / split out with t1 as the ReLU mask (a stride-2
// layer: dy's rows scattered into a zeroed map first)
int Backward::conv2_gx(const amp_model::BlockAct& ba, const ConvW& c2, int st2, int h1, int w1, float* d_t2, float* d_t2_up, float* d_t1) {
    amp_conv_desc dw;
    dw.B = B; dw.H = h1; dw.W = w1; dw.Cin = ba.mid; dw.Cout = ba.mid; dw.KH = 3; dw.KW = 3; dw.stride = st2; dw.pad = 1; dw.relu = 0; dw.res_mode = 0; dw.out_mode = 0;
    AMP_REQUIRE(amp_grouped_wgrad_scratch_floats(&dw) <= WG_SCRATCH && (size_t)ba.mid * 9 * 64 <= WT_SCRATCH, "backward: grouped scratch too small");
    AMP_REQUIRE(st2 == 1 || st2 == 2, "backward: conv2 with stride %d", st2);
    AMP_ALLOC(t1_dec, float, (size_t)B * h1 * w1 * ba.mid);
    AMP_TRY(amp_unsplit_rows(ctx, ba.t1, (long long)B * h1 * w1, ba.mid, t1_dec));      // x is read nine times per pixel: decoded once; dy once: decoded on the load
    AMP_TRY(amp::wgrad_async_join(ctx));      // the grouped kernels use wg_scratch on the main stream
    if (gx_dy_pass(g_tsw)) {
        AMP_ALLOC(dt2_dec, float, (size_t)B * ba.oh * ba.ow * ba.mid);
        AMP_TRY(amp_unsplit_rows(ctx, d_t2, (long long)B * ba.oh * ba.ow, ba.mid, dt2_dec));
        AMP_TRY(amp_conv2d_grouped_wgrad_fmt(ctx, &dw, c2.groups, t1_dec, dt2_dec, c2.scale, wg_scratch, GW(c2), 0, 16));
    } else {
        AMP_TRY(amp_conv2d_grouped_wgrad_fmt(ctx, &dw, c2.groups, t1_dec, d_t2, c2.scale, wg_scratch, GW(c2), 2, 16));
    }
    AMP_TRY(amp_group_dgrad_weights(ctx, c2.w, c2.scale, ba.mid, 3, 3, wt_scratch));
    const float* dy2 = d_t2;
    if (st2 == 2) { AMP_TRY(amp_scatter2_rows(ctx, d_t2, d_t2_up, B, h1, w1, ba.mid)); dy2 = d_t2_up; }
    amp_conv_desc dd = dw;
    dd.stride = 1;
    forget_dys();
    return amp::conv_run(ctx, &dd, c2.groups, dy2, wt_scratch, nullptr, 0, nullptr, nullptr, nullptr, ba.t1, d_t1, 0, 1 | 2 | 8);
}

// A stage's first block (projection shortcut), when the stage below is trained: the shortcut's and conv1's data gradients join the stage-exit map
// d_res[stage - 1] (fp32, input resolution: it already holds the FPN lateral's share).  Per chain.
int Backward::projection_tail(const amp_model::BlockAct& ba, const ConvW& c1, const ConvW& cs, int st1, int h1, int w1, const float* d_t1) {
    float* dprev = d_res[ba.stage - 1];
    if (plan.GS) {
        AMP_ALLOC(tmp_sc, float, (size_t)B * ba.oh * ba.ow * ba.cin);
        AMP_ALLOC(tmp_in, float, (size_t)B * ba.oh * ba.ow * ba.cin);
        AMP_TRY(dgrad_s(cs, dcur, B, ba.oh, ba.ow, 0, nullptr, nullptr, tmp_sc));
        AMP_TRY(dgrad_s(c1, d_t1, B, ba.oh, ba.ow, 0, tmp_sc, nullptr, tmp_in));
        if (ba.stride == 2) return amp_subsample2_bwd_split(ctx, tmp_in, dprev, B, ba.in_h, ba.in_w, ba.cin, 16);
        amp::set_error("backward: stride-1 projection block is not expected here");
        return AMP_ERR_STATE;
    }
    if (plan.GX) {
        // conv1's data gradient lives at the INPUT resolution and joins the fp32 stage-exit map there
        if (ba.stride != 2 || st1 != 1) { amp::set_error("backward: a ResNeXt projection block with stride %d / %d is not expected here", ba.stride, st1); return AMP_ERR_STATE; }
        AMP_ALLOC(tmp_sc, float, (size_t)B * ba.oh * ba.ow * ba.cin);
        AMP_ALLOC(tmp_full, float, (size_t)B * ba.in_h * ba.in_w * ba.cin);
        AMP_TRY(dgrad_s(cs, dcur, B, ba.oh, ba.ow, 0, nullptr, nullptr, tmp_sc));
        AMP_TRY(dgrad_s(c1, d_t1, B, h1, w1, 0, nullptr, nullptr, tmp_full));
        AMP_TRY(amp_accumulate_split(ctx, tmp_full, dprev, (long long)B * ba.in_h * ba.in_w, ba.cin, 16));
        return amp_subsample2_bwd_split(ctx, tmp_sc, dprev, B, ba.in_h, ba.in_w, ba.cin, 16);
    }
    AMP_ALLOC(tmp_sc, float, (size_t)B * ba.oh * ba.ow * ba.cin);
    AMP_TRY(dgrad(cs, dcur, B, ba.oh, ba.ow, 0, nullptr, nullptr, tmp_sc));
    if (ba.stride != 2) { amp::set_error("backward: stride-1 projection block is not expected here"); return AMP_ERR_STATE; }
    if (st1 == 2) {     // both branches at the block's output resolution: add, then spread over the input map
        AMP_ALLOC(tmp_in, float, (size_t)B * ba.oh * ba.ow * ba.cin);
        AMP_TRY(dgrad(c1, d_t1, B, ba.oh, ba.ow, 0, tmp_sc, nullptr, tmp_in));
        return amp_subsample2_bwd(ctx, tmp_in, dprev, B, ba.in_h, ba.in_w, ba.cin);
    }
    // conv1 ran at the input resolution: its data gradient joins dprev there; the strided shortcut's is spread
    AMP_ALLOC(tmp_full, float, (size_t)B * ba.in_h * ba.in_w * ba.cin);
    AMP_TRY(dgrad(c1, d_t1, B, h1, w1, 0, dprev, nullptr, tmp_full));
    AMP_HIP_CHECK(hipMemcpyAsync(dprev, tmp_full, (size_t)B * ba.in_h * ba.in_w * ba.cin * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return amp_subsample2_bwd(ctx, tmp_sc, dprev, B, ba.in_h, ba.in_w, ba.cin);
}

// One bottleneck block of res5 .. res3 (run_train walks them in reverse order), on one of three chains:
//   plain  fp32 gradients (chain 0: fp32 activations, chain 1: split activations)
//   GS     every gradient of the chain is a scaled split tensor (see dgrad_s): R50 / R101
//   GX     the same for ResNeXt: conv3 / conv1 / shortcut exactly as GS, conv2 grouped (conv2_gx)
// The stage-entry conversion, conv3's two gradients, conv1's weight gradient and the identity-shortcut tail are the same code for all three; conv2's
// gradients and the projection block's tail differ.
int Backward::block(int bi) {
    const amp_model::BlockAct& ba = m->blocks[bi];
    const int nblk = (int)m->blocks.size();
    const bool last_of_stage = (bi + 1 == nblk) || m->blocks[bi + 1].stage != ba.stage;
    if (last_of_stage) {
        // gradient from the FPN lateral; the next stage's first block (if any) has already added its share into d_res
        dcur = d_res[ba.stage];
        dcur_masked = false;
    }
    const size_t out_elems = (size_t)B * ba.oh * ba.ow * ba.cout;
    const ConvW& c3 = CONV((ba.key + ".conv3").c_str());
    const ConvW& c2 = CONV((ba.key + ".conv2").c_str());
    const ConvW& c1 = CONV((ba.key + ".conv1").c_str());
    // RESNETS.STRIDE_IN_1X1: the block's stride sits in conv1 (MSRA R50 / R101) or in the 3x3 conv2 (ResNeXt); t1 is conv1's output
    const int st1 = c.stride_in_1x1 ? ba.stride : 1, st2 = c.stride_in_1x1 ? 1 : ba.stride;
    const int h1 = (ba.in_h - 1) / st1 + 1, w1 = (ba.in_w - 1) / st1 + 1;
    AMP_ALLOC(d_t2, float, (size_t)B * ba.oh * ba.ow * ba.mid);
    AMP_ALLOC(d_t1, float, (size_t)B * h1 * w1 * ba.mid);
    float* d_t2_up = nullptr;            // stride-2 conv2: dy spread over the even positions of a zeroed map, then a stride-1 data gradient
    if (st2 == 2) { AMP_ALLOC(up, float, (size_t)B * h1 * w1 * ba.mid); d_t2_up = up; }
    const bool need_dx = !(ba.stage == 1 && ba.has_sc);   // the input of res3.0 is the frozen res2 output
    const bool split = plan.GS || plan.GX;                // the chain's gradients are scaled split tensors
    const int xf = split ? 3 : (AS ? 1 : 0);              // ... and its weight gradients take them so (plain: x split on the native trunk)

    // ---- into the block: d(pre-activation) = d(out) * (out > 0); inside a stage the previous iteration's input-gradient conv has applied it already ----
    if (split) {
        if (last_of_stage) {
            AMP_ALLOC(dcur_s, float, out_elems);
            AMP_TRY(amp_relu_mask_to_split(ctx, dcur, ba.out, dcur_s, out_elems, ba.cout, 16));
            dcur = dcur_s;
        } else if (!dcur_masked) {
            amp::set_error("backward: a block whose input is not the previous block's output is not expected inside a stage");
            return AMP_ERR_STATE;
        }
    } else if (!dcur_masked) {
        AMP_TRY(AS ? amp_relu_mask_split(ctx, dcur, ba.out, out_elems, ba.cout) : amp_relu_mask(ctx, dcur, ba.out, out_elems));
    }
    dcur_masked = false;

    // ---- conv3 ----
    AMP_TRY(wgrad(c3, ba.t2, B, ba.oh, ba.ow, 1, 0, dcur, false, false, xf));
    if (split) AMP_TRY(dgrad_s(c3, dcur, B, ba.oh, ba.ow, 0, nullptr, ba.t2, d_t2));
    else AMP_TRY(dgrad(c3, dcur, B, ba.oh, ba.ow, 0, nullptr, ba.t2, d_t2, AS));

    // ---- conv2 ----
    if (plan.GS) {      // (dense 3x3, the block's stride in conv1: t1 at the output resolution)
        AMP_TRY(wgrad(c2, ba.t1, B, ba.oh, ba.ow, 1, 1, d_t2, false, false, 3));
        AMP_TRY(dgrad_s(c2, d_t2, B, ba.oh, ba.ow, 1, nullptr, ba.t1, d_t1));
    } else if (plan.GX) {
        AMP_TRY(conv2_gx(ba, c2, st2, h1, w1, d_t2, d_t2_up, d_t1));
    } else {
        AMP_TRY(conv2_plain(ba, c2, st2, h1, w1, d_t2, d_t2_up, d_t1));
    }

    // ---- conv1 and the shortcut ----
    AMP_TRY(wgrad(c1, ba.x_in, B, ba.in_h, ba.in_w, st1, 0, d_t1, false, false, xf));      // (GS: st1 is the block's stride)
    if (ba.has_sc) {
        const ConvW& cs = CONV((ba.key + ".shortcut").c_str());
        AMP_TRY(wgrad(cs, ba.x_in, B, ba.in_h, ba.in_w, ba.stride, 0, dcur, false, false, xf));
        if (need_dx) AMP_TRY(projection_tail(ba, c1, cs, st1, h1, w1, d_t1));
    } else {
        AMP_ALLOC(d_in, float, out_elems);
        // + identity shortcut, times the ReLU mask of the block below (its output IS this block's input)
        const bool fuse = bi > 0 && m->blocks[bi - 1].out == ba.x_in;
        if (split) AMP_TRY(dgrad_s(c1, d_t1, B, ba.oh, ba.ow, 0, dcur, fuse ? ba.x_in : nullptr, d_in));
        else AMP_TRY(dgrad(c1, d_t1, B, ba.oh, ba.ow, 0, dcur, fuse ? ba.x_in : nullptr, d_in, AS));
        dcur = d_in;
        dcur_masked = fuse;
    }
    if (bi == 0 || m->blocks[bi - 1].stage != ba.stage) AMP_TRY(issue_bucket(m, 7 - ba.stage));   // res5 -> 4, res4 -> 5, res3 -> 6
    return AMP_OK;
}

int Backward::end() {
    if (async_scope.on) { async_scope.on = false; AMP_TRY(amp::wgrad_async_end(ctx)); }
    if (!dry) {
        if (m->grad_overlap != 0) AMP_TRY(amp::comm_mark_producer_end(ctx));
        m->grads_valid = true;
    }
    return AMP_OK;
}

// Training-mode forward + losses, and with backward the gradients. With ws.dry nothing is launched (workspace sizing only).
int run_train(amp_model* m, const uint8_t* imgs_d, int B, int H, int W, const amp_gt* gt, unsigned int seed, float losses[5], bool backward) {
    struct ModeGuard { amp_ctx* c; int mode; ~ModeGuard() { c->conv_mode = mode; } } mode_guard{m->ctx, m->ctx->conv_mode};
    TrainStep s(m, imgs_d, B, H, W, gt, seed, losses, backward);
    AMP_TRY(s.trunk());
    AMP_TRY(s.rpn_losses());
    AMP_TRY(s.box_head());
    AMP_TRY(s.mask_buffers());
    if (s.dry && !backward) return AMP_OK;
    AMP_TRY(s.mask_head());
    AMP_TRY(s.read_losses());
    if (!backward) return AMP_OK;

    Backward bw(s);
    AMP_TRY(bw.begin());
    AMP_TRY(bw.mask_head());
    AMP_TRY(issue_bucket(m, 0));
    AMP_TRY(bw.box_head());
    AMP_TRY(issue_bucket(m, 1));
    AMP_TRY(bw.rpn_head());
    AMP_TRY(issue_bucket(m, 2));
    AMP_TRY(bw.fpn());
    AMP_TRY(issue_bucket(m, 3));
    // ResNet res5 .. res3 (reverse block order); res2 is frozen.  (a dry run saved no block: it reserves their buffers instead)
    if (s.dry) AMP_TRY(bw.reserve_blocks());
    for (int bi = (int)m->blocks.size() - 1; bi >= 0 && m->blocks[bi].stage != 0; --bi) AMP_TRY(bw.block(bi));
    return bw.end();
}

}  // namespace
