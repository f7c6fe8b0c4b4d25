// What model.hip's orchestration shares between inference and the training step (model_train.h): the layer and workspace types, amp_model itself,
// the trunk's and the proposal stage's results, and the small helpers both sides launch through.  Host code only.
// For model.hip alone (one translation unit): the helpers are not inline.
#pragma once
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "train_plan.h"

namespace {

struct ConvW {
    float* w = nullptr;      // device [Cout][KH][KW][Cin]
    float* scale = nullptr;  // device [Cout] or null
    float* shift = nullptr;  // device [Cout] or null
    int cout = 0, cin = 0, kh = 0, kw = 0;
    float* w_split = nullptr; // AMP_CONV_F16X3 operand copy of w (amp_split_weights), made at finalize; null: not eligible / out of range
    float* wt_split = nullptr; // training: split data-gradient form of w (refresh_dgrad_weights, once per step); null: not made
    float w_absmax = 0.f;    // max |w| seen at load (range check of the split copy)
    int groups = 1;          // > 1: w is the window layout [Cout][KH][KW][64] of amp_group_expand_weights (ResNeXt conv2)
};

struct NamedBuf {
    void* ptr;
    int dtype;   // 0 f32, 1 i32, 2 u64
    int ndim;
    long long shape[5];
};

struct Bump {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    bool dry = false;
    void* alloc(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        off = a + bytes;
        if (off > peak) peak = off;
        if (dry) return reinterpret_cast<void*>(a + 256);   // non-null fake
        return (off <= cap) ? base + a : nullptr;
    }
    template <class T>
    T* get(size_t n) { return reinterpret_cast<T*>(alloc(n * sizeof(T))); }
};

const char* kStage[4] = {"res2", "res3", "res4", "res5"};
const int kOut[4] = {256, 512, 1024, 2048};
const int kStride[4] = {1, 2, 2, 2};

}  // namespace

struct amp_model {
    amp_ctx* ctx = nullptr;
    amp_model_cfg cfg;
    amp_anchor_cfg anchors;              // MODEL.ANCHOR_GENERATOR.{SIZES, ASPECT_RATIOS}; n_sizes 0 = the sizes 32 .. 512 with the ratios 0.5, 1, 2
    int rpn_A = 3;                       // anchors per location; the predictor tensor holds A logit rows, 4 A delta rows and zero rows up to amp::rpn_ld(A)
    int nblk[4] = {3, 4, 6, 3};          // RESNETS.DEPTH 50 / 101
    int mid[4] = {64, 128, 256, 512};     // NUM_GROUPS * WIDTH_PER_GROUP * 2^stage
    // ---- parameters ----
    float* parena = nullptr;
    size_t parena_floats = 0, parena_used = 0;
    std::map<std::string, ConvW> conv;                     // keyed by detectron2 module prefix
    std::map<std::string, std::vector<float>> host_raw;    // raw host copies needed at finalize (BN stats, fused parts)
    std::map<std::string, bool> loaded;
    std::map<std::string, bool> raw_fresh;                 // halves of the fused predictor matrices loaded since the last amp_model_finalize
    std::vector<std::string> expected;
    bool finalized = false;
    // ---- workspace ----
    Bump ws;
    std::map<std::string, NamedBuf> taps;
    int* d_batch_iota = nullptr;        // [max_batch * post_nms_topk] roi -> image
    int* d_flags = nullptr;             // [4] overflow flags
    // pinned host staging
    int* h_counts = nullptr;            // [max_batch] (pinned)
    int* h_small = nullptr;             // pinned scratch for small uploads
    char* h_res = nullptr;              // pinned: the per-detection results of one call (one D2H copy)
    size_t h_res_bytes = 0;
    std::vector<char> host_out;         // result storage
    // host results of the last call
    std::vector<int> r_n, r_classes, r_rle_len;
    std::vector<float> r_boxes, r_scores;
    std::vector<unsigned long long> r_rle_off;
    std::vector<uint32_t> r_pool;       // (fallback when the pinned pool below could not be allocated)
    uint32_t* h_pool = nullptr;         // pinned, host-cacheable: the run lengths of one call land here by DMA and are handed out in place
    size_t h_pool_counts = 0;
    const uint32_t* r_pool_ptr = nullptr;
    int rle_mode = 0;                   // amp_model_set_rle_output: 0 run lengths, 1 counts strings (encoded on the device), 2 both
    char* h_str = nullptr;              // pinned: the counts strings of one call
    size_t h_str_bytes = 0;
    hipEvent_t ev_counts = nullptr;     // marks the arrival of the detection counts on the host (run(): the wait that is not a stream sync)
    size_t str_bytes_last = 0;      // bytes of counts strings the previous inference produced (the size of the speculative read-back)
    std::vector<unsigned long long> r_str_off;
    std::vector<int> r_str_len;
    std::vector<int> r_out_h, r_out_w;
    float last_stage_ms[8];
    // ---- training ----
    float* garena = nullptr;            // gradients, same offsets as parena
    float* varena = nullptr;            // SGD momentum buffers, same offsets
    amp_loss_opts loss_opts = {AMP_BOXLOSS_SMOOTH_L1, 0.f, 1.f, 1.f, AMP_BOXLOSS_SMOOTH_L1, 0.f, 1.f};   // amp_model_set_loss_opts (= amp_loss_opts_default)
    bool saving = false;                // run_trunk keeps every activation the backward pass needs
    bool acts_split = false;            // ... and kept them in the split row format (training on the native trunk, AMP_CONV_F16X3)
    int last_rpn_sparse = -1;           // 1: the last backward pass ran the RPN head's gradients over the sampled pixels only (rpn_sparse.hip)
    int last_chain = -1;                // the last backward pass's backbone chain: 0 fp32 storage, 1 split activations + fp32 gradients, 2 scaled split gradients (R50 / R101), 3 the same for ResNeXt blocks
    bool gs_chain_ok = false;           // ... and the backbone's backward chain can run on scaled split gradients (dense 3x3, stride in conv1: R50 / R101)
    struct BlockAct { std::string key; float *x_in, *t1, *t2, *sc, *out; int in_h, in_w, oh, ow, cin, mid, cout, stride, stage; bool has_sc; };
    std::vector<BlockAct> blocks;
    float* lat[4] = {nullptr, nullptr, nullptr, nullptr};
    float* rpn_t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool rpn_train_fused = false;       // this training step's RPN head ran with the predictors in the conv's epilogue (no hidden tensor saved): the sparse backward recomputes its rows
    struct Trainable { float* p; size_t n; };
    std::vector<Trainable> trainable;
    unsigned long long* sgd_chunks = nullptr;   // device table for amp::sgd_chunks_run, built at the first amp_model_sgd_step
    int sgd_nchunks = 0;
    amp::SgdPlan sgd_plan;                      // the general step (amp_model_sgd_step_ex): built at its first call, one tensor per state_dict entry
    bool sgd_plan_built = false;
    bool clip_stats_valid = false;              // sgd_plan.ttab holds N / k of a norm-clipped step
    int last_sgd_path = 0;                      // amp_debug_last_sgd_path: 1 sgd_chunks_kernel, 2 the general kernels
    struct JobTable { amp::WeightJob* jobs = nullptr; void* chunks = nullptr; int nchunks = 0; };
    JobTable fwd_jobs, dgrad_jobs;              // refresh_split_weights / refresh_dgrad_weights: every layer's split copy in one launch
    bool fwd_jobs_dirty = true, dgrad_jobs_dirty = true;
    float* dgrad_arena = nullptr;               // split data-gradient weights (ConvW::wt_split), AMP_CONV_F16X3 training
    size_t dgrad_floats = 0;
    bool grads_valid = false;
    float* split_arena = nullptr;       // f16x3 operand copies of the weights (inference)
    size_t split_floats = 0;
    bool split_stale = false;
    int f32_reruns = 0;                 // batches re-run in AMP_CONV_F32 after the range flag was raised
    uint8_t* img_stage = nullptr;       // device copy of host images (amp_model_infer / forward_losses with imgs_on_host), grown on demand
    size_t img_stage_bytes = 0;
    std::vector<int> img_hw;            // optional per-image valid sizes for the next batches
    // ---- gradient exchange (comm.hip): merged arena ranges per bucket, in the order the backward pass completes them ----
    std::vector<int> gb_bucket;
    std::vector<size_t> gb_off, gb_n;
    int grad_overlap = -1;              // -1: on when the context has a communicator; 0 / 1: amp_model_set_grad_overlap
    unsigned int* bm_scratch = nullptr; // window bit maps of amp_mask_targets_bitmask (bitmask ground truth), grown on demand
    size_t bm_words = 0;
    int* bm_flag = nullptr;
    unsigned issued_mask = 0;           // buckets of the current gradients already handed to RCCL (bit b); all set = exchanged
};

namespace {

// The training step's switches (train_plan.h): g_tsw_env is what the environment said when the library was loaded, g_tsw the process's one instance --
// amp_debug_set_* (model.hip) write 0 / 1 into it, or with -1 the environment's value back.
const TrainSwitches g_tsw_env;
TrainSwitches g_tsw = g_tsw_env;

int launch_conv(amp_model* m, const ConvW& cw, const float* x, int B, int H, int W, int stride, int pad, bool relu,
                int res_mode, const float* res, int out_mode, float* y, int fmt = 0) {
    amp_conv_desc d;
    d.B = B; d.H = H; d.W = W; d.Cin = cw.cin; d.Cout = cw.cout; d.KH = cw.kh; d.KW = cw.kw;
    d.stride = stride; d.pad = pad; d.relu = relu ? 1 : 0; d.res_mode = res_mode; d.out_mode = out_mode;
    // pre-split weights when the layer has them; a layer whose weights exceed the fp16 range of the split copy stays on fp32 MFMA
    const bool eligible = cw.cin % 32 == 0 || (cw.cin == 4 && cw.kw == 8);   // dense and grouped layers, the padded stem
    // (after an SGD step the split copies are stale until the next inference refreshes them: split per call then)
    return amp::conv_run(m->ctx, &d, cw.groups, x, cw.w, m->split_stale ? nullptr : cw.w_split, (eligible && !cw.w_split) ? 1 : 0, cw.scale, cw.shift, res,
                         nullptr, y, 0, fmt);
}

// Inference in AMP_CONV_F16X3: tensors that only feed convolutions travel in the split operand format (written by the producer's
// epilogue / by RoIAlign, same bytes as fp32), so their consumers stage both operands by LDS-DMA and split nothing.
bool split_chain(amp_model* m, std::initializer_list<const char*> keys) {
    if (!split_chain_allowed(g_tsw, m->ws.dry, m->ctx->conv_mode, m->split_stale)) return false;
    for (const char* k : keys) {
        auto it = m->conv.find(k);
        if (it == m->conv.end() || !it->second.w_split) return false;
    }
    return true;
}

void tap(amp_model* m, const char* name, void* p, int dtype, std::initializer_list<long long> shape) {
    NamedBuf nb;
    nb.ptr = p; nb.dtype = dtype; nb.ndim = (int)shape.size();
    int i = 0;
    for (long long s : shape) nb.shape[i++] = s;
    m->taps[name] = nb;
}

#define AMP_TRY(expr) do { int _s = (expr); if (_s != AMP_OK) return _s; } while (0)
#define AMP_ALLOC(var, T, n)                                                                  \
    T* var = ws.get<T>((size_t)(n));                                                          \
    if (!var) { amp::set_error("amp_model: workspace exhausted allocating %s (%zu bytes, cap %zu)", #var, \
                               (size_t)(n) * sizeof(T), ws.cap); return AMP_ERR_NOMEM; }

// Hand bucket b of the gradient arena to RCCL: everything the backward pass has launched so far is ordered before it, everything
// it launches from here on overlaps it.  No-op without a communicator or with the overlap switched off.
int issue_bucket(amp_model* m, int b) {
    amp_ctx* ctx = m->ctx;
    if (m->ws.dry || !ctx->comm || m->grad_overlap == 0) return AMP_OK;
    AMP_TRY(amp::wgrad_async_join(ctx));      // the bucket's last reductions may still be on the side stream
    // every range of the bucket, in groups of at most 64 per grouped RCCL call (a fragmented arena may hold more than 64)
    size_t off[64], n[64];
    int nr = 0;
    for (size_t i = 0; i < m->gb_bucket.size(); ++i) {
        if (m->gb_bucket[i] != b) continue;
        off[nr] = m->gb_off[i]; n[nr] = m->gb_n[i];
        if (++nr == 64) { AMP_TRY(amp::comm_allreduce_ranges(ctx, m->garena, off, n, nr, b)); nr = 0; }
    }
    AMP_TRY(amp::comm_allreduce_ranges(ctx, m->garena, off, n, nr, b));
    m->issued_mask |= 1u << b;
    return AMP_OK;
}

struct Trunk {
    float* feat[5];
    int fh[5], fw[5];
    amp_rpn_levels lv;
    amp_fpn_feats ff;
    int max_n;
    const int* img_hw;    // device [B][2] per-image sizes (amp_model_set_image_sizes) or null: clip / rescale with these, not the frame
    bool feat_split;      // p2..p6 are in the split row format (the trunk's native activation format in AMP_CONV_F16X3 inference)
};

struct Proposals {
    float* boxes;    // [B][Rcap][4]
    float* logits;   // [B][Rcap]
    int* count;      // [B]
    int* anchor;     // [B][Rcap] global anchor index each proposal was decoded from
    int Rcap;
};

// model.hip
int run_trunk(amp_model* m, const uint8_t* imgs_d, int B, int H, int W, Trunk& T);
int run_proposals(amp_model* m, const Trunk& T, int B, int H, int W, int k, int Rcap, Proposals& P);
int refresh_split_weights(amp_model* m);
int refresh_dgrad_weights(amp_model* m);

}  // namespace
