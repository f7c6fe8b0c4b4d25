// Convolution as implicit GEMM on the gfx950 matrix pipe: the launch table (conv_run, launch_*) and the C entry points.  One translation unit;
// every kernel family is a header of its own (DESIGN.md §4 has the table), included here at file scope, OUTSIDE the anonymous namespace below:
// nested in it, every mangled name would change.
//
// Replaces the cuDNN convolutions detectron2 runs for AMPIS:
// ResNet-50 stem+res2..res5, FPN lateral/output convs, the RPN head, the box-head FCs (as 1x1 convs over
// "pixels" = RoIs) and the mask head (3x3 convs, ConvTranspose 2x2 s2, 1x1 predictor).
//
// Which orders are part of the machine code: template kernels are emitted in the order of their first use in the host code of THIS file (the four
// launch_* functions in front of the stem launches, then the cases of conv_run's switch), wherever they are defined.  The six kernels that are not
// templates are emitted in source order, so these includes keep mask_tail.h, then conv_weights.h, then stem_pool.h:
//   mask_tail_kernel, split_weights_kernel, weight_jobs_kernel, unsplit_rows_kernel, group_expand_kernel, stem_pool_u8_kernel
#include "common.h"
#include <type_traits>
#include "lds_ring.h"
#include "conv_args.h"          // types, BK, ConvArgs, fastdiv, conv_pixel
#include "conv_epilogue.h"      // the epilogues and the f16x3 MFMA step
#include "conv_mfma.h"          // conv_mfma_kernel (fp32, register-staged)
#include "conv_glds.h"          // conv_glds_kernel (LDS-DMA; fp32, f16x3, G32)
#include "conv_predict.h"       // the fused mask-predictor and RPN tails
#include "conv_split.h"         // conv_split_kernel, g_stamp, STAMP_*
#include "mask_tail.h"          // mask_tail_kernel                                            -- order: first of the non-template kernels
#include "conv3x3_patch.h"      // conv3x3_patch_kernel
#include "conv3x3_c64.h"        // conv3x3_c64_kernel, Fuse3Args
#include "conv_f16x3.h"         // conv_f16x3_kernel, split8
#include "conv_weights.h"       // split_weights, weight_jobs, unsplit_rows, group_expand      -- order: after mask_tail.h
#include "stem_pool.h"          // stem_pool_f16x3_kernel, stem_pool_u8_kernel                 -- order: after conv_weights.h
#include "conv_nloop.h"         // conv1x1_nloop_kernel (experiment, default off)
#include "conv_plan.h"          // ConvSwitches, conv_plan (host only)

namespace {

// epi -> template argument of a launch: f(std::integral_constant<int, E>()) for the first E of E0, Es... that equals epi, for the last otherwise
template <int E0, int... Es, class F>
void with_epi(int epi, F f) {
    if (sizeof...(Es) == 0 || epi == E0) f(std::integral_constant<int, E0>());
    else if constexpr (sizeof...(Es) > 0) with_epi<Es...>(epi, f);
}
struct ConvLaunch {       // one convolution launch: the kernel's arguments behind (a, x bytes, w bytes) follow the thread count
    const ConvArgs& a; hipStream_t st; unsigned int xb, wb;
    template <class K, class... More>
    void operator()(K kernel, int threads, More... more) const { AMP_TIMED_LAUNCH(kernel, dim3(a.nblk), dim3(threads), 0, st, a, xb, wb, more...); }
};
// Four launches as functions of their own, in front of the stem launches: templates are instantiated in the order of their first use, and the
// listing has had these kernels first.
// grouped, <= 32 channels per group: one K-step per tap
void launch_f16x3s_g32(const ConvLaunch& launch, int epi) { with_epi<1, 2, 0>(epi, [&](auto E) { launch(conv_glds_kernel<64, false, E(), true, true>, 256); }); }
// the two-workgroups-per-CU form (two buffers, no ping-pong: the SIMD partner is the other workgroup's wave)
void launch_split_short(const ConvLaunch& launch, int epi) { with_epi<2, 1>(epi, [&](auto E) { launch(conv_split_kernel<128, 128, E(), 2>, 256); }); }
// Cout = 64 (res2's 3x3 and 1x1 layers): 256 x 64 tiles, four waves of 64 x 64 (one wave spans all 64 output channels: 2/3 of the LDS bytes per
// MFMA of the 128 x 64 tiles' 64 x 32 wave tiles), two buffers, two workgroups per CU
void launch_split_tall64(const ConvLaunch& launch) { launch(conv_split_kernel<256, 64, 1, 2>, 256); }
void launch_f16x3_stem(const ConvLaunch& launch, int epi) { with_epi<1, 0>(epi, [&](auto E) { launch(conv_f16x3_kernel<64, E(), true>, 256); }); }

void set_fastdiv(unsigned int d, unsigned int* mul, int* shr) {
    int l = 0;
    while ((1ull << l) < d) ++l;
    *shr = 29 + l;
    *mul = (unsigned int)(((1ull << *shr) + d - 1) / d);
}

}  // namespace

static ConvSwitches g_sw;
extern "C" void amp_debug_set_f16x3_bn256(int v) { g_sw.f16x3_bn256 = v; }
extern "C" void amp_debug_set_short_k(int v) { g_sw.short_k = v; }
extern "C" void amp_debug_set_tall64(int v) { g_sw.tall64 = v; }
extern "C" void amp_debug_set_split_ring(int v) { g_sw.split_ring = v; }
extern "C" void amp_debug_set_korder(int v) { g_sw.korder = v; }
extern "C" void amp_debug_set_patch256(int v) { g_sw.patch256 = v; }
extern "C" void amp_debug_set_nloop(int v) { g_sw.nloop = v; }
extern "C" void amp_debug_set_mask_tail_loop(int v) { g_sw.mask_tail_loop = v; }
extern "C" void amp_debug_set_patch_conv(int v) { g_sw.patch_conv = v; }
extern "C" void amp_debug_set_conv_generic_epilogue(int on) { g_sw.generic_epi = on; }
extern "C" void amp_debug_set_conv_ablate(int mode) { g_sw.ablate = mode; }
#ifdef AMP_STAMP
extern "C" int amp_debug_read_stamps(unsigned long long* out) {     // 64 values; zeroes the device counters
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    unsigned long long z[64] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
extern "C" int amp_debug_read_stamp_clock(unsigned long long* out) {     // 2 values (g_stamp_clk); zeroes the device counters
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp_clk), sizeof(unsigned long long) * 2) != hipSuccess) return -1;
    unsigned long long z[2] = {0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_clk), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

static int conv_impl(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w, const float* scale,
                     const float* shift, const float* res, const float* mask, float* y) {
    return amp::conv_run(ctx, d, groups, x, w, nullptr, 0, scale, shift, res, mask, y);
}

// w [rows][K] fp32 (K % 32 == 0) -> the operand layout of the AMP_CONV_F16X3 kernels, same byte size (rows * K * 4)
int amp::weight_jobs_run(amp_ctx* ctx, const amp::WeightJob* jobs_dev, const void* chunks_dev, int nchunks) {
    if (nchunks <= 0) return AMP_OK;
    hipLaunchKernelGGL(weight_jobs_kernel, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, jobs_dev, reinterpret_cast<const uint2*>(chunks_dev));
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

/* The split data-gradient form of one weight tensor: wt_split = split rows (amp_split_weights) of Wt[c][KH-1-ky][KW-1-kx][n] =
 * w[n][ky][kx][c] * scale[n] (amp_dgrad_weights), bit for bit, in one pass.  Cout % 32 == 0.  A training step of the model makes these
 * for all its layers in one launch (weight_jobs_kernel); this entry runs the same kernel on one tensor (it allocates its two small
 * tables per call: for tests and bindings, not for a hot loop). */
extern "C" int amp_dgrad_weights_split(amp_ctx* ctx, const float* w, const float* scale, int Cout, int KH, int KW, int Cin, float* wt_split) {
    AMP_REQUIRE(ctx && w && wt_split && Cout > 0 && KH > 0 && KW > 0 && Cin > 0 && Cout % 32 == 0, "amp_dgrad_weights_split: bad argument (Cout %% 32 != 0?)");
    amp::WeightJob job{w, scale, reinterpret_cast<unsigned int*>(wt_split), Cout, KH, KW, Cin, (Cout % 64 == 0 && Cin % 64 == 0) ? 2 : 1};
    std::vector<unsigned int> ch;
    if (job.transpose == 2) {
        const size_t ntiles = (size_t)KH * KW * (Cout / 64) * (Cin / 64);
        for (size_t t = 0; t < ntiles; ++t) { ch.push_back(0u); ch.push_back((unsigned int)t); }
    } else {
        const size_t npairs = (size_t)Cout * KH * KW * Cin / 2;
        for (size_t p0 = 0; p0 < npairs; p0 += 8192) { ch.push_back(0u); ch.push_back((unsigned int)p0); }
    }
    amp::WeightJob* d_job = nullptr;
    unsigned int* d_ch = nullptr;
    AMP_HIP_CHECK(hipMalloc(&d_job, sizeof(job)));
    if (hipMalloc(&d_ch, ch.size() * sizeof(unsigned int)) != hipSuccess) { (void)hipFree(d_job); AMP_REQUIRE(false, "amp_dgrad_weights_split: out of device memory"); }
    int st = AMP_OK;
    if (hipMemcpy(d_job, &job, sizeof(job), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_ch, ch.data(), ch.size() * sizeof(unsigned int), hipMemcpyHostToDevice) != hipSuccess) st = AMP_ERR_HIP;
    if (st == AMP_OK) st = amp::weight_jobs_run(ctx, d_job, d_ch, (int)(ch.size() / 2));
    if (st == AMP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = AMP_ERR_HIP;     // the tables are freed below
    (void)hipFree(d_job);
    (void)hipFree(d_ch);
    return st;
}

extern "C" int amp_split_weights(amp_ctx* ctx, const float* w, long long rows, int K, float* w_split) {
    AMP_REQUIRE(ctx && w && w_split && rows > 0 && K > 0 && K % 32 == 0, "amp_split_weights: bad argument (K %% 32 != 0?)");
    hipLaunchKernelGGL(split_weights_kernel, dim3(2048), dim3(256), 0, ctx->stream, w, (size_t)rows, K, reinterpret_cast<unsigned int*>(w_split));
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

// the inverse of amp_split_weights / of a producer's split output: rows of hi|lo' halves -> fp32 (hi + lo' * 2^-11, exact)
extern "C" int amp_unsplit_rows(amp_ctx* ctx, const float* x_split, long long rows, int C, float* out) {
    AMP_REQUIRE(ctx && x_split && out && rows > 0 && C > 0 && C % 32 == 0, "amp_unsplit_rows: bad argument (C %% 32 != 0?)");
    hipLaunchKernelGGL(unsplit_rows_kernel, dim3(2048), dim3(256), 0, ctx->stream, reinterpret_cast<const unsigned int*>(x_split), (size_t)rows, C, out);
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

extern "C" int amp_conv2d_nhwc_fmt(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* w, const float* scale, const float* shift,
                                   const float* res, float* y, int fmt) {
    AMP_REQUIRE(fmt >= 0 && fmt < 8, "amp_conv2d_nhwc_fmt: bad fmt");
    AMP_REQUIRE(fmt == 0 || (ctx && ctx->conv_mode == AMP_CONV_F16X3), "amp_conv2d_nhwc_fmt: split formats exist in AMP_CONV_F16X3 only");
    return amp::conv_run(ctx, d, 1, x, w, nullptr, 0, scale, shift, res, nullptr, y, 0, fmt);
}

// Stage a11, fused: x [B,H,W,256] (a pyramid level, split rows) -> 3x3 conv 256 -> 256 + bias + ReLU -> the 16 predictor rows (3 objectness
// logits, 12 anchor deltas, one zero row; w_pred [16][256], b_pred [16]) -> pred [B*H*W][16]; the hidden tensor is never written.
// The predictor rows are split here per call (the model keeps its own split copy); B*H*W >= amp::RPN_FUSE_MIN_PIXELS so that the 128 x 256 tiles fill the chip.
extern "C" int amp_rpn_head_fused(amp_ctx* ctx, const float* x_split, int B, int H, int W, const float* w_conv, const float* b_conv, const float* w_pred,
                                  const float* b_pred, float* pred) {
    return amp_rpn_head_fused_ld(ctx, x_split, B, H, W, w_conv, b_conv, w_pred, b_pred, 16, pred);
}
// ... with ld = 16, 32 or 48 predictor rows (A logits, 4 A deltas, zero rows): w_pred [ld][256], b_pred [ld] -> pred [B*H*W][ld]
extern "C" int amp_rpn_head_fused_ld(amp_ctx* ctx, const float* x_split, int B, int H, int W, const float* w_conv, const float* b_conv, const float* w_pred,
                                     const float* b_pred, int ld, float* pred) {
    AMP_REQUIRE(ctx && x_split && w_conv && b_conv && w_pred && b_pred && pred && B > 0 && H > 0 && W > 0, "amp_rpn_head_fused: bad argument");
    AMP_REQUIRE(ld == 16 || ld == 32 || ld == 48, "amp_rpn_head_fused: ld = %d, must be 16, 32 or 48", ld);
    AMP_REQUIRE(ctx->conv_mode == AMP_CONV_F16X3, "amp_rpn_head_fused: AMP_CONV_F16X3 only (the fp32 path runs the two convolutions)");
    AMP_REQUIRE((long long)B * H * W >= amp::RPN_FUSE_MIN_PIXELS, "amp_rpn_head_fused: fewer than %lld pixels: run the two convolutions (amp_conv2d_nhwc_fmt)", amp::RPN_FUSE_MIN_PIXELS);
    float* wps = nullptr;
    AMP_HIP_CHECK(hipMalloc(&wps, (size_t)ld * 256 * sizeof(float)));
    hipLaunchKernelGGL(split_weights_kernel, dim3(8), dim3(256), 0, ctx->stream, w_pred, (size_t)ld, 256, reinterpret_cast<unsigned int*>(wps));
    amp_conv_desc d;
    d.B = B; d.H = H; d.W = W; d.Cin = 256; d.Cout = 256; d.KH = 3; d.KW = 3; d.stride = 1; d.pad = 1; d.relu = 1; d.res_mode = 0; d.out_mode = 0;
    amp::RpnFuse rf{wps, b_pred, pred, ld};
    const int st = amp::conv_run(ctx, &d, 1, x_split, w_conv, nullptr, 0, nullptr, b_conv, nullptr, nullptr, pred, 0, 1, nullptr, &rf);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(wps);
    return st;
}

// Stage a16 tail, fused: x [N,14,14,256] in the split row format -> ConvTranspose2d 2x2 s2 (w_deconv [(ky,kx,co)][256], bias [1024]: the
// bias of co repeated per tap) -> ReLU -> 1x1 predictor row of classes[n] (pred_w [K][256], pred_b [K]) -> sigmoid -> prob [N,28,28]
extern "C" int amp_mask_deconv_predict(amp_ctx* ctx, const float* x_split, int N, const float* w_deconv, const float* bias, const float* pred_w,
                                       const float* pred_b, const int* classes, int K, float* prob) {
    AMP_REQUIRE(ctx && x_split && w_deconv && bias && pred_w && pred_b && classes && prob && N >= 0 && K >= 1, "amp_mask_deconv_predict: bad argument");
    AMP_REQUIRE(ctx->conv_mode == AMP_CONV_F16X3, "amp_mask_deconv_predict: AMP_CONV_F16X3 only (the fp32 path runs the three stages)");
    if (N == 0) return AMP_OK;
    amp_conv_desc d;
    d.B = N; d.H = 14; d.W = 14; d.Cin = 256; d.Cout = 1024; d.KH = 1; d.KW = 1; d.stride = 1; d.pad = 0; d.relu = 1; d.res_mode = 0; d.out_mode = 1;
    amp::PredictFuse f{pred_w, pred_b, classes, K, prob};
    return amp::conv_run(ctx, &d, 1, x_split, w_deconv, nullptr, 0, nullptr, bias, nullptr, nullptr, prob, 0, 1, &f);
}

extern "C" int amp_conv2d_nhwc_ex(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* w, const float* scale,
                                  const float* shift, const float* res, const float* mask, float* y) {
    return conv_impl(ctx, d, 1, x, w, scale, shift, res, mask, y);
}

// Grouped convolution (ResNeXt conv2: Cin == Cout, groups | Cin, channels per group in {8,16,32,64}).  The kernel is the dense
// LDS-DMA kernel with 64-wide N tiles whose K range is restricted to the tile's own 64 input channels; `w_win` is the
// block-diagonal window layout [Cout][KH][KW][64] produced by amp_group_expand_weights (zeros outside the channel's group).
extern "C" int amp_conv2d_grouped_nhwc(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w_win,
                                       const float* scale, const float* shift, const float* res, float* y) {
    AMP_REQUIRE(d && groups >= 1, "amp_conv2d_grouped_nhwc: bad argument");
    return conv_impl(ctx, d, groups, x, w_win, scale, shift, res, nullptr, y);
}

// the same with split-format tensors (AMP_CONV_F16X3; fmt as in amp_conv2d_nhwc_fmt: bit 0 x, bit 1 y, bit 2 res)
extern "C" int amp_conv2d_grouped_nhwc_fmt(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w_win,
                                           const float* scale, const float* shift, const float* res, float* y, int fmt) {
    AMP_REQUIRE(d && groups >= 1 && fmt >= 0 && fmt < 8, "amp_conv2d_grouped_nhwc_fmt: bad argument");
    AMP_REQUIRE(fmt == 0 || (ctx && ctx->conv_mode == AMP_CONV_F16X3), "amp_conv2d_grouped_nhwc_fmt: split formats exist in AMP_CONV_F16X3 only");
    return amp::conv_run(ctx, d, groups, x, w_win, nullptr, 0, scale, shift, res, nullptr, y, 0, fmt);
}

// Tests (tests/test_conv_exact_gpu.py): conv_run as the model's training step calls it -- a ReLU mask (fp32, or split rows with AMP_FMT_MASK_SPLIT),
// a scaled input (in_shift), force_f32 and weights split beforehand (w_split: amp_split_weights / amp_dgrad_weights_split of w, or null for the per-call
// split) have no entry in the public header.  No fused tail.
extern "C" int amp_debug_conv_run(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w, const float* w_split, const float* scale,
                                  const float* shift, const float* res, const float* mask, float* y, int in_shift, int fmt, int force_f32) {
    AMP_REQUIRE(d && groups >= 1 && fmt >= 0 && fmt < 16 && in_shift >= 0 && in_shift <= 24, "amp_debug_conv_run: bad argument");
    AMP_REQUIRE(fmt == 0 || (ctx && ctx->conv_mode == AMP_CONV_F16X3), "amp_debug_conv_run: split formats exist in AMP_CONV_F16X3 only");
    return amp::conv_run(ctx, d, groups, x, w, w_split, force_f32, scale, shift, res, mask, y, in_shift, fmt);
}

// w [Cout][KH][KW][cpg] (grouped OHWI) -> w_win [Cout][KH][KW][64]
extern "C" int amp_group_expand_weights(amp_ctx* ctx, const float* w, int Cout, int KH, int KW, int cpg, float* w_win) {
    AMP_REQUIRE(ctx && w && w_win && Cout > 0 && KH > 0 && KW > 0, "amp_group_expand_weights: bad argument");
    AMP_REQUIRE((cpg == 8 || cpg == 16 || cpg == 32 || cpg == 64) && Cout % 64 == 0,
                "amp_group_expand_weights: channels per group must be 8/16/32/64 and Cout a multiple of 64 (got %d, %d)", cpg, Cout);
    const size_t total = (size_t)Cout * KH * KW * 64;
    hipLaunchKernelGGL(group_expand_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, ctx->stream, w, Cout,
                       KH * KW, cpg, w_win);
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

static int g_stem_pool = getenv("AMP_NO_STEM_POOL") ? 0 : 1;      // EXPERIMENT switch: 0 = stem and pool as two kernels
extern "C" void amp_debug_set_stem_pool(int v) { g_stem_pool = v; }
// Stem (7x7 stride 2 on the [B,H,W,4] input, weights [64][7][8][4], ReLU) + max-pool 3x3 stride 2 pad 1 in one kernel: AMP_CONV_F16X3 with
// pre-split weights only.  Returns 1 (nothing launched) when the fused form does not apply -- the caller runs the two kernels.
bool amp::stem_pool_applies(amp_ctx* ctx, const float* w_split) {
    return g_stem_pool && ctx->conv_mode == AMP_CONV_F16X3 && w_split && g_sw.ablate == 0;
}
// a profiling record for the launch that follows: null outside a profile, or when the pool is used up (the profile is then marked truncated).
// variant 0 = a launch of the DOMINANT kernel (conv_split_kernel<128x256>, fp32 mode conv_glds_kernel<128>)
static amp_prof_rec* prof_open(amp_ctx* ctx, double flops, double bytes, int M, int N, int K, int variant = 1) {
    if (!ctx->prof_on) return nullptr;
    if (ctx->prof_used >= ctx->prof_pool.size()) { ctx->prof_truncated = true; return nullptr; }
    amp_prof_rec* rec = &ctx->prof_pool[ctx->prof_used++];
    rec->flops = flops; rec->variant = variant; rec->bytes = bytes; rec->M = M; rec->N = N; rec->K = K;
    return rec;
}
// the stem as the fused stem + pool kernels see it: 7x7 stride 2 pad 3 over the H x W frame of 4-channel pixels (x: null for the uint8 kernel)
static ConvArgs stem_args(amp_ctx* ctx, int B, int H, int W, const float* x, const float* w_split, const float* scale, const float* shift) {
    ConvArgs a = ConvArgs();
    a.x = x; a.w = w_split; a.scale = scale; a.shift = shift;
    a.B = B; a.H = H; a.W = W; a.Cin = 4; a.Cout = 64;
    a.KH = 7; a.KW = 8; a.stride = 2; a.pad = 3;
    a.Ho = (H + 2 * 3 - 7) / 2 + 1;
    a.Wo = (W + 2 * 3 - 7) / 2 + 1;
    a.cin_win = 4;
    a.K = 7 * 8 * 4; a.nsteps = 7;
    a.relu = 1;
    a.in_scale = a.out_scale = 1.0f;
    a.range_flag = ctx->d_conv_flag;
    return a;
}
int amp::stem_pool_run(amp_ctx* ctx, int B, int H, int W, const float* x, int x_split, const float* w_split, const float* scale, const float* shift,
                       float* pool, int pool_split) {
    if (!amp::stem_pool_applies(ctx, w_split)) return 1;
    const ConvArgs a = stem_args(ctx, B, H, W, x, w_split, scale, shift);
    const size_t x_bytes = (size_t)B * H * W * 4 * sizeof(float), w_bytes = (size_t)64 * a.K * sizeof(float);
    if (a.Ho < 1 || a.Wo < 1 || x_bytes >= (size_t)OOB_VOFF || (long long)B * H * W >= (1ll << 27)) {
        AMP_REQUIRE(!x_split, "stem_pool_run: a split input needs the fused kernel, which this size does not fit");
        return 1;
    }
    StemPoolArgs sp;
    sp.pool = pool; sp.pool_split = pool_split;
    sp.Hq = (a.Ho + 2 - 3) / 2 + 1; sp.Wq = (a.Wo + 2 - 3) / 2 + 1;
    sp.tiles_y = amp::cdiv(sp.Hq, SP_PH); sp.tiles_x = amp::cdiv(sp.Wq, SP_PW);
    // flops: useful work of the stem (as conv_run counts it), not the halo; bytes: input + weights + the pooled tensor
    amp_prof_rec* rec = prof_open(ctx, 2.0 * (double)B * a.Ho * a.Wo * 64.0 * 7.0 * 8.0 * 4.0,
                                  (double)x_bytes + (double)w_bytes + 4.0 * (double)B * sp.Hq * sp.Wq * 64.0, B * a.Ho * a.Wo, 64, 7 * 8 * 4);
    amp::ProfLaunchScope timed(rec ? rec->e0 : nullptr, rec ? rec->e1 : nullptr);      // attached to the launch below (AMP_TIMED_LAUNCH)
    if (x_split) AMP_TIMED_LAUNCH(stem_pool_f16x3_kernel<true>, dim3((unsigned)(B * sp.tiles_y * sp.tiles_x)), dim3(512), 0, ctx->stream, a, sp,
                                    (unsigned int)x_bytes, (unsigned int)w_bytes);
    else AMP_TIMED_LAUNCH(stem_pool_f16x3_kernel<false>, dim3((unsigned)(B * sp.tiles_y * sp.tiles_x)), dim3(512), 0, ctx->stream, a, sp,
                            (unsigned int)x_bytes, (unsigned int)w_bytes);
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

static int g_stem_u8 = getenv("AMP_NO_STEM_U8") ? 0 : 1;      // EXPERIMENT switch: 0 = preprocess_kernel + stem_pool_f16x3_kernel
extern "C" void amp_debug_set_stem_u8(int v) { g_stem_u8 = v; }
bool amp::stem_u8_applies(amp_ctx* ctx, const float* w_split) { return g_stem_u8 && amp::stem_pool_applies(ctx, w_split); }
// The fused stem + pool from the uint8 image (stem_pool_u8_kernel): Hp x Wp is the padded frame the convolution sees.
int amp::stem_pool_u8_run(amp_ctx* ctx, const uint8_t* img, int B, int H, int W, int Hp, int Wp, const float mean[3], const float std_[3],
                          const int* img_hw, const float* w_split, const float* scale, const float* shift, float* pool, int pool_split) {
    AMP_REQUIRE(amp::stem_u8_applies(ctx, w_split) && img && mean && std_ && pool && B > 0 && Hp >= H && Wp >= W, "stem_pool_u8_run: bad argument");
    const ConvArgs a = stem_args(ctx, B, Hp, Wp, nullptr, w_split, scale, shift);
    const size_t w_bytes = (size_t)64 * a.K * sizeof(float);
    StemPoolArgs sp;
    sp.pool = pool; sp.pool_split = pool_split;
    sp.Hq = (a.Ho + 2 - 3) / 2 + 1; sp.Wq = (a.Wo + 2 - 3) / 2 + 1;
    sp.tiles_y = amp::cdiv(sp.Hq, SP_PH); sp.tiles_x = amp::cdiv(sp.Wq, SP_PW);
    StemU8Args u;
    u.img = img; u.H = H; u.W = W; u.img_hw = img_hw;
    u.m0 = mean[0]; u.m1 = mean[1]; u.m2 = mean[2]; u.s0 = std_[0]; u.s1 = std_[1]; u.s2 = std_[2];
    // flops: useful work of the stem (as conv_run counts it), not the halo; bytes: uint8 pixels + weights + the pooled tensor
    amp_prof_rec* rec = prof_open(ctx, 2.0 * (double)B * a.Ho * a.Wo * 64.0 * 7.0 * 8.0 * 4.0,
                                  3.0 * (double)B * H * W + (double)w_bytes + 4.0 * (double)B * sp.Hq * sp.Wq * 64.0, B * a.Ho * a.Wo, 64, 7 * 8 * 4);
    amp::ProfLaunchScope timed(rec ? rec->e0 : nullptr, rec ? rec->e1 : nullptr);
    AMP_TIMED_LAUNCH(stem_pool_u8_kernel, dim3((unsigned)(B * sp.tiles_y * sp.tiles_x)), dim3(512), 0, ctx->stream, a, sp, u, (unsigned int)w_bytes);
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

extern "C" int amp_conv2d_nhwc(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* w,
                               const float* scale, const float* shift, const float* res, float* y) {
    return amp_conv2d_nhwc_ex(ctx, d, x, w, scale, shift, res, nullptr, y);
}

amp::ConvKernel amp::conv_kernel_for(int conv_mode, const amp_conv_desc& d, int groups, int fmt, int in_shift, bool res, bool mask) {
    ConvPlan p;
    return conv_plan({conv_mode, d, groups, fmt, in_shift, 0, res, mask, false, 0, 0}, g_sw, &p) == AMP_OK ? p.kernel : amp::ConvKernel::COUNT;
}

int amp::conv_run(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w, const float* w_split, int force_f32,
                  const float* scale, const float* shift, const float* res, const float* mask, float* y, int in_shift, int fmt,
                  const amp::PredictFuse* fuse, const amp::RpnFuse* rpn) {
    AMP_REQUIRE(ctx && d && x && w && y, "amp_conv2d_nhwc: null argument");
    AMP_REQUIRE(!fuse || (fuse->pred_w && fuse->pred_b && fuse->cls && fuse->prob && fuse->K >= 1), "conv: incomplete PredictFuse");
    AMP_REQUIRE(!rpn || (rpn->w_split && rpn->bias && rpn->pred), "conv: incomplete RpnFuse");
    AMP_REQUIRE(!(fuse && rpn), "conv: the fused RPN epilogue needs a split input, Cout = 256, ReLU and the ring kernel");
    ConvPlan p;
    AMP_TRY_STATUS(conv_plan({ctx->conv_mode, *d, groups, fmt, in_shift, force_f32, res != nullptr, mask != nullptr, scale != nullptr,
                              fuse ? 1 : (rpn ? 2 : 0), rpn ? rpn->ld : 0}, g_sw, &p));
    // the profiling record: useful flops; algorithmic bytes of this launch: every operand once (amp_prof_launches; a 1x1 conv reads only the pixels its stride samples)
    const double MN = (double)p.M * d->Cout;
    const double in_rows = (d->KH == 1 && d->KW == 1) ? (double)p.M : (double)d->B * d->H * d->W;
    const double out_vals = p.out_mode == 3 ? (double)p.M * 4.0 : p.out_mode == 4 ? (double)p.M * 16.0 * p.rpn_nbp : MN;
    const double res_vals = !res ? 0.0 : (d->res_mode == 2 ? MN / 4.0 : MN);
    amp_prof_rec* rec = prof_open(ctx, 2.0 * MN * (double)d->KH * (double)d->KW * (double)p.cpg,
                                  4.0 * (in_rows * d->Cin + (double)d->Cout * p.K + out_vals + res_vals + (mask ? MN : 0.0)),
                                  p.M, d->Cout, d->KH * d->KW * p.cpg, p.dominant ? 0 : 1);
    amp::ProfLaunchScope timed(rec ? rec->e0 : nullptr, rec ? rec->e1 : nullptr);      // the convolution kernel launched below carries the events
    if (p.f16x3 && !w_split) {   // per-call split into the context's scratch (stream order makes the reuse safe)
        if (ctx->split_bytes < p.w_bytes) {
            AMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            if (ctx->split_scratch) AMP_HIP_CHECK(hipFree(ctx->split_scratch));
            ctx->split_scratch = nullptr; ctx->split_bytes = 0;
            AMP_HIP_CHECK(hipMalloc(&ctx->split_scratch, p.w_bytes));
            ctx->split_bytes = p.w_bytes;
        }
        hipLaunchKernelGGL(split_weights_kernel, dim3(2048), dim3(256), 0, ctx->stream, w, (size_t)d->Cout, p.K,
                           reinterpret_cast<unsigned int*>(ctx->split_scratch));
        w_split = ctx->split_scratch;
    }
    ConvArgs a;
    a.x = x; a.w = p.f16x3 ? w_split : w; a.scale = scale; a.shift = shift; a.res = res; a.mask = mask; a.y = y;
    a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
    a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
    a.Ho = p.Ho; a.Wo = p.Wo; a.M = p.M; a.K = p.K; a.nsteps = p.nsteps;
    a.grouped = groups > 1; a.cin_win = p.cin_win;
    a.relu = d->relu; a.res_mode = d->res_mode; a.out_mode = p.out_mode;
    a.ntn = p.ntn; a.nblk = p.nblk; a.stagger = p.stagger; a.korder = p.korder; a.direct_epi = 1;
    a.in_scale = (in_shift != 0) ? ldexpf(1.0f, in_shift) : 1.0f;
    a.out_scale = (in_shift != 0) ? ldexpf(1.0f, -in_shift) : 1.0f;
    a.y_split = p.y_split; a.res_split = (fmt & 4) ? 1 : 0; a.mask_split = (fmt & 8) ? 1 : 0;
    a.range_flag = ctx->d_conv_flag;
    a.pred_w = fuse ? fuse->pred_w : nullptr; a.pred_b = fuse ? fuse->pred_b : nullptr; a.pred_cls = fuse ? fuse->cls : nullptr;
    a.pred_K = fuse ? fuse->K : 0; a.prob = fuse ? fuse->prob : nullptr;
    a.rpn_w = rpn ? rpn->w_split : nullptr; a.rpn_b = rpn ? rpn->bias : nullptr; a.rpn_pred = rpn ? rpn->pred : nullptr;
    set_fastdiv((unsigned int)(a.Ho * a.Wo), &a.div_howo_mul, &a.div_howo_shr);
    set_fastdiv((unsigned int)a.Wo, &a.div_wo_mul, &a.div_wo_shr);
    const unsigned int xb = (unsigned int)p.x_bytes, wb = (unsigned int)p.w_bytes;
    hipStream_t st = ctx->stream;
    using amp::ConvKernel;
    // (templates are instantiated in the order of their first use, depth first, so the cases stand in the order the listing has had its kernels in)
    const ConvLaunch launch{a, st, xb, wb};
    auto launch_f16x3 = [&](auto BN_) {      // activations split in the kernel; in_scale != 1: multiplied by that power of two first (SCALED)
        constexpr int BN = decltype(BN_)::value, NT_ = (BN == 256) ? 512 : 256;
        if (a.in_scale != 1.0f) with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_f16x3_kernel<BN, E(), false, true>, NT_); });
        else with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_f16x3_kernel<BN, E()>, NT_); });
    };
    switch (p.kernel) {
        case ConvKernel::C64_PATCH_DIAG: launch(conv3x3_c64_kernel<true>, 256, p.tiles_x, p.tiles_y, Fuse3Args()); break;
        case ConvKernel::C64_PATCH: launch(conv3x3_c64_kernel<false>, 256, p.tiles_x, p.tiles_y, Fuse3Args()); break;
        case ConvKernel::PATCH256: with_epi<5, 4, 3, 1>(p.epi, [&](auto E) { launch(conv3x3_patch_kernel<E()>, 512, p.tiles_x, p.tiles_y); }); break;
        case ConvKernel::MASK_TAIL: launch(mask_tail_kernel, 512); break;
        case ConvKernel::SPLIT_128x256:
            if (a.korder)      // EXPERIMENT (AMP_KORDER=1): channel-major K order
                with_epi<3, 2, 1>(p.epi, [&](auto E) { launch(conv_split_kernel<128, 256, E(), 3, true>, 512); });
            else if (p.epi >= 3 && p.epi <= 5)      // the fused tails: the mask head's, or the RPN tail with 16, 32 or 48 predictor rows
                with_epi<3, 4, 5>(p.epi, [&](auto E) { launch(conv_split_kernel<128, 256, 3, 3, false, E() - 2>, 512); });
            else
                with_epi<2, 1>(p.epi, [&](auto E) { launch(conv_split_kernel<128, 256, E()>, 512); });
            break;
        case ConvKernel::SPLIT_SHORT_128x128: launch_split_short(launch, p.epi); break;
        case ConvKernel::NLOOP_SCATTER: launch(conv1x1_nloop_kernel<true>, 512, p.nloop_nt); break;
        case ConvKernel::NLOOP: launch(conv1x1_nloop_kernel<false>, 512, p.nloop_nt); break;
        case ConvKernel::SPLIT_256x128: with_epi<2, 1>(p.epi, [&](auto E) { launch(conv_split_kernel<256, 128, E()>, 512); }); break;
        case ConvKernel::SPLIT_TALL64: launch_split_tall64(launch); break;
        case ConvKernel::F16X3S_256: with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_glds_kernel<256, false, E(), true>, 512); }); break;
        case ConvKernel::F16X3S_128: with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_glds_kernel<128, false, E(), true>, 256); }); break;
        case ConvKernel::F16X3S_G32: launch_f16x3s_g32(launch, p.epi); break;
        case ConvKernel::F16X3S_64: with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_glds_kernel<64, false, E(), true>, 256); }); break;
        case ConvKernel::F16X3_STEM: launch_f16x3_stem(launch, p.epi); break;
        case ConvKernel::F16X3_64: launch_f16x3(std::integral_constant<int, 64>()); break;
        case ConvKernel::F16X3_256: launch_f16x3(std::integral_constant<int, 256>()); break;
        case ConvKernel::F16X3_128: launch_f16x3(std::integral_constant<int, 128>()); break;
        case ConvKernel::GLDS_STEM: with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_glds_kernel<64, true, E()>, 256); }); break;
        case ConvKernel::GLDS_128: with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_glds_kernel<128, false, E()>, 256); }); break;
        case ConvKernel::GLDS_64: with_epi<1, 2, 0>(p.epi, [&](auto E) { launch(conv_glds_kernel<64, false, E()>, 256); }); break;
        case ConvKernel::MFMA_128:
            with_epi<1, 2, 3, 0>(g_sw.ablate, [&](auto ABL) { AMP_TIMED_LAUNCH((conv_mfma_kernel<128, 128, ABL()>), dim3(a.nblk), dim3(256), 0, st, a); });
            break;
        case ConvKernel::MFMA_64: AMP_TIMED_LAUNCH((conv_mfma_kernel<128, 64>), dim3(a.nblk), dim3(256), 0, st, a); break;
        case ConvKernel::COUNT: break;
    }
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

// Host-only view of conv_plan for tests/test_conv_plan.py and tools/conv_plan_table.py: no device, no context.  in: the 22 integers of ConvPlanIn in
// declaration order (mode, the 12 of amp_conv_desc, groups, fmt, in_shift, force_f32, res, mask, scale, fuse, rpn_ld); sw: the 12 switches in the
// order of ConvSwitches, or null for the process's current state.
struct amp_debug_conv_plan_out { int kernel, epi, ntn, nblk, stagger, dominant, tiles_x, tiles_y, nloop_nt, rpn_nbp; };
extern "C" int amp_debug_conv_plan(const int* in, const int* sw, amp_debug_conv_plan_out* out) {
    AMP_REQUIRE(in && out, "amp_debug_conv_plan: null argument");
    ConvPlanIn pi;
    pi.mode = in[0];
    pi.d.B = in[1]; pi.d.H = in[2]; pi.d.W = in[3]; pi.d.Cin = in[4]; pi.d.Cout = in[5]; pi.d.KH = in[6]; pi.d.KW = in[7]; pi.d.stride = in[8]; pi.d.pad = in[9];
    pi.d.relu = in[10]; pi.d.res_mode = in[11]; pi.d.out_mode = in[12];
    pi.groups = in[13]; pi.fmt = in[14]; pi.in_shift = in[15]; pi.force_f32 = in[16];
    pi.res = in[17] != 0; pi.mask = in[18] != 0; pi.scale = in[19] != 0; pi.fuse = in[20]; pi.rpn_ld = in[21];
    ConvSwitches s = g_sw;
    if (sw) {
        s.f16x3_bn256 = sw[0]; s.short_k = sw[1]; s.tall64 = sw[2]; s.split_ring = sw[3]; s.korder = sw[4]; s.patch256 = sw[5]; s.nloop = sw[6];
        s.mask_tail_loop = sw[7]; s.patch_conv = sw[8]; s.stagger = sw[9]; s.generic_epi = sw[10]; s.ablate = sw[11];
    }
    ConvPlan p;
    AMP_TRY_STATUS(conv_plan(pi, s, &p));
    *out = {(int)p.kernel, p.epi, p.ntn, p.nblk, p.stagger, p.dominant ? 1 : 0, p.tiles_x, p.tiles_y, p.nloop_nt, p.rpn_nbp};
    return AMP_OK;
}
extern "C" const char* amp_debug_conv_kernel_name(int kernel) {      // null past the last value
    static const char* const names[] = {"C64_PATCH", "C64_PATCH_DIAG", "PATCH256", "MASK_TAIL", "SPLIT_128x256", "SPLIT_SHORT_128x128", "SPLIT_256x128", "SPLIT_TALL64",
                                        "NLOOP", "NLOOP_SCATTER", "F16X3S_256", "F16X3S_128", "F16X3S_64", "F16X3S_G32", "F16X3_STEM", "F16X3_256", "F16X3_128", "F16X3_64",
                                        "GLDS_STEM", "GLDS_128", "GLDS_64", "MFMA_128", "MFMA_64"};
    static_assert(sizeof(names) / sizeof(names[0]) == (size_t)amp::ConvKernel::COUNT, "one name per ConvKernel");
    return (kernel >= 0 && kernel < (int)amp::ConvKernel::COUNT) ? names[kernel] : nullptr;
}

// conv2 (3x3, 64 -> 64, FrozenBN, ReLU) + conv3 (1x1, 64 -> C3, FrozenBN, + residual, ReLU) of a res2 bottleneck in one launch (conv3x3_c64_kernel<false, true>):
// every operand in the split row format; returns 1 when the fused kernel does not apply (the caller launches the two convolutions).
static int g_fuse23 = getenv("AMP_NO_FUSE23") ? 0 : 1;      // EXPERIMENT switch
extern "C" void amp_debug_set_fuse23(int v) { g_fuse23 = v; }
int amp::conv_c64_fused3_run(amp_ctx* ctx, int B, int H, int W, const float* x_split, const float* w2_split, const float* scale2, const float* shift2,
                             const float* w3_split, const float* scale3, const float* shift3, int C3, const float* res_split, float* y_split) {
    if (!g_fuse23 || g_sw.patch_conv == 0 || ctx->conv_mode != AMP_CONV_F16X3 || !w2_split || !w3_split) return 1;
    if (C3 % 64 != 0 || C3 > 256 || B < 1 || H < 1 || W < 1) return 1;
    const size_t x_bytes = (size_t)B * H * W * 64 * sizeof(float), w_bytes = (size_t)64 * 576 * sizeof(float), r_bytes = (size_t)B * H * W * C3 * sizeof(float);
    const long long tiles = (long long)B * amp::cdiv(H, 8) * amp::cdiv(W, 16);
    if (x_bytes >= (size_t)OOB_VOFF || r_bytes >= ((size_t)1 << 32) || (long long)B * H * W >= (1ll << 29) / 4 || !c64_patch_fills(g_sw, tiles)) return 1;
    ConvArgs a = ConvArgs();
    a.x = x_split; a.w = w2_split; a.scale = scale2; a.shift = shift2;
    a.B = B; a.H = H; a.W = W; a.Cin = 64; a.Cout = 64; a.KH = 3; a.KW = 3; a.stride = 1; a.pad = 1; a.Ho = H; a.Wo = W;
    a.M = B * H * W; a.K = 576; a.nsteps = 18; a.cin_win = 64; a.grouped = 0;
    a.relu = 1; a.in_scale = a.out_scale = 1.0f; a.y_split = 1; a.direct_epi = 1;
    a.range_flag = ctx->d_conv_flag;
    a.ntn = 1; a.nblk = (int)tiles;
    set_fastdiv((unsigned int)(a.Ho * a.Wo), &a.div_howo_mul, &a.div_howo_shr);
    set_fastdiv((unsigned int)a.Wo, &a.div_wo_mul, &a.div_wo_shr);
    Fuse3Args f3;
    f3.w3 = w3_split; f3.scale3 = scale3; f3.shift3 = shift3; f3.res = res_split; f3.y = y_split; f3.C3 = C3; f3.w3_bytes = (unsigned int)((size_t)C3 * 64 * sizeof(float));
    // bytes: input + weights + residual + output (t2 is never in memory)
    amp_prof_rec* rec = prof_open(ctx, 2.0 * (double)a.M * (64.0 * 576.0 + (double)C3 * 64.0),
                                  (double)x_bytes + (double)w_bytes + (double)f3.w3_bytes + 2.0 * (double)r_bytes, a.M, C3, 576 + 64);
    amp::ProfLaunchScope timed(rec ? rec->e0 : nullptr, rec ? rec->e1 : nullptr);
    AMP_TIMED_LAUNCH((conv3x3_c64_kernel<false, true>), dim3(a.nblk), dim3(256), 0, ctx->stream, a, (unsigned int)x_bytes, (unsigned int)w_bytes, amp::cdiv(W, 16), amp::cdiv(H, 8), f3);
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

// C-ABI of the fused block tail (tests, and a host that drives res2 itself): all tensors split rows; AMP_ERR_STATE when the kernel does not apply.
extern "C" int amp_bottleneck64_tail(amp_ctx* ctx, int B, int H, int W, const float* x_split, const float* w2_split, const float* scale2, const float* shift2,
                                     const float* w3_split, const float* scale3, const float* shift3, int C3, const float* res_split, float* y_split) {
    AMP_REQUIRE(ctx && x_split && w2_split && w3_split && res_split && y_split, "%s", "amp_bottleneck64_tail: null argument");
    const int st = amp::conv_c64_fused3_run(ctx, B, H, W, x_split, w2_split, scale2, shift2, w3_split, scale3, shift3, C3, res_split, y_split);
    if (st == 1) { amp::set_error("amp_bottleneck64_tail: the fused kernel does not apply (AMP_CONV_F16X3, C3 %% 64 == 0, C3 <= 256, >= 512 tiles of 8 x 16)"); return AMP_ERR_STATE; }
    return st;
}
