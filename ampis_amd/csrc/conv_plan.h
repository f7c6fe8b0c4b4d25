// Which kernel takes a layer: the switches, the thresholds and the pure selection function conv_plan.  Host code only: no kernel header.
// For conv.hip alone: ConvSwitches and the thresholds stand outside the anonymous namespace, as they always did, and the functions are not inline --
// a second includer would define them twice.
#pragma once
#include "common.h"
#include "lds_ring.h"      // OOB_VOFF
#include "conv_args.h"     // BK (the K-step has no smaller home: it is a constant of the kernels; nothing else of that header is used here)

// The switches conv_plan reads: one instance (g_sw), written by the amp_debug_set_* entries of conv.hip; the environment gives the initial values.
struct ConvSwitches {
    int f16x3_bn256 = 1;   // EXPERIMENT switch: 256-wide 8-wave tiles where Cout % 256 == 0
    int short_k = getenv("AMP_NO_SHORT_K") ? 0 : 1;      // EXPERIMENT switch: K <= 64 layers on 128 x 128 tiles, two workgroups per CU (0: the 128 x 256 ring tiles)
    int tall64 = getenv("AMP_TALL64") ? atoi(getenv("AMP_TALL64")) : 1;      // Cout = 64 layers on 256 x 64 tiles of conv_split_kernel, two workgroups per CU (0: the 128 x 64 ring tiles of conv_glds_kernel): res2 3x3 160 -> 145 us, 1x1 256 -> 64 148 -> 140 us, bit-identical
    int split_ring = getenv("AMP_SPLIT_RING") ? atoi(getenv("AMP_SPLIT_RING")) : 1;    // EXPERIMENT switch: the 3-buffer conv_split_kernel for pre-split inputs (0: the 2-buffer conv_glds_kernel<.., F16>)
    int korder = getenv("AMP_KORDER") ? atoi(getenv("AMP_KORDER")) : 0;     // EXPERIMENT switch: 1 = channel-major K order in conv_split_kernel (ConvArgs::korder)
    // EXPERIMENT switch, default OFF: 1 = conv3x3_patch_kernel for the wide 3x3 layers (0: conv_split_kernel<128, 256>); 2 = whatever the grid size (tests).
    // Measured (round 4, tools/lab/time_conv.py, tools/lab/pmc_p256.sh): FETCH_SIZE per launch of the FPN output conv at p2 1.97 -> 0.44 M KiB, L2 misses
    // 35.7 -> 11.2 M -- and the SAME wall time on random operands (1410-1420 us either way; the chip holds 1.85 GHz under the ring kernel's loop and
    // 1.97-2.16 GHz under this one, which needs 2230 cycles per K-step against 1970): the layer is limited by the power the MFMAs draw, not by its
    // traffic; on all-zero operands (2.4 GHz either way) the ring kernel wins by the cycle ratio, 1049 against 1124 us.  And the channel-major sums move
    // one box of the full-size gate from 0.9e-3 to 1.01e-3 px off the fp32 oracle (bare tolerance 1e-3): not adopted.
    int patch256 = getenv("AMP_PATCH256") ? atoi(getenv("AMP_PATCH256")) : 0;
    // EXPERIMENT switch, default OFF (AMP_NLOOP=1): several N tiles per workgroup for the short-K 1x1 layers (conv1x1_nloop_kernel).  Measured (round 4,
    // tools/lab/time_nloop.py, A/B in one process, bit-identical): the training step's deconv 930-970 -> 856 us, res3.0's stride-2 shortcut 315 -> 291 us at B = 16
    // and 154 -> 151 at B = 8, res4.0's shortcut 223 -> 240 us (WORSE), an inference step 16.16 against 16.12 ms: what bounds these layers is not the ring's
    // cold start (that was the mask tail's case: four taps over the SAME pixels and a store-free epilogue) but their bytes; 0.1 ms of a 74-ms training step
    // does not pay for a second loop structure on the training path.
    int nloop = getenv("AMP_NLOOP") ? atoi(getenv("AMP_NLOOP")) : 0;
    int mask_tail_loop = getenv("AMP_NO_MASK_TAIL_LOOP") ? 0 : 1;      // EXPERIMENT switch: 0 = the fused mask-head tail on conv_split_kernel<128, 256, 3> (one tap per workgroup)
    int patch_conv = getenv("AMP_NO_PATCH_CONV") ? 0 : 1;      // EXPERIMENT switch: 0 = the implicit-GEMM kernels for the 64-channel-window 3x3 layers; 2 = conv3x3_c64_kernel whatever the grid size (tests)
    int stagger = getenv("AMP_STAGGER") ? atoi(getenv("AMP_STAGGER")) : 1;      // ConvArgs::stagger (tools/stamp_conv.py)
    int generic_epi = 0;   // tests: force the generic epilogue
    int ablate = 0;        // tools/bench_conv_ablate.py: timing variants of the register-staged kernel
};

// Two thresholds that were switches once.  One round of 128 x 256 tiles (192 ... 511 of them) is taken from WIDE_NSTEPS K-steps on.  Round 4 measured the
// alternative's bound -- two 128 x 128 workgroups per CU move 64 KB per 1536 MFMA cycles through an L2 -> LDS path that gives a CU ~33 B/clk -- and 16 instead
// of 64: res4's conv1 (M = 32768, K = 1024) 54 -> 49 us, fc2 55 -> 47 us, res4.0 conv1 32 -> 29 us in the per-launch table (bit-identical), 506.3 / 507.7
// against 509.0 / 506.0 images/s for the step: nothing outside the noise, so the rule stays at 64
constexpr int WIDE_NSTEPS = 64;
constexpr int SHORT_K_STEPS = 16;     // the two-buffer 128 x 128 tiles take K <= 512

namespace {
struct ConvPlanIn {             // what the selection depends on: conv_run's arguments with presence flags for the pointers
    int mode;                   // amp_ctx::conv_mode
    amp_conv_desc d;
    int groups, fmt, in_shift, force_f32;
    bool res, mask, scale;
    int fuse;                   // 0: none, 1: PredictFuse, 2: RpnFuse with rpn_ld predictor rows
    int rpn_ld;
};
struct ConvPlan {
    amp::ConvKernel kernel;
    int epi;                    // the launch's epilogue template argument (0 generic, 1 rows, 2 scatter / upsampled residual, 3: predict or RPN tail with 16 rows, 4 / 5: 32 / 48 rows)
    int ntn, nblk, stagger;     // ConvArgs::ntn, ::nblk (the grid), ::stagger
    int tiles_x, tiles_y;       // the patch kernels' 8 x 16 pixel tiles
    int nloop_nt;               // N tiles per workgroup of conv1x1_nloop_kernel
    int rpn_nbp;                // blocks of 16 predictor rows of the fused RPN tail
    bool dominant;              // a launch of the dominant kernel (amp_prof_rec::variant 0)
    bool f16x3;                 // the kernel reads the weights in the split layout
    int Ho, Wo, M, K, nsteps, cin_win, cpg, out_mode, y_split, korder;      // the layer as ConvArgs carries it
    size_t x_bytes, w_bytes;
};

// conv3x3_c64_kernel is taken from 512 tiles of 8 x 16 pixels x 64 channels on (patch_conv = 2: whatever the grid size)
bool c64_patch_fills(const ConvSwitches& sw, long long tiles) { return sw.patch_conv == 2 || tiles >= 512; }

// Which kernel takes the layer, and with which grid: pure host code (no HIP call, nothing of a context but its mode).  AMP_ERR_ARG + amp_last_error
// on a combination no kernel supports.
int conv_plan(const ConvPlanIn& in, const ConvSwitches& sw, ConvPlan* plan) {
    using amp::ConvKernel;
    const amp_conv_desc* d = &in.d;
    ConvPlan p = ConvPlan();
    AMP_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "amp_conv2d_nhwc: bad shape");
    AMP_REQUIRE(d->Cin % 4 == 0, "amp_conv2d_nhwc: Cin=%d must be a multiple of 4 (pad the input)", d->Cin);
    AMP_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "amp_conv2d_nhwc: bad window");
    AMP_REQUIRE(d->res_mode >= 0 && d->res_mode <= 2 && d->out_mode >= 0 && d->out_mode <= 2,
                "amp_conv2d_nhwc: bad res_mode/out_mode");
    AMP_REQUIRE(d->res_mode == 0 || in.res, "amp_conv2d_nhwc: res_mode=%d needs res", d->res_mode);
    const int Cin = d->Cin, Cout = d->Cout, KH = d->KH, KW = d->KW;
    p.Ho = (d->H + 2 * d->pad - KH) / d->stride + 1;
    p.Wo = (d->W + 2 * d->pad - KW) / d->stride + 1;
    AMP_REQUIRE(p.Ho > 0 && p.Wo > 0, "amp_conv2d_nhwc: empty output");
    AMP_REQUIRE(d->res_mode != 2 || (p.Ho % 2 == 0 && p.Wo % 2 == 0),
                "amp_conv2d_nhwc: res_mode=2 needs even output size, got %dx%d", p.Ho, p.Wo);
    AMP_REQUIRE(d->out_mode != 1 || Cout % 4 == 0, "amp_conv2d_nhwc: out_mode=1 needs Cout %% 4 == 0");
    const long long Mll = (long long)d->B * p.Ho * p.Wo;
    AMP_REQUIRE(Mll < (1ll << 31) / 4 && (long long)d->B * d->H * d->W < (1ll << 31),
                "amp_conv2d_nhwc: tensor too large for 32-bit pixel indices");
    p.M = (int)Mll;
    const bool grouped = in.groups > 1;
    p.cin_win = p.cpg = Cin;
    if (grouped) {
        AMP_REQUIRE(Cin == Cout && Cin % in.groups == 0 && Cout % 64 == 0 && d->out_mode == 0,
                    "amp_conv2d_grouped_nhwc: needs Cin == Cout, a multiple of 64 and of groups, out_mode 0");
        p.cpg = Cin / in.groups;
        AMP_REQUIRE(p.cpg == 8 || p.cpg == 16 || p.cpg == 32 || p.cpg == 64, "amp_conv2d_grouped_nhwc: %d channels per group (8/16/32/64 supported)", p.cpg);
        p.cin_win = 64;
    }
    p.K = KH * KW * p.cin_win;
    p.nsteps = amp::cdiv(p.K, BK);
    const int epi = (sw.generic_epi || (Cout & 3) != 0) ? 0 : ((d->res_mode == 2 || d->out_mode != 0) ? 2 : 1);
    const int ntm = amp::cdiv(p.M, 128);
    p.x_bytes = (size_t)d->B * d->H * d->W * Cin * sizeof(float);
    p.w_bytes = (size_t)Cout * p.K * sizeof(float);
    // LDS-DMA kernel: every layer but the stem (Cin = 4); buffers must stay below the out-of-range marker (2 GiB)
    const bool small = sw.ablate == 0 && p.x_bytes < (size_t)OOB_VOFF && p.w_bytes < (size_t)OOB_VOFF;
    const bool glds = (Cin % BK == 0) && small;
    AMP_REQUIRE(!grouped || glds, "amp_conv2d_grouped_nhwc: operands must stay below 2 GiB");
    const bool stem = Cin == 4 && KW == 8 && Cout <= 64 && small;   // the padded 7x7 stem
    const bool x_is_split = (in.fmt & 1) != 0, res_split = (in.fmt & 4) != 0, mask_split = (in.fmt & 8) != 0;
    p.y_split = (in.fmt & 2) ? 1 : 0;
    p.korder = (sw.korder && KH * KW > 1) ? 1 : 0;
    p.out_mode = d->out_mode;
    p.rpn_nbp = 1;
    if (in.fuse == 1) {     // the mask head's deconv with ReLU + predictor + sigmoid in its epilogue (conv_epilogue_predict)
        AMP_REQUIRE(x_is_split && d->out_mode == 1 && Cout == 1024 && KH == 1 && KW == 1 && d->relu && !in.res && !in.mask && !in.scale && sw.split_ring,
                    "conv: the fused deconv-predict epilogue needs a split input, Cout = 4 x 256, ReLU and the ring kernel");
        p.out_mode = 3;
    } else if (in.fuse == 2) {      // the RPN head's predictors in the 3x3 conv's epilogue (conv_epilogue_rpn): one 128 x 256 tile = all hidden channels of 128 pixels
        AMP_REQUIRE(x_is_split && d->out_mode == 0 && Cout == 256 && d->relu && !in.res && !in.mask && sw.split_ring && in.in_shift == 0,
                    "conv: the fused RPN epilogue needs a split input, Cout = 256, ReLU and the ring kernel");
        AMP_REQUIRE(in.rpn_ld == 16 || ((in.rpn_ld == 32 || in.rpn_ld == 48) && !p.korder), "conv: the fused RPN epilogue writes 16, 32 or 48 predictor rows (16 with AMP_KORDER), not %d", in.rpn_ld);
        p.rpn_nbp = in.rpn_ld / 16;
        p.out_mode = 4;
        p.y_split = 0;
    }
    AMP_REQUIRE(!mask_split || (in.mask && epi != 0 && Cout % 32 == 0 && p.out_mode == 0), "conv: a split-format mask needs mask, Cout %% 32 == 0, out_mode 0 and a fast epilogue");
    AMP_REQUIRE(!res_split || (in.res && epi != 0 && Cout % 32 == 0), "conv: a split-format residual needs res, Cout %% 32 == 0 and a fast epilogue");
    // split output: out_mode 0; or the 2x2 deconv scatter (out_mode 1) straight from the ring kernel's accumulators -- checked again where the kernel is chosen
    const bool deconv_split = p.y_split && p.out_mode == 1;
    AMP_REQUIRE(!p.y_split || ((p.out_mode == 0 || p.out_mode == 1) && Cout % 32 == 0 && epi != 0), "conv: split output needs out_mode 0 (or the deconv scatter) and Cout %% 32 == 0");
    AMP_REQUIRE(!deconv_split || ((Cout / 4) % 64 == 0 && !in.res && !in.mask && x_is_split && sw.split_ring && Cout % 256 == 0),
                "conv: a split deconv output needs Cout / 4 %% 64 == 0, a split input, no residual / mask and the ring kernel's direct epilogue");
    AMP_REQUIRE(!x_is_split || (in.mode == AMP_CONV_F16X3 && !in.force_f32 && Cin % 32 == 0 && glds),
                "conv: a split-format input needs AMP_CONV_F16X3, Cin %% 32 == 0 and operands below 2 GiB");
    p.epi = epi;
    p.stagger = sw.stagger;
    p.tiles_x = amp::cdiv(p.Wo, 16); p.tiles_y = amp::cdiv(p.Ho, 8);
    auto take = [&](ConvKernel k, int ntn, long long nblk, bool dominant = false) {
        p.kernel = k; p.ntn = ntn; p.nblk = (int)nblk; p.dominant = dominant;
        *plan = p;
        return AMP_OK;
    };
    const int nblk128 = ntm * amp::cdiv(Cout, 128);
    if (in.mode == AMP_CONV_F16X3 && !in.force_f32 && sw.ablate == 0 && (glds || stem)) {
        p.f16x3 = true;
        // 256-wide tiles (8 waves, one workgroup per CU) when they fill the chip twice -- or once, if the K loop is long enough to
        // amortise a single round (fc1: M = 8000, K = 12544: 64-wide tiles re-read the 400 MB activation matrix from HBM)
        const int nblk256 = (Cout % 256 == 0) ? ntm * (Cout / 256) : 0;
        const bool wide256 = sw.f16x3_bn256 && !grouped && !stem && (nblk256 >= 512 || (nblk256 >= 192 && p.nsteps >= WIDE_NSTEPS));
        const int ntm256 = amp::cdiv(p.M, 256);
        // a split input that carries a 2^in_shift (scaled loss gradients): only the ring kernel undoes it (out_scale in its fold)
        AMP_REQUIRE(!(x_is_split && in.in_shift != 0) || (sw.split_ring && epi != 0 && wide256 && p.out_mode != 3),
                    "conv: a scaled split input needs a layer the 128 x 256 ring kernel takes (Cout %% 256 == 0, enough tiles)");
        // N tiles per workgroup for the short-K 1x1 layers on the ring kernel (0: not such a layer): as many as leave a full round of workgroups
        int nloop_nt = 0;
        if (KH == 1 && KW == 1 && d->pad == 0 && !grouped && Cout % 256 == 0 && Cout >= 512 && Cin % BK == 0 && p.nsteps >= 2 && p.nsteps <= 16 && !p.korder &&
            p.y_split && !in.mask && d->res_mode == 0 && (p.out_mode == 0 || p.out_mode == 1)) {      // (no residual, no mask: see conv_epilogue_direct_rows PLAIN)
            const int ntn_ = Cout / 256;
            nloop_nt = ntn_ < 8 ? ntn_ : 8;
            while (nloop_nt > 1 && (ntn_ % nloop_nt != 0 || (long long)ntm * (ntn_ / nloop_nt) < 256)) --nloop_nt;
        }
        const long long tiles = (long long)d->B * p.tiles_y * p.tiles_x;      // 8 x 16 pixel tiles of the patch kernels
        const long long p256_tiles = tiles * (Cout / 256);
        const bool plain_3x3 = KH == 3 && KW == 3 && d->stride == 1 && d->pad == 1;
        const bool patch256_ok = sw.patch256 != 0 && x_is_split && sw.split_ring && epi != 0 && !grouped && plain_3x3 &&
            Cin % 32 == 0 && Cin >= 64 && Cout % 256 == 0 && p.nsteps == 9 * (Cin / 32) &&
            (p.out_mode == 4 || (p.out_mode == 0 && p.y_split && (!in.mask || mask_split) && (d->res_mode == 0 || (d->res_mode == 1 && res_split)))) &&
            (sw.patch256 == 2 || ((p256_tiles >= 512 || (p256_tiles >= 192 && p.nsteps >= 64)) && p256_tiles * 100 <= (long long)nblk256 * 108));
        const bool ring = x_is_split && sw.split_ring && epi != 0;      // conv_split_kernel's precondition
        if (sw.patch_conv != 0 && x_is_split && p.y_split && plain_3x3 && p.cin_win == 64 && (grouped || (Cin == 64 && Cout == 64)) &&
            p.out_mode == 0 && d->res_mode == 0 && epi != 0 && (!in.mask || mask_split) && in.in_shift == 0 && Cout % 64 == 0 && c64_patch_fills(sw, tiles * (Cout / 64)))
            // res2's dense 64 -> 64 layers and the ResNeXt conv2: a pixel patch staged once, nine taps read out of it (conv3x3_c64_kernel)
            return take(grouped && p.cpg <= 32 ? ConvKernel::C64_PATCH_DIAG : ConvKernel::C64_PATCH, Cout / 64, tiles * (Cout / 64));
        if (patch256_ok) {
            // FPN output / RPN / res4 / res5 3x3: 8 x 16 pixel tiles, the patch of a 32-channel chunk staged once for its nine taps (conv3x3_patch_kernel)
            p.epi = p.out_mode == 4 ? 2 + p.rpn_nbp : 1;
            return take(ConvKernel::PATCH256, Cout / 256, p256_tiles, true);
        }
        if (p.out_mode == 3 && sw.mask_tail_loop && Cin % BK == 0 && !p.korder && p.Ho * p.Wo >= 128 /* a 128-pixel block spans at most two RoIs */)
            return take(ConvKernel::MASK_TAIL, 1, ntm);      // fused mask-head tail: the four taps of a pixel block in one workgroup (a kernel of its own: not the dominant one)
        if (p.out_mode == 3) {                                // ... one (pixel block, tap) tile per workgroup on the 128 x 256 ring kernel
            p.epi = 3;
            return take(ConvKernel::SPLIT_128x256, 4, ntm * 4, true);
        }
        if (p.out_mode == 4) {                                // fused RPN tail: one N tile
            p.epi = 2 + p.rpn_nbp;
            return take(ConvKernel::SPLIT_128x256, 1, ntm, true);
        }
        if (ring && sw.short_k && !grouped && p.nsteps <= SHORT_K_STEPS && in.res && d->res_mode == 1 && res_split && p.y_split && !in.mask &&
            Cout % 128 == 0 && ntm * (Cout / 128) >= 1024) {
            // the trunk's conv3 + residual (K = 64 ... 256 into 4 K channels: byte-bound): 128 x 128 tiles on TWO buffers -- tile s + 2 goes into
            // the buffer of tile s once every wave holds its fragments, same prefetch distance as the three-buffer ring -- so that TWO
            // workgroups fit a CU and one's residual loads and stores overlap the other's staging: res2 -5 %, res3 -8 %, res4 -3 % on these
            // launches (A/B in one call; bit-identical); without a residual it is 4 % slower
            p.stagger = 0;
            return take(ConvKernel::SPLIT_SHORT_128x128, Cout / 128, ntm * (Cout / 128));
        }
        if (sw.nloop && nloop_nt >= 2 && ring && (wide256 || deconv_split)) {
            // short-K 1x1 layers: several N tiles of a pixel block in one workgroup, the ring carried across them (conv1x1_nloop_kernel)
            p.nloop_nt = nloop_nt;
            return take(p.out_mode == 1 ? ConvKernel::NLOOP_SCATTER : ConvKernel::NLOOP, Cout / 256, ntm * (Cout / 256 / nloop_nt));
        }
        if (ring && (wide256 || deconv_split))                // 128 x 256 tiles, 3-buffer ring
            // (the K = 256 deconv with its scatter epilogue on two-buffer 128 x 128 tiles, two workgroups per CU: 1009 against 931 us -- measured, not kept)
            return take(ConvKernel::SPLIT_128x256, Cout / 256, ntm * (Cout / 256), true);
        if (ring && !grouped && Cout % 128 == 0 && (ntm256 * (Cout / 128) >= 512 || (ntm256 * (Cout / 128) >= 192 && p.nsteps >= 64)))
            return take(ConvKernel::SPLIT_256x128, Cout / 128, ntm256 * (Cout / 128));      // Cout = 128 (or 384, ...): 256 x 128 tiles
        if (ring && sw.tall64 && epi == 1 && !grouped && Cout == 64 && in.in_shift == 0 && ntm256 >= 1024) {
            p.stagger = 0;
            return take(ConvKernel::SPLIT_TALL64, 1, ntm256);
        }
        if (x_is_split) {      // both operands by LDS-DMA
            if (wide256) return take(ConvKernel::F16X3S_256, Cout / 256, ntm * (Cout / 256));
            if (!grouped && Cout > 64 && nblk128 >= 512) return take(ConvKernel::F16X3S_128, amp::cdiv(Cout, 128), nblk128);
            // (grouped: the window of a 64-wide N tile is the tile's own 64 input channels = 256 B of a split row too; <= 32 channels per group: one K-step per tap)
            return take(grouped && p.cpg <= 32 ? ConvKernel::F16X3S_G32 : ConvKernel::F16X3S_64, amp::cdiv(Cout, 64), ntm * amp::cdiv(Cout, 64));
        }
        if (stem) {
            p.epi = epi == 2 ? 0 : epi;
            return take(ConvKernel::F16X3_STEM, 1, ntm);
        }
        if (grouped) return take(ConvKernel::F16X3_64, Cout / 64, ntm * (Cout / 64));     // the window of a 64-wide N tile is the tile's own 64 input channels
        if (wide256) return take(ConvKernel::F16X3_256, Cout / 256, ntm * (Cout / 256));
        if (Cout > 64 && nblk128 >= 512) return take(ConvKernel::F16X3_128, amp::cdiv(Cout, 128), nblk128);
        return take(ConvKernel::F16X3_64, amp::cdiv(Cout, 64), ntm * amp::cdiv(Cout, 64));
    }
    if (stem) return take(ConvKernel::GLDS_STEM, 1, ntm);
    if (glds) {     // BN = 64 also for wide layers whose 128-wide grid would leave CUs idle (2 workgroups fit per CU)
        if (!grouped && Cout > 64 && nblk128 >= 512) return take(ConvKernel::GLDS_128, amp::cdiv(Cout, 128), nblk128, true);
        return take(ConvKernel::GLDS_64, amp::cdiv(Cout, 64), ntm * amp::cdiv(Cout, 64));
    }
    if (Cout > 64) return take(ConvKernel::MFMA_128, amp::cdiv(Cout, 128), nblk128);
    return take(ConvKernel::MFMA_64, 1, ntm);
}
}  // namespace
