// The fused tails: the mask predictor (conv_epilogue_predict, with its prefetch) and the RPN predictor rows (conv_epilogue_rpn*).
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"

namespace {

// The predictor rows a wave tile can need, fetched ahead of the epilogue (conv_split_kernel issues this BEFORE its K loop): a wave tile is 64
// consecutive GEMM rows = pixels of at most TWO RoIs (196 pixels each), so two class ids, two weight quads per lane and two biases cover it.
// Before round 4 every one of the 16 row groups of the epilogue walked pred_cls[b] -> pred_w[cls] again -- two dependent global round trips
// per group, and two more in the final reduction: ~8 us of a 19-us tile (K = 256: 8 K-steps) that nothing hid.
struct PredictPrefetch {
    unsigned int b0;
    f32x4 wp0, wp1;
    float pb0, pb1;
};
__device__ __forceinline__ PredictPrefetch predict_prefetch(const ConvArgs& a, int wave, int lane, int m0) {
    const int wm = wave >> 2, wn = wave & 3, l15 = lane & 15;
    const int mw0 = m0 + wm * 64;
    const unsigned int mf = min((unsigned int)mw0, (unsigned int)(a.M - 1)), ml = min((unsigned int)(mw0 + 63), (unsigned int)(a.M - 1));
    PredictPrefetch p;
    p.b0 = fastdiv(mf, a.div_howo_mul, a.div_howo_shr);
    const unsigned int b1 = fastdiv(ml, a.div_howo_mul, a.div_howo_shr);
    int c0 = a.pred_cls[p.b0], c1 = a.pred_cls[b1];
    c0 = (c0 >= 0 && c0 < a.pred_K) ? c0 : 0;
    c1 = (c1 >= 0 && c1 < a.pred_K) ? c1 : 0;
    const int co = wn * 64 + l15 * 4;
    p.wp0 = *reinterpret_cast<const f32x4*>(a.pred_w + (size_t)c0 * 256 + co);
    p.wp1 = *reinterpret_cast<const f32x4*>(a.pred_w + (size_t)c1 * 256 + co);
    p.pb0 = a.pred_b[c0];
    p.pb1 = a.pred_b[c1];
    return p;
}

// Epilogue of the fused mask-head tail (out_mode 3).  The GEMM is the ConvTranspose2d 2x2 s2 as a 1x1 convolution to
// Cout = 4 * 256 channels ordered (tap, co); a 128 x 256 tile is therefore 128 input pixels x ONE tap x all 256 output channels.
// Per tile row (RoI b, input pixel (oy, ox), tap (ky, kx)): v[co] = relu(acc[co] + bias[co]) is the deconv output at output pixel
// (2oy + ky, 2ox + kx); the predictor's logit for the RoI's class c is  sum_co v[co] * wp[c][co] + bp[c];  the mask probability its
// sigmoid.  fp32 products and sums in a fixed order (4 columns per lane, xor tree over the 16 lanes of a row, the 4 N-waves in order):
// deterministic.  Replaces a 1.28 GB write, its read-back, the 1x1 predictor GEMM and mask_prob_kernel (B = 8, 200 detections).
__device__ __forceinline__ void conv_epilogue_predict(const ConvArgs& a, f32x4 (&acc)[4][4], float* lds, int wave, int lane, int m0, int n0, const PredictPrefetch& pf) {
    constexpr int WTM = 64, WTN = 64, SLD = WTN + 4;
    const int wm = wave >> 2, wn = wave & 3;
    const int l15 = lane & 15, lq = lane >> 4;
    float* stage = lds + wave * (WTM * SLD);
    float* red = lds + 8 * (WTM * SLD);                 // [4 N-waves][128 rows] partial sums (2 KiB behind the staging tiles)
#pragma unroll
    for (int i = 0; i < 4; ++i)                          // role-swapped accumulators: lane = (tile row l15, channels swap_channel(16 j + 4 lq + e))
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(stage + (i * 16 + l15) * SLD + 32 * (j >> 1) + 8 * lq + 4 * (j & 1)) = acc[i][j];
    __builtin_amdgcn_wave_barrier();
    const int tap = n0 >> 8;                            // Cout = 4 * 256: the tile's N range is one tap
    const int co = wn * WTN + l15 * 4;                  // this lane's 4 output channels
    const int mw0 = m0 + wm * WTM;
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (a.shift) bias = *reinterpret_cast<const f32x4*>(a.shift + n0 + co);
    bool bad = false;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const int rl = it * 4 + lq;                     // row of the wave tile
        const unsigned int m = min((unsigned int)(mw0 + rl), (unsigned int)(a.M - 1));
        const unsigned int b = fastdiv(m, a.div_howo_mul, a.div_howo_shr);
        const f32x4 wp = (b == pf.b0) ? pf.wp0 : pf.wp1;         // the RoI's class row, fetched ahead (same values as pred_w[pred_cls[b]])
        const f32x4 v = *reinterpret_cast<const f32x4*>(stage + rl * SLD + l15 * 4);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bad = bad || !(fabsf(v[q]) <= 3.0e38f);
            const float o = fmaxf(__fadd_rn(v[q], bias[q]), 0.f);
            s = __fadd_rn(s, __fmul_rn(o, wp[q]));
        }
        s = __fadd_rn(s, __shfl_xor(s, 8, 16));
        s = __fadd_rn(s, __shfl_xor(s, 4, 16));
        s = __fadd_rn(s, __shfl_xor(s, 2, 16));
        s = __fadd_rn(s, __shfl_xor(s, 1, 16));
        if (l15 == 0) red[wn * 128 + wm * WTM + rl] = s;
    }
    if (bad) atomicOr(a.range_flag, 1);
    __syncthreads();
    if (wn == 0) {                                      // 2 waves x 64 rows: one row per lane
        const int rl = wm * WTM + lane;
        const int m = m0 + rl;
        if (m < a.M) {
            unsigned int b, oy, ox;
            conv_pixel(a, (unsigned int)m, b, oy, ox);
            float x = __fadd_rn(__fadd_rn(__fadd_rn(red[rl], red[128 + rl]), red[256 + rl]), red[384 + rl]);
            x = __fadd_rn(x, (b == pf.b0) ? pf.pb0 : pf.pb1);
            const float p = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x)));
            a.prob[((size_t)b * 2 * a.Ho + 2 * oy + (tap >> 1)) * (2 * a.Wo) + 2 * ox + (tap & 1)] = p;
        }
    }
}

// Epilogue of the fused RPN tail (out_mode 4, 128 x 256 tile = 128 pixels x all 256 hidden channels).  With the role-swapped MFMA a lane
// holds, per tile row, channels [8 lq, 8 lq + 8) of each 32-channel group of its wave's 64 -- after affine, ReLU and the split, exactly the
// A fragment (row = pixel l15, k group lq) of a v_mfma_f32_16x16x32_f16 over that group.  So the 1x1 predictors are a second f16x3
// product right here: B = the predictor rows (16 outputs x 32 channels, split rows, straight from memory), 2 groups per wave, the four
// N-waves' partial sums added through LDS in wave order, + bias -> pred [M][16].  Same operands as the separate 1x1 launch read from the
// stored hidden tensor (the halves are identical), another summation order.  Replaces a 537 MB write + read at p2 and a launch per level.
// row_of(i, r): the GEMM row (pixel) of row r (0..15) of the wave tile's 16-row block i, or a.M (or more) for a row outside the image
// NBP blocks of 16 predictor rows (A <= 3, 6, 9 anchors per location): lane l15 of block j owns predictor row 16 j + l15; per block the same three MFMAs per
// 32-channel group and the same wave-order reduction, the 32 KB reduction buffer re-used behind a barrier, the block's weight fragments loaded inside the
// loop (16 registers, not 16 NBP).  NBP = 1 is the 16-row head as it always was.
template <int NBP, class RowOf>
__device__ __forceinline__ void conv_epilogue_rpn_rows(const ConvArgs& a, f32x4 (&acc)[4][4], float* lds, int wave, int lane, int n0, RowOf row_of) {
    const int wm = wave >> 2, wn = wave & 3;
    const int l15 = lane & 15, lq = lane >> 4;
    const int nw0 = n0 + wn * 64;
    f32x2 sc[2][4], sh[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int n = nw0 + 32 * g + 8 * lq;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sc[g][p] = a.scale ? f32x2{a.scale[n + 2 * p], a.scale[n + 2 * p + 1]} : f32x2{1.f, 1.f};
            sh[g][p] = a.shift ? f32x2{a.shift[n + 2 * p], a.shift[n + 2 * p + 1]} : f32x2{0.f, 0.f};
        }
    }
    f32x4* red = reinterpret_cast<f32x4*>(lds);                     // [wm][wn][i][lane]
#pragma unroll
    for (int j = 0; j < NBP; ++j) {
        if (j > 0) __syncthreads();                                 // the previous block's sums have been read
        f16x8 wh[2], wl[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int n = nw0 + 32 * g + 8 * lq;
            const char* wb = reinterpret_cast<const char*>(a.rpn_w + (size_t)(16 * j + l15) * a.Cout) + (size_t)(n >> 5) * 128 + (size_t)(n & 31) * 2;
            wh[g] = *reinterpret_cast<const f16x8*>(wb);
            wl[g] = *reinterpret_cast<const f16x8*>(wb + 64);
        }
        f32x2 chk = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 d = {0.f, 0.f, 0.f, 0.f}, dx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                f16x8 hi, lo;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const f32x4& blk = acc[i][2 * g + (p >> 1)];
                    const f32x2 v = {blk[2 * (p & 1)], blk[2 * (p & 1) + 1]};
                    if (j == 0) chk = __builtin_elementwise_fma(v, f32x2{0.f, 0.f}, chk);
                    f32x2 o = v * sc[g][p] + sh[g][p];
                    o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f);
                    const f16x2 h = __builtin_convertvector(o, f16x2);
                    const f32x2 hf = {(float)h[0], (float)h[1]};
                    // the hidden value is an OPERAND of the product below, never stored: finite sums whose FrozenBN + ReLU leave the f16 range
                    // (hi = inf) have no consumer that would notice, so the half itself is checked
                    if (j == 0) chk = __builtin_elementwise_fma(hf, f32x2{0.f, 0.f}, chk);
                    const f32x2 l = __builtin_elementwise_fma(hf, f32x2{-LO_SCALE, -LO_SCALE}, o * LO_SCALE);
                    const f16x2 lh = __builtin_convertvector(l, f16x2);
                    hi[2 * p] = h[0]; hi[2 * p + 1] = h[1];
                    lo[2 * p] = lh[0]; lo[2 * p + 1] = lh[1];
                }
                dx = __builtin_amdgcn_mfma_f32_16x16x32_f16(lo, wh[g], dx, 0, 0, 0);
                dx = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi, wl[g], dx, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi, wh[g], d, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = fold(d[e], dx[e]);
            red[((wm * 4 + wn) * 4 + i) * 64 + lane] = d;
        }
        if (j == 0) { if (!(chk[0] == 0.f) || !(chk[1] == 0.f)) atomicOr(a.range_flag, 1); }
        __syncthreads();
        if (wn == 0) {                                              // lane = (output 16 j + l15, pixels 4 lq .. 4 lq + 3 of block i)
            const float bias = a.rpn_b[16 * j + l15];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 s = red[((wm * 4 + 0) * 4 + i) * 64 + lane];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const f32x4 t = red[((wm * 4 + w) * 4 + i) * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] = __fadd_rn(s[e], t[e]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int m = row_of(i, 4 * lq + e);
                    if (m < a.M) a.rpn_pred[(size_t)m * (16 * NBP) + 16 * j + l15] = __fadd_rn(s[e], bias);
                }
            }
        }
    }
}
template <int NBP>
__device__ __forceinline__ void conv_epilogue_rpn(const ConvArgs& a, f32x4 (&acc)[4][4], float* lds, int wave, int lane, int m0, int n0) {
    const int mw0 = m0 + (wave >> 2) * 64;
    conv_epilogue_rpn_rows<NBP>(a, acc, lds, wave, lane, n0, [mw0](int i, int r) { return mw0 + i * 16 + r; });
}

}  // namespace
