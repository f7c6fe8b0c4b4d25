// Convolution epilogues: the LDS-transposed generic / fast forms, the f16x3 MFMA step, and conv_split_kernel's row / direct / swapped forms.
#pragma once
#include "common.h"
#include <type_traits>
#include "lds_ring.h"
#include "conv_args.h"

namespace {

// Epilogue shared by both kernels: accumulators -> LDS (per-wave tile, [m][n]) -> row-wise float4 residual loads + stores.
// The MFMA C layout puts one n per lane and 16 m in registers: stored directly that is 64 dword stores per lane and,
// with a residual, 64 dependent dword loads.  Transposed through LDS every lane owns 4 consecutive n of one row per step:
// 16-B coalesced residual loads (all issued before the first store) and 16-B stores.  Callers pass the wave's tile origin
// (mw0, nw0) and must have synchronised the workgroup after the last operand reads.
template <int WTM, int WTN>
__device__ __forceinline__ void conv_epilogue_generic_rows(const ConvArgs& a, float* stage, int lane, int mw0, int nw0, int HoWo);

template <int WTM, int WTN, int MT, int NT, bool CHECK = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x16 (&acc)[MT][NT], float* lds, int wave, int lane,
                                              int mw0, int nw0, int HoWo) {
    if (CHECK) {
        bool bad = false;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) bad = bad || !(fabsf(acc[i][j][e]) <= 3.0e38f);
        if (bad) atomicOr(a.range_flag, 1);
    }
    const int l31 = lane & 31, lh = lane >> 5;
    constexpr int SLD = WTN + 4;                       // padded row of the staging tile (floats)
    float* stage = lds + wave * (WTM * SLD);
    // (the loop's last __syncthreads() already ordered every wave's operand reads before these writes)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stage[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * SLD + j * 32 + l31] = acc[i][j][e];
    conv_epilogue_generic_rows<WTM, WTN>(a, stage, lane, mw0, nw0, HoWo);
}

// the same from MB x NB blocks of 16x16 MFMA accumulators
template <int WTM, int WTN, int MB, int NB, bool CHECK = false>
__device__ __forceinline__ void conv_epilogue16(const ConvArgs& a, f32x4 (&acc)[MB][NB], float* lds, int wave, int lane,
                                                int mw0, int nw0, int HoWo) {
    if (CHECK) {
        bool bad = false;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) bad = bad || !(fabsf(acc[i][j][e]) <= 3.0e38f);
        if (bad) atomicOr(a.range_flag, 1);
    }
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr int SLD = WTN + 4;
    float* stage = lds + wave * (WTM * SLD);
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                stage[(i * 16 + 4 * lq + e) * SLD + j * 16 + l15] = acc[i][j][e];
    conv_epilogue_generic_rows<WTM, WTN>(a, stage, lane, mw0, nw0, HoWo);
}

template <int WTM, int WTN>
__device__ __forceinline__ void conv_epilogue_generic_rows(const ConvArgs& a, float* stage, int lane, int mw0, int nw0, int HoWo) {
    constexpr int SLD = WTN + 4;                       // padded row of the staging tile (floats)
    constexpr int F4R = WTN / 4;                       // float4 per row
    constexpr int RPI = 64 / F4R;                      // rows per iteration (one wave)
    constexpr int NIT = WTM / RPI;

    const int erow = lane / F4R;                       // row within an iteration
    const int ec4 = lane % F4R;
    const int n = nw0 + ec4 * 4;
    const bool vec = (a.Cout & 3) == 0;                // rows of y / res are 16-B aligned
    const bool nv = n < a.Cout;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (n + q < a.Cout) {
            if (a.scale) sc[q] = a.scale[n + q];
            if (a.shift) sh[q] = a.shift[n + q];
        }
    }
    const int C2 = a.Cout >> 2;                        // deconv scatter only

    size_t yoff[NIT];
    f32x4 rres[NIT];
    bool mv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int m = mw0 + it * RPI + erow;
        mv[it] = nv && m < a.M;
        yoff[it] = (size_t)m * a.Cout + n;
        rres[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!mv[it]) continue;
        if (a.res_mode != 0 || a.out_mode != 0) {
            const int b = m / HoWo;
            const int rem = m - b * HoWo;
            const int oy = rem / a.Wo;
            const int ox = rem - oy * a.Wo;
            size_t roff = yoff[it];
            if (a.res_mode == 2)
                roff = ((size_t)(b * (a.Ho >> 1) + (oy >> 1)) * (a.Wo >> 1) + (ox >> 1)) * a.Cout + n;
            if (a.res_mode != 0) {
                if (vec) {
                    rres[it] = *reinterpret_cast<const f32x4*>(a.res + roff);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (n + q < a.Cout) rres[it][q] = a.res[roff + q];
                }
            }
            if (a.out_mode == 1) {
                const int kk = n / C2;
                const int co = n - kk * C2;
                const int oy2 = 2 * oy + (kk >> 1), ox2 = 2 * ox + (kk & 1);
                yoff[it] = ((size_t)(b * 2 * a.Ho + oy2) * (2 * a.Wo) + ox2) * C2 + co;
            } else if (a.out_mode == 2) {   // stride-2 scatter into a [B,2Ho,2Wo,Cout] tensor (data gradient of a strided 1x1 conv)
                yoff[it] = ((size_t)(b * 2 * a.Ho + 2 * oy) * (2 * a.Wo) + 2 * ox) * a.Cout + n;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();                   // staging writes of this wave precede its reads (same-wave LDS order)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(stage + (it * RPI + erow) * SLD + ec4 * 4);
        if (!mv[it]) continue;
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float t = __fadd_rn(__fmul_rn(v[q], sc[q]), sh[q]);
            if (a.res_mode != 0) t = __fadd_rn(t, rres[it][q]);
            if (a.relu) t = fmaxf(t, 0.f);
            o[q] = t;
        }
        if (a.mask && a.mask_split) {                  // the gating activation in the split row format (Cout % 32 == 0, out_mode 0)
            const char* mb = reinterpret_cast<const char*>(a.mask + (yoff[it] - (size_t)n)) + (n >> 5) * 128 + (n & 31) * 2;
            const f16x4 mh = *reinterpret_cast<const f16x4*>(mb);
            const f16x4 ml = *reinterpret_cast<const f16x4*>(mb + 64);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = fold((float)mh[q], (float)ml[q]) > 0.f ? o[q] : 0.f;
        } else if (a.mask) {
            if (vec) {
                const f32x4 mk = *reinterpret_cast<const f32x4*>(a.mask + yoff[it]);
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = mk[q] > 0.f ? o[q] : 0.f;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (n + q < a.Cout) o[q] = a.mask[yoff[it] + q] > 0.f ? o[q] : 0.f;
            }
        }
        if (vec) {
            *reinterpret_cast<f32x4*>(a.y + yoff[it]) = o;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (n + q < a.Cout) a.y[yoff[it] + q] = o[q];
        }
    }
}

// One K-step (32 k) of the AMP_CONV_F16X3 product on a wave tile of MB x NB blocks of 16 x 16, operands in the LDS row format
// (per row 64 B of hi halves, 64 B of lo' halves, 16-B chunks XOR-swizzled by (row >> 1) & 7).  v_mfma_f32_16x16x32_f16: lane =
// (row l15 of a block, k group lq), so the hi halves of k 8lq.. are chunk lq of the row and their lo' halves chunk 4 + lq: one
// ds_read_b128 each, conflict-free over the 16 rows of a lane group.  Every AMP_CONV_F16X3 forward kernel computes through this
// function, whoever staged the tiles: that is what makes "split in the kernel" and "split by the producer" the same arithmetic.
// (Shape: the 16x16x32 MFMA does the flops of the 32x32x16 one in the same cycles with the same LDS bytes, but on random operands
// the chip holds a higher clock under it -- MI355X_MICROARCH.md -- measured here: +2..9 % on the 3x3 / fc layers.)
template <int MB, int NB>
struct F16x3Frags {
    f16x8 ah[MB], al[MB], bh[NB], bl[NB];
};
template <int MB, int NB>
__device__ __forceinline__ void f16x3_load16(const float* As, const float* Bs, int fo_hi, int fo_lo, F16x3Frags<MB, NB>& f) {
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        f.ah[i] = *reinterpret_cast<const f16x8*>(As + i * 16 * BK + fo_hi);
        f.al[i] = *reinterpret_cast<const f16x8*>(As + i * 16 * BK + fo_lo);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        f.bh[j] = *reinterpret_cast<const f16x8*>(Bs + j * 16 * BK + fo_hi);
        f.bl[j] = *reinterpret_cast<const f16x8*>(Bs + j * 16 * BK + fo_lo);
    }
}
// SWAP = true: the weights are the MFMA's A operand (rows) and the activations its B operand (columns): the same exact products
// summed in the same order into acc[i][j] / acx[i][j] (i: 16 tile rows m, j: 16 channels n), but a lane now holds, per block, FOUR
// CHANNELS (4 lq + e) of ONE tile row (l15) instead of four rows of one channel -- what conv_epilogue_direct needs.
template <int MB, int NB, bool SWAP = false>
__device__ __forceinline__ void f16x3_mfma16(const F16x3Frags<MB, NB>& f, f32x4 (&acc)[MB][NB], f32x4 (&acx)[MB][NB]) {
    // per accumulator the order is lo'*hi, hi*lo' (cross sums), hi*hi; consecutive MFMAs never share an accumulator (NB apart)
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        if (SWAP) {
#pragma unroll
            for (int j = 0; j < NB; ++j) acx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.bh[j], f.al[i], acx[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NB; ++j) acx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.bl[j], f.ah[i], acx[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.bh[j], f.ah[i], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) acx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.al[i], f.bh[j], acx[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NB; ++j) acx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.ah[i], f.bl[j], acx[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
        }
    }
}
template <int MB, int NB>
__device__ __forceinline__ void f16x3_step16(const float* As, const float* Bs, int fo_hi, int fo_lo, f32x4 (&acc)[MB][NB], f32x4 (&acx)[MB][NB]) {
    F16x3Frags<MB, NB> f;
    f16x3_load16<MB, NB>(As, Bs, fo_hi, fo_lo, f);
    f16x3_mfma16<MB, NB>(f, acc, acx);
}

// Fast epilogue for the layouts the model actually uses (Cout % 4 == 0): same LDS transposition and the same arithmetic as
// conv_epilogue, but straight-line: the row offsets advance by additions (SPATIAL = false: out_mode 0, res_mode 0/1) or come from
// two multiply-shift divisions per row (SPATIAL = true: upsampled residual, deconv / stride-2 scatter); residual and mask loads of
// all rows are issued before the first store; a block-uniform `full` flag removes the per-row bounds predicates from every tile
// but the last one.  (Measured on gfx950: the generic epilogue's per-row branches cost 13-55 % of the short-K layers.)
template <int WTM, int WTN, bool SPATIAL, bool CHECK>
__device__ __forceinline__ void conv_epilogue_rows(const ConvArgs& a, float* stage, int lane, int mw0, int nw0);
template <int WTM, int WTN, bool SPATIAL, bool CHECK>
__device__ __forceinline__ void conv_epilogue_rows8(const ConvArgs& a, float* stage, int lane, int mw0, int nw0);

template <int WTM, int WTN, int MT, int NT, bool SPATIAL, bool CHECK = false>
__device__ __forceinline__ void conv_epilogue_fast(const ConvArgs& a, f32x16 (&acc)[MT][NT], float* lds, int wave, int lane,
                                                   int mw0, int nw0) {
    const int l31 = lane & 31, lh = lane >> 5;
    constexpr int SLD = WTN + 4;
    float* stage = lds + wave * (WTM * SLD);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stage[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * SLD + j * 32 + l31] = acc[i][j][e];
    if (a.y_split && !a.mask && a.out_mode == 0) conv_epilogue_rows8<WTM, WTN, SPATIAL, CHECK>(a, stage, lane, mw0, nw0);
    else conv_epilogue_rows<WTM, WTN, SPATIAL, CHECK>(a, stage, lane, mw0, nw0);
}

// the same from 16x16 MFMA accumulators (v_mfma_f32_16x16x32_f16: lane = column, 4 consecutive rows per lane group of 16)
template <int WTM, int WTN, int MT, int NT, bool SPATIAL, bool CHECK = false>
__device__ __forceinline__ void conv_epilogue_fast16(const ConvArgs& a, f32x4 (&acc)[MT][NT], float* lds, int wave, int lane,
                                                     int mw0, int nw0) {
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr int SLD = WTN + 4;
    float* stage = lds + wave * (WTM * SLD);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                stage[(i * 16 + 4 * lq + e) * SLD + j * 16 + l15] = acc[i][j][e];
    if (a.y_split && !a.mask && a.out_mode == 0) conv_epilogue_rows8<WTM, WTN, SPATIAL, CHECK>(a, stage, lane, mw0, nw0);
    else conv_epilogue_rows<WTM, WTN, SPATIAL, CHECK>(a, stage, lane, mw0, nw0);
}

// Split-format output (the trunk's native activation format), 8 channels per lane: a lane's share of an output row is 16 B of hi
// halves and 16 B of lo' halves (and the same of a split residual), so every global access is a full dwordx4 -- with 4 channels per
// lane (conv_epilogue_rows) they were 8-B accesses and the memory-bound 1x1 layers ran 10 % slower than with fp32 rows.
// out_mode 0, no mask (inference), Cout % 32 == 0; same arithmetic, same order as conv_epilogue_rows.
template <int WTM, int WTN, bool SPATIAL, bool CHECK>
__device__ __forceinline__ void conv_epilogue_rows8(const ConvArgs& a, float* stage, int lane, int mw0, int nw0) {
    constexpr int SLD = WTN + 4;
    constexpr int L8R = WTN / 8;                       // lanes per row
    constexpr int RPI = 64 / L8R;                      // rows per iteration
    constexpr int NIT = WTM / RPI;
    const int erow = lane / L8R;
    const int ec8 = lane % L8R;
    const int n = nw0 + ec8 * 8;
    const bool nv = n < a.Cout;                        // Cout % 32 == 0
    float sc[8], sh[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        sc[q] = (nv && a.scale) ? a.scale[n + q] : 1.f;
        sh[q] = (nv && a.shift) ? a.shift[n + q] : 0.f;
    }
    const bool has_res = a.res_mode != 0;
    const size_t col_b = (size_t)(n >> 5) * 128 + (size_t)(n & 31) * 2;   // byte offset of this lane's hi halves inside a split row
#pragma unroll
    for (int h = 0; h < 2; ++h) {                      // two passes of NIT / 2 rows: bounds the live registers
        constexpr int HN = NIT / 2;
        size_t yrow[HN], rrow[HN];                     // float index of the row start in y / res
        bool mv[HN];
        f32x4 r0[HN], r1[HN];
#pragma unroll
        for (int t = 0; t < HN; ++t) {
            const int it = h * HN + t;
            const int mrow = mw0 + it * RPI + erow;
            mv[t] = nv && mrow < a.M;
            const unsigned int m = min((unsigned int)mrow, (unsigned int)(a.M - 1));
            yrow[t] = (size_t)m * a.Cout;
            rrow[t] = yrow[t];
            if (SPATIAL && a.res_mode == 2) {
                unsigned int b, oy, ox;
                conv_pixel(a, m, b, oy, ox);
                rrow[t] = ((size_t)(b * (a.Ho >> 1) + (oy >> 1)) * (a.Wo >> 1) + (ox >> 1)) * a.Cout;
            }
        }
        if (has_res) {
#pragma unroll
            for (int t = 0; t < HN; ++t) {
                if (!mv[t]) continue;
                if (a.res_split) {
                    const char* rb = reinterpret_cast<const char*>(a.res + rrow[t]) + col_b;
                    r0[t] = *reinterpret_cast<const f32x4*>(rb);          // 8 hi halves
                    r1[t] = *reinterpret_cast<const f32x4*>(rb + 64);     // 8 lo' halves
                } else {
                    r0[t] = *reinterpret_cast<const f32x4*>(a.res + rrow[t] + n);
                    r1[t] = *reinterpret_cast<const f32x4*>(a.res + rrow[t] + n + 4);
                }
            }
        }
        if (h == 0) __builtin_amdgcn_wave_barrier();   // staging writes of this wave precede its reads (same-wave LDS order)
        bool bad = false;
#pragma unroll
        for (int t = 0; t < HN; ++t) {
            const int it = h * HN + t;
            const float* sp = stage + (it * RPI + erow) * SLD + ec8 * 8;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp), v1 = *reinterpret_cast<const f32x4*>(sp + 4);
            f16x8 hi, lo;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float v = q < 4 ? v0[q] : v1[q - 4];
                if (CHECK) bad = bad || !(fabsf(v) <= 3.0e38f);
                float o = __fadd_rn(__fmul_rn(v, sc[q]), sh[q]);
                if (has_res) {
                    float r;
                    if (a.res_split) {
                        const f16x8 rh = __builtin_bit_cast(f16x8, r0[t]), rl = __builtin_bit_cast(f16x8, r1[t]);
                        r = fold((float)rh[q], (float)rl[q]);
                    } else {
                        r = q < 4 ? r0[t][q] : r1[t][q - 4];
                    }
                    o = __fadd_rn(o, r);
                }
                if (a.relu) o = fmaxf(o, 0.f);
                const _Float16 hh = (_Float16)o;
                hi[q] = hh;
                lo[q] = (_Float16)((o - (float)hh) * LO_SCALE);
            }
            if (mv[t]) {
                char* base = reinterpret_cast<char*>(a.y + yrow[t]) + col_b;
                *reinterpret_cast<f16x8*>(base) = hi;
                *reinterpret_cast<f16x8*>(base + 64) = lo;
            }
        }
        if (CHECK && bad) atomicOr(a.range_flag, 1);
    }
}

// ---- epilogues of conv_split_kernel (role-swapped MFMA, see f16x3_mfma16<.., SWAP = true>) ---------------------------------------
// Channel order inside a wave's 64 channels: LDS weight row w = 16 j + 4 q + e (block j, MFMA row 4 q + e) holds channel
// swap_channel(w) = 32 (j >> 1) + 8 q + 4 (j & 1) + e, so that lane (l15, lq = q) owns, per tile row, channels [8 lq, 8 lq + 8) of
// each of the two 32-channel groups: 16 B of hi halves and 16 B of lo' halves per group in the split row format.
__device__ __forceinline__ int swap_channel(int w) {
    const int j = w >> 4, q = (w >> 2) & 3, e = w & 3;
    return 32 * (j >> 1) + 8 * q + 4 * (j & 1) + e;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Straight from the accumulators to split rows -- no LDS staging (the staged epilogue moves 128 KB per tile through ds_write_b32 at
// 64 B/clk: ~2000 cycles, plus the read-back) and packed arithmetic: per pair of outputs v_pk_mul/add (affine), 2 v_max (ReLU),
// v_cvt_pk_f16_f32 (hi), v_pk_mul (x 2^11), v_pk_fma (hi * -2^11 + o * 2^11: the exact difference, already scaled), v_cvt_pk (lo').
// Same values as conv_epilogue_rows8, bit for bit: o - hi and the scaling by 2^11 are exact in fp32, so the fused form rounds once,
// where the unfused one did not round at all.  Range check: s = fma(v, 0, s) stays 0 unless an accumulator is inf or NaN.
// out_mode 0, split output; residual none or in the split format (res_mode 1: same row; 2: the coarser level's row); ReLU mask
// (training: the data gradient gated by the forward activation) none or in the split format.
// out_mode 1 (SPATIAL instantiation; round 4): the ConvTranspose 2x2 s2 of the mask head as a 1x1 conv to (tap, co) = 4 x C2 channels -- a wave's
// 64 columns lie inside ONE tap (C2 % 64 == 0), tile row m = input pixel (b, oy, ox) goes to output pixel (b, 2 oy + ky, 2 ox + kx), a row of C2
// channels: the same 16-B stores at another row address, so the 1.6-GB tensor of a training step no longer takes the staged epilogue's trip
// through LDS (1048 us at 1.96 TB/s before).
// MBR row blocks of 16 per wave tile (4: the 64 x 64 wave tiles of conv_split_kernel; 2: conv3x3_c64_kernel); mrow_in[i] + (nothing): the GEMM row of
// this lane in row block i (any value >= a.M: not stored) -- consecutive rows for the GEMM tiles, rows of a 2-D pixel patch for the patch kernel
// AFFINE_LDS: scale / shift come from LDS copies indexed by the channel relative to nrel0 (conv1x1_nloop_kernel: a global load between two K-steps
// would wait for the ring's prefetched tiles -- vector-memory operations retire in order)
// PLAIN: the layer has neither residual nor mask, known at compile time -- behind a RUN-TIME "has residual" branch the compiler waits for the branch's
// loads with vmcnt(0) at the join, on both paths, which inside conv1x1_nloop_kernel's loop would drain the ring at every tile
template <bool SPATIAL, bool CHECK, int MBR, bool AFFINE_LDS = false, bool PLAIN = false>
__device__ __forceinline__ void conv_epilogue_direct_rows(const ConvArgs& a, f32x4 (&acc)[MBR][4], int lane, const int (&mrow_in)[MBR], int nw0,
                                                          const float* lsc = nullptr, const float* lsh = nullptr, int nrel0 = 0) {
    const int lq = lane >> 4;
    const bool has_res = !PLAIN && a.res_mode != 0, has_mask = !PLAIN && a.mask != nullptr;
    const bool deconv = SPATIAL && a.out_mode == 1;
    const int C2 = a.Cout >> 2;
    const int tap = deconv ? nw0 / C2 : 0, ncol0 = deconv ? nw0 - tap * C2 : nw0;      // column of this wave inside an output row
    const int yld = deconv ? C2 : a.Cout;                                              // floats per output row
    f32x2 sc[2][4], sh[2][4];
    size_t colb[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int n = nw0 + 32 * g + 8 * lq;
        const int nc = ncol0 + 32 * g + 8 * lq;
        colb[g] = (size_t)(nc >> 5) * 128 + (size_t)(nc & 31) * 2;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if constexpr (AFFINE_LDS) {
                const int nr = nrel0 + 32 * g + 8 * lq + 2 * p;
                sc[g][p] = f32x2{lsc[nr], lsc[nr + 1]};
                sh[g][p] = f32x2{lsh[nr], lsh[nr + 1]};
            } else {
                sc[g][p] = a.scale ? f32x2{a.scale[n + 2 * p], a.scale[n + 2 * p + 1]} : f32x2{1.f, 1.f};
                sh[g][p] = a.shift ? f32x2{a.shift[n + 2 * p], a.shift[n + 2 * p + 1]} : f32x2{0.f, 0.f};
            }
        }
    }
    f32x2 chk = {0.f, 0.f};
    // The residual rows of ALL four row groups are requested before the first store: y and res may alias as far as the compiler knows, so
    // it keeps a group's loads behind the previous group's stores -- and loads return in order BEHIND older stores (one vmcnt queue), so
    // every group paid a store round trip plus a load round trip.  The 64 registers are the cross-term accumulators', dead since the fold.
    f16x8 rha[MBR][2], rla[MBR][2];
#ifdef AMP_NO_HOIST
    constexpr bool HOIST = false;
#else
    constexpr bool HOIST = true;
#endif
    auto load_res = [&](int i) {
        {
            const unsigned int m = min((unsigned int)mrow_in[i], (unsigned int)(a.M - 1));
            size_t rrow = (size_t)m * a.Cout;
            if (SPATIAL && a.res_mode == 2) {
                unsigned int b, oy, ox;
                conv_pixel(a, m, b, oy, ox);
                rrow = ((size_t)(b * (a.Ho >> 1) + (oy >> 1)) * (a.Wo >> 1) + (ox >> 1)) * a.Cout;
            }
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const char* rb = reinterpret_cast<const char*>(a.res + rrow) + colb[g];
                rha[i][g] = *reinterpret_cast<const f16x8*>(rb);
                rla[i][g] = *reinterpret_cast<const f16x8*>(rb + 64);
            }
        }
    };
    if (has_res && HOIST) {
#pragma unroll
        for (int i = 0; i < MBR; ++i) load_res(i);
    }
    // the same for the gating activation (training: data gradients): all four row groups up front
    f16x8 mha[MBR][2], mla[MBR][2];
    auto load_mask = [&](int i) {
        const unsigned int m = min((unsigned int)mrow_in[i], (unsigned int)(a.M - 1));
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const char* mb = reinterpret_cast<const char*>(a.mask + (size_t)m * a.Cout) + colb[g];
            mha[i][g] = *reinterpret_cast<const f16x8*>(mb);
            mla[i][g] = *reinterpret_cast<const f16x8*>(mb + 64);
        }
    };
    if (has_mask && HOIST) {
#pragma unroll
        for (int i = 0; i < MBR; ++i) load_mask(i);
    }
#pragma unroll
    for (int i = 0; i < MBR; ++i) {
        const int mrow = mrow_in[i];
        const bool mv = mrow < a.M;
        const unsigned int m = min((unsigned int)mrow, (unsigned int)(a.M - 1));
        size_t yrow = (size_t)m * a.Cout;
        if (deconv) {
            unsigned int b, oy, ox;
            conv_pixel(a, m, b, oy, ox);
            yrow = (((size_t)b * 2 * a.Ho + 2 * oy + (tap >> 1)) * (2 * a.Wo) + 2 * ox + (tap & 1)) * (size_t)yld;
        }
        f16x8 rh[2], rl[2], mh[2], ml[2];
        if (has_res) {
            if (!HOIST) load_res(i);
#pragma unroll
            for (int g = 0; g < 2; ++g) { rh[g] = rha[i][g]; rl[g] = rla[i][g]; }
        }
        if (has_mask) {                                  // the gating activation (training), split rows indexed like y
            if (!HOIST) load_mask(i);
#pragma unroll
            for (int g = 0; g < 2; ++g) { mh[g] = mha[i][g]; ml[g] = mla[i][g]; }
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f16x8 hi, lo;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const f32x4& blk = acc[i][2 * g + (p >> 1)];
                const f32x2 v = {blk[2 * (p & 1)], blk[2 * (p & 1) + 1]};
                if (CHECK) chk = __builtin_elementwise_fma(v, f32x2{0.f, 0.f}, chk);
                f32x2 o = v * sc[g][p] + sh[g][p];
                if (has_res) {
                    const f32x2 r1 = {(float)rh[g][2 * p], (float)rh[g][2 * p + 1]};
                    const f32x2 r2 = {(float)rl[g][2 * p], (float)rl[g][2 * p + 1]};
                    o = o + (r1 + r2 * (1.0f / LO_SCALE));
                }
                if (a.relu) { o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f); }
                if (has_mask) {
                    const f32x2 mk = f32x2{(float)mh[g][2 * p], (float)mh[g][2 * p + 1]} + f32x2{(float)ml[g][2 * p], (float)ml[g][2 * p + 1]} * (1.0f / LO_SCALE);
                    o[0] = mk[0] > 0.f ? o[0] : 0.f;
                    o[1] = mk[1] > 0.f ? o[1] : 0.f;
                }
                const f16x2 h = __builtin_convertvector(o, f16x2);
                const f32x2 hf = {(float)h[0], (float)h[1]};
                const f32x2 l = __builtin_elementwise_fma(hf, f32x2{-LO_SCALE, -LO_SCALE}, o * LO_SCALE);
                const f16x2 lh = __builtin_convertvector(l, f16x2);
                hi[2 * p] = h[0]; hi[2 * p + 1] = h[1];
                lo[2 * p] = lh[0]; lo[2 * p + 1] = lh[1];
            }
            if (mv) {
                char* base = reinterpret_cast<char*>(a.y + yrow) + colb[g];
                *reinterpret_cast<f16x8*>(base) = hi;
                *reinterpret_cast<f16x8*>(base + 64) = lo;
            }
        }
    }
    if (CHECK && (!(chk[0] == 0.f) || !(chk[1] == 0.f))) atomicOr(a.range_flag, 1);
}

template <bool SPATIAL, bool CHECK>
__device__ __forceinline__ void conv_epilogue_direct(const ConvArgs& a, f32x4 (&acc)[4][4], int lane, int mw0, int nw0) {
    const int l15 = lane & 15;
    const int mrows[4] = {mw0 + l15, mw0 + 16 + l15, mw0 + 32 + l15, mw0 + 48 + l15};
    conv_epilogue_direct_rows<SPATIAL, CHECK, 4>(a, acc, lane, mrows, nw0);
}

// The staged epilogues (fp32 output, mask, scatter modes) behind the role-swapped MFMA: only the staging indices differ.
template <int WTM, int WTN, bool SPATIAL, bool CHECK>
__device__ __forceinline__ void conv_epilogue_swapped(const ConvArgs& a, f32x4 (&acc)[4][4], float* lds, int wave, int lane, int mw0, int nw0) {
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr int SLD = WTN + 4;
    float* stage = lds + wave * (WTM * SLD);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(stage + (i * 16 + l15) * SLD + 32 * (j >> 1) + 8 * lq + 4 * (j & 1)) = acc[i][j];
    if (a.y_split && !a.mask && a.out_mode == 0) conv_epilogue_rows8<WTM, WTN, SPATIAL, CHECK>(a, stage, lane, mw0, nw0);
    else conv_epilogue_rows<WTM, WTN, SPATIAL, CHECK>(a, stage, lane, mw0, nw0);
}

// rows of a wave's staged [WTM][WTN] tile -> affine, residual, ReLU, mask -> y (fp32 or split rows)
template <int WTM, int WTN, bool SPATIAL, bool CHECK>
__device__ __forceinline__ void conv_epilogue_rows(const ConvArgs& a, float* stage, int lane, int mw0, int nw0) {
    constexpr int SLD = WTN + 4;
    constexpr int F4R = WTN / 4;
    constexpr int RPI = 64 / F4R;
    constexpr int NIT = WTM / RPI;

    const int erow = lane / F4R;
    const int ec4 = lane % F4R;
    const int n = nw0 + ec4 * 4;
    const bool nv = n < a.Cout;                        // Cout % 4 == 0: the whole float4 is in range or none of it
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (nv) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (a.scale) sc[q] = a.scale[n + q];
            if (a.shift) sh[q] = a.shift[n + q];
        }
    }
    const bool full = __builtin_amdgcn_readfirstlane(mw0) + WTM <= a.M && __builtin_amdgcn_readfirstlane(nw0) + WTN <= a.Cout;
    const bool has_res = a.res_mode != 0, has_mask = a.mask != nullptr;

    size_t yoff[NIT], roff[NIT];
    if (!SPATIAL) {
        const size_t step = (size_t)RPI * a.Cout;
        yoff[0] = (size_t)(mw0 + erow) * a.Cout + n;
#pragma unroll
        for (int it = 1; it < NIT; ++it) yoff[it] = yoff[it - 1] + step;
#pragma unroll
        for (int it = 0; it < NIT; ++it) roff[it] = yoff[it];
    } else {
        const int C2 = a.Cout >> 2;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const unsigned int m = min((unsigned int)(mw0 + it * RPI + erow), (unsigned int)(a.M - 1));   // clamped rows are never stored
            unsigned int b, oy, ox;
            conv_pixel(a, m, b, oy, ox);
            roff[it] = (a.res_mode == 2) ? ((size_t)(b * (a.Ho >> 1) + (oy >> 1)) * (a.Wo >> 1) + (ox >> 1)) * a.Cout + n
                                         : (size_t)m * a.Cout + n;
            if (a.out_mode == 1) {
                const int kk = n / C2;
                const int co = n - kk * C2;
                yoff[it] = ((size_t)(b * 2 * a.Ho + 2 * oy + (kk >> 1)) * (2 * a.Wo) + 2 * ox + (kk & 1)) * C2 + co;
            } else if (a.out_mode == 2) {
                yoff[it] = ((size_t)(b * 2 * a.Ho + 2 * oy) * (2 * a.Wo) + 2 * ox) * a.Cout + n;
            } else {
                yoff[it] = (size_t)m * a.Cout + n;
            }
        }
    }

    auto body = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        bool mv[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) mv[it] = FULL || (nv && mw0 + it * RPI + erow < a.M);
        f32x4 rres[NIT], mk[NIT];
        if (has_res && a.res_split) {
            // the residual tensor lives in the split row format: this lane's 4 channels are 8 B of hi halves and 8 B of lo' halves
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                if (mv[it]) {
                    const char* rb = reinterpret_cast<const char*>(a.res + (roff[it] - (size_t)n)) + (n >> 5) * 128 + (n & 31) * 2;
                    const f16x4 rh = *reinterpret_cast<const f16x4*>(rb);
                    const f16x4 rl = *reinterpret_cast<const f16x4*>(rb + 64);
#pragma unroll
                    for (int q = 0; q < 4; ++q) rres[it][q] = fold((float)rh[q], (float)rl[q]);
                }
        } else if (has_res) {
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                if (mv[it]) rres[it] = *reinterpret_cast<const f32x4*>(a.res + roff[it]);
        }
        if (has_mask && a.mask_split) {
            // the activation whose sign gates the gradient lives in the split row format (training on the native trunk): decoded like a
            // split residual; hi + lo' * 2^-11 > 0 exactly when the stored activation was (down to 2^-35, below which both halves are 0)
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                if (mv[it]) {
                    const char* mb = reinterpret_cast<const char*>(a.mask + (yoff[it] - (size_t)n)) + (n >> 5) * 128 + (n & 31) * 2;
                    const f16x4 mh = *reinterpret_cast<const f16x4*>(mb);
                    const f16x4 ml = *reinterpret_cast<const f16x4*>(mb + 64);
#pragma unroll
                    for (int q = 0; q < 4; ++q) mk[it][q] = fold((float)mh[q], (float)ml[q]);
                }
        } else if (has_mask) {
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                if (mv[it]) mk[it] = *reinterpret_cast<const f32x4*>(a.mask + yoff[it]);
        }
        __builtin_amdgcn_wave_barrier();               // staging writes of this wave precede its reads (same-wave LDS order)
        bool bad = false;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(stage + (it * RPI + erow) * SLD + ec4 * 4);
            if (CHECK) bad = bad || !(fabsf(v[0]) <= 3.0e38f) || !(fabsf(v[1]) <= 3.0e38f) || !(fabsf(v[2]) <= 3.0e38f) || !(fabsf(v[3]) <= 3.0e38f);
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float t = __fadd_rn(__fmul_rn(v[q], sc[q]), sh[q]);
                if (has_res) t = __fadd_rn(t, rres[it][q]);
                if (a.relu) t = fmaxf(t, 0.f);
                if (has_mask) t = mk[it][q] > 0.f ? t : 0.f;
                o[q] = t;
            }
            if (a.y_split) {
                // row-relative: 32 channels = 64 B of hi halves + 64 B of lo' halves; this lane's 4 channels -> 8 B in each
                if (mv[it]) {
                    f16x4 hi, lo;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const _Float16 h = (_Float16)o[q];
                        hi[q] = h;
                        lo[q] = (_Float16)((o[q] - (float)h) * LO_SCALE);
                    }
                    const size_t row = yoff[it] - (size_t)n;                     // float index of the row start
                    char* base = reinterpret_cast<char*>(a.y + row) + (n >> 5) * 128 + (n & 31) * 2;
                    *reinterpret_cast<f16x4*>(base) = hi;
                    *reinterpret_cast<f16x4*>(base + 64) = lo;
                }
            } else if (mv[it]) {
                *reinterpret_cast<f32x4*>(a.y + yoff[it]) = o;
            }
        }
        if (CHECK && bad) atomicOr(a.range_flag, 1);
    };
    if (full) body(std::true_type{});
    else body(std::false_type{});
}

}  // namespace
