// conv_f16x3_kernel: fp32 activations split on the VALU, f16 matrix pipe; split8.
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// conv_f16x3_kernel (amp_set_conv_mode(ctx, AMP_CONV_F16X3)): the same implicit GEMM on the f16 matrix pipe, fp32 in / fp32 out.
// Every operand x is split as x = hi + lo with hi = f16(x) and lo = x - hi (exact in fp32); the low half is stored as
// lo' = f16(lo * 2^11), which has the magnitude of hi, so it stays a normal f16 number however small x is (22 significant bits
// down to |x| ~ 2^-25; a plain f16(lo) would go subnormal below |x| = 0.125).  a*b ~= a_hi*b_hi + (a_hi*b_lo' + a_lo'*b_hi) * 2^-11,
// every product an exact-product v_mfma_f32_32x32x16_f16 accumulated in fp32, the cross terms in their own accumulators that
// the epilogue folds in with one exact scaling (the dropped a_lo*b_lo term is < 2^-22 |a*b|): 3 MFMAs of 32 cycles do the work
// of 8 fp32 MFMAs of 64 cycles (5.3x the fp32 matrix rate).
// Weights are split once (split_weights_kernel: per K-step of 32 a row holds 64 B of hi halves then 64 B of lo' halves) and
// staged by LDS-DMA exactly like the fp32 kernel; activations stay fp32 in HBM, are fetched with bounds-checked buffer loads
// (zero fill outside the image) one K-step ahead into registers, split on the VALU and written to LDS in the same hi|lo' row
// format.  Range: |operand| must stay below 65504 (fp16 max) -- checked: a violation makes an accumulator non-finite, the
// epilogue raises ctx->d_conv_flag and the caller re-runs in fp32; the fp32 kernel has no such limit.
// ------------------------------------------------------------------------------------------------------------------

template <bool SCALED>
__device__ __forceinline__ void split8(const f32x4& v0, const f32x4& v1, f16x8& hi, f16x8& lo, float in_scale) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float x = j < 4 ? v0[j] : v1[j - 4];
        if (SCALED) x *= in_scale;
        const _Float16 h = (_Float16)x;
        hi[j] = h;
        lo[j] = (_Float16)((x - (float)h) * LO_SCALE);
    }
}

// STEM = true: the 7x7 stride-2 stem on the [B,H,W,4] input with weights [64][7][8][4] (see conv_glds_kernel): a K-step is one
// kernel row, a lane's 8 consecutive k are two taps x 4 channels, each tap bounds-checked on its own.
// SCALED = true: activations are multiplied by a.in_scale before the split and the result by a.out_scale (powers of two, exact).
// The data-gradient convolutions use it: loss gradients of 1e-9..1e-4 would sit in the f16 subnormals (the hi half keeps 11 bits
// only above 6.1e-5); scaled by 2^16 they split like activations.
// BN = 256 runs 8 waves (2 x 4, one workgroup per CU): the activation tile is fetched and split once for 256 output channels, so a
// wave carries half the split work and half the activation loads per MFMA of the 4-wave tiles.
template <int BN, int EPI, bool STEM = false, bool SCALED = false>
__global__ __launch_bounds__(BN == 256 ? 512 : 256, BN == 256 ? 1 : 2) void conv_f16x3_kernel(const ConvArgs a, const unsigned int x_bytes,
                                                                                                const unsigned int w_bytes) {
    constexpr int BM = 128;
    constexpr int WTM = BM / 2, WTN = (BN == 64) ? 32 : 64;
    constexpr int NWN = BN / WTN, NW = 2 * NWN;   // waves across N, waves per workgroup
    constexpr int RPT = 512 / (64 * NW);  // activation rows per lane (128 rows x 4 lanes per row over the workgroup)
    constexpr int GB = BN / NW / 8;       // DMA instructions per wave per step for B: BN/NW rows per wave, 8 rows each
    constexpr int TILE_FLOATS = (BM + BN) * BK;   // a row = 32 k = 64 B hi halves + 64 B lo halves = 32 dwords, as in the fp32 kernel
    constexpr int SLD = WTN + 4;
    constexpr int STAGE_FLOATS = NW * WTM * SLD;
    constexpr int LDS_FLOATS = (2 * TILE_FLOATS > STAGE_FLOATS) ? 2 * TILE_FLOATS : STAGE_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;

    const int tile = amp::xcd_remap(blockIdx.x, a.nblk);
    const int tile_n = tile % a.ntn;
    const int tile_m = tile / a.ntn;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;
    const int HoWo = a.Ho * a.Wo;

    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);

    // ---- A (activations): lane = 4 * (row in a 16-row group) + kg; a lane owns 8 consecutive k (32 B) of rows ra[0], ra[1] ----
    const int arow = lane >> 2, akg = lane & 3;
    int a_iy0[RPT], a_ix0[RPT], a_pb[RPT], a_row[RPT];
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        const int r = p * 64 + wave * 16 + arow;
        a_row[p] = r;
        const int m = m0 + r;
        if (m < a.M) {
            const unsigned int b = fastdiv((unsigned int)m, a.div_howo_mul, a.div_howo_shr);
            const unsigned int rem = (unsigned int)m - b * (unsigned int)HoWo;
            const unsigned int oy = fastdiv(rem, a.div_wo_mul, a.div_wo_shr);
            const unsigned int ox = rem - oy * (unsigned int)a.Wo;
            a_iy0[p] = (int)oy * a.stride - a.pad;
            a_ix0[p] = (int)ox * a.stride - a.pad;
            a_pb[p] = (int)b * a.H * a.W;
        } else {
            a_iy0[p] = -(1 << 28);
            a_ix0[p] = 0;
            a_pb[p] = 0;
        }
    }
    // ---- B (split weights): LDS-DMA, 8 rows x 128 B per wave-instruction, source chunk XOR-swizzled ----
    const int srow = dma_row(lane), spos = dma_pos(lane);
    unsigned int b_voff[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int r = wave * (BN / NW) + 8 * g + srow;
        const int n = n0 + r;
        b_voff[g] = (n < a.Cout) ? (unsigned int)(((size_t)n * a.K + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }

    const int csteps = STEM ? 1 : a.cin_win / BK;
    const int a_win = a.grouped ? n0 * 4 : 0;   // bytes: first input channel of this N tile's window (grouped conv, BN = 64 only)
    int ky = 0, kx = 0, cs = 0, kstep = 0;     // block-uniform state of the K-step being FETCHED
    unsigned int a_voff[RPT];
    u32x4 ra[RPT][2];                             // fetched, not yet split: [row][half of the 32 B]

    auto fetch = [&](int buf) {                 // A(kstep) -> registers, B(kstep) -> LDS[buf]
        if (STEM) {
#pragma unroll
            for (int p = 0; p < RPT; ++p) {
                const int iy = a_iy0[p] + kstep;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int ix = a_ix0[p] + 2 * akg + h;
                    const bool v = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                    const unsigned int vo = v ? (unsigned int)((a_pb[p] + iy * a.W + ix) * 16) : OOB_VOFF;
                    ra[p][h] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)vo, 0, 0);
                }
            }
        } else if (cs == 0) {
#pragma unroll
            for (int p = 0; p < RPT; ++p) {
                const int iy = a_iy0[p] + ky, ix = a_ix0[p] + kx;
                const bool v = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                a_voff[p] = v ? (unsigned int)(((a_pb[p] + iy * a.W + ix) * a.Cin + 8 * akg) * 4) : OOB_VOFF;
            }
        }
        const int a_soff = cs * (BK * 4) + a_win;
        const int b_soff = kstep * (BK * 4);
        if (!STEM) {
#pragma unroll
            for (int p = 0; p < RPT; ++p) {
                ra[p][0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)a_voff[p], a_soff, 0);
                ra[p][1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)a_voff[p] + 16, a_soff, 0);
            }
        }
        float* Bs = lds + buf * TILE_FLOATS + BM * BK;
#pragma unroll
        for (int g = 0; g < GB; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bs + (wave * (BN / NW) + 8 * g) * BK),
                                                     16, (int)b_voff[g], b_soff, 0, 0);
        ++kstep;
        if (++cs == csteps) {
            cs = 0;
            if (++kx == a.KW) { kx = 0; ++ky; }
        }
    };
    auto commit = [&](int buf) {                // split the fetched A registers into LDS[buf]
        float* As = lds + buf * TILE_FLOATS;
#pragma unroll
        for (int p = 0; p < RPT; ++p) {
            f16x8 hi, lo;
            split8<SCALED>(__builtin_bit_cast(f32x4, ra[p][0]), __builtin_bit_cast(f32x4, ra[p][1]), hi, lo, a.in_scale);
            const int r = a_row[p], sw = (r >> 1) & 7;
            *reinterpret_cast<f16x8*>(As + r * BK + 4 * (akg ^ sw)) = hi;
            *reinterpret_cast<f16x8*>(As + r * BK + 4 * ((4 + akg) ^ sw)) = lo;
        }
    };

    constexpr int MB = WTM / 16, NB = WTN / 16;
    f32x4 acc[MB][NB], acx[MB][NB];        // hi*hi sums; cross-term sums (scaled by 2^11): blocks of 16 x 16 (f16x3_step16)
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[i][j][e] = 0.f; acx[i][j][e] = 0.f; }

    const int l15 = lane & 15, lq = lane >> 4;
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));

    fetch(0);
    commit(0);
    __builtin_amdgcn_s_waitcnt(0x0F70);     // B(0) has landed (see the loop)
    __syncthreads();
    if (a.nsteps > 1) fetch(1);

    for (int step = 0; step < a.nsteps; ++step) {
        const int cur = step & 1;
        f16x3_step16<MB, NB>(lds + cur * TILE_FLOATS + (wm * WTM + l15) * BK, lds + cur * TILE_FLOATS + BM * BK + (wn * WTN + l15) * BK,
                             fo16_hi, fo16_lo, acc, acx);
        // A(step+1) is in registers (loads issued a step ago, behind the previous barrier), B(step+1) is landing in LDS[cur^1]
        if (step + 1 < a.nsteps) commit(cur ^ 1);
        // The weight DMA into LDS[cur^1] must have LANDED before anyone reads it.  The compiler only counts the register loads of
        // fetch() (it emitted vmcnt(2..3) here and no vmcnt(0) at the barrier: a race that showed up as soon as the weights were
        // cold in L2), so the wait is explicit: vmcnt(0), other counters untouched.
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();   // LDS[cur] is free, LDS[cur^1] complete
        if (step + 2 < a.nsteps) fetch(cur);    // A(step+2) -> registers, B(step+2) -> LDS[cur]
    }

    // fold the cross terms in (their 2^-11 is exact), then the shared epilogue
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[i][j][e] = fold(acc[i][j][e], acx[i][j][e]);
                if (SCALED) acc[i][j][e] *= a.out_scale;
            }
    if (EPI == 0) conv_epilogue16<WTM, WTN, MB, NB, true>(a, acc, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN, HoWo);
    else conv_epilogue_fast16<WTM, WTN, MB, NB, EPI == 2, true>(a, acc, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN);
}

}  // namespace
