// conv_split_kernel: both operands in split rows through a ring of LDS buffers; g_stamp and the STAMP_* macros of the lab build.
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"
#include "conv_predict.h"      // EPI 3: conv_epilogue_predict / conv_epilogue_rpn

namespace {

// ------------------------------------------------------------------------------------------------------------------
// conv_split_kernel: AMP_CONV_F16X3 with BOTH operands already in the split hi|lo' row format (the trunk's native activation
// format in inference, and the pre-split weights), 8 waves on a 128x256 or 256x128 tile, one workgroup per CU.
// Compared with conv_glds_kernel<.., F16 = true> (two LDS buffers, vmcnt(0) + barrier at the end of every K-step) the operand
// tiles travel through a ring of THREE LDS buffers: the LDS-DMA of tile s+2 is issued when tile s starts computing, and the wait
// in front of tile s is vmcnt(NDMA) -- everything but the youngest tile's requests.  Why: a K-step is 24 MFMAs per wave
// (1536 cycles per SIMD at two waves per SIMD, ~0.8 us) but an LDS-DMA request needs ~1.1 us from issue to landing when every CU
// streams (MI355X_MICROARCH.md, cost cell "ldsdma-fill"), so with one tile in flight every step ended in a stall on its own
// prefetch; with two in flight the request has two steps to land.  3 x 48 KB = 144 KB of the CU's 160 KB.
// ------------------------------------------------------------------------------------------------------------------
#ifdef AMP_STAMP
// Lab build only (make EXTRA=-DAMP_STAMP): in-kernel phase timing of conv_split_kernel -- cycles per wave slot and phase, summed over
// all workgroups: [wave][0] wait+barrier, [1] DMA issue, [2] fragment reads (issue + return), [3] MFMA issue, [4] whole loop,
// [5] kernel entry -> loop, [6] loop end -> epilogue stores issued, [7] loop end -> past the final barrier.
__device__ unsigned long long g_stamp[8 * 8];
// [0] shader cycles (s_memtime) and [1] 100-MHz ticks (s_memrealtime) around the K loop of wave 0, summed over workgroups: the clock the chip held
// in the loop = [0] / [1] * 100 MHz (MI355X_MICROARCH.md, "DVFS give-back" item 6)
__device__ unsigned long long g_stamp_clk[2];
#define STAMP_T(var) const long long var = clock64()
#define STAMP_ADD(slot, t0, t1) st_acc[slot] += (t1) - (t0)
#else
#define STAMP_T(var)
#define STAMP_ADD(slot, t0, t1)
#endif
// NBP (EPI 3, the fused RPN tail only): blocks of 16 predictor rows -- 1, 2 or 3 (conv_epilogue_rpn_rows)
template <int BM, int BN, int EPI, int NSTAGE = 3, bool CHAN = false, int NBP = 1>
__global__ __launch_bounds__((BM / 64) * (BN / 64) * 64, NSTAGE == 2 ? 2 : 1) void conv_split_kernel(const ConvArgs a, const unsigned int x_bytes,
                                                                                                     const unsigned int w_bytes) {
    constexpr int WTM = 64, WTN = 64;
    constexpr int NWM = BM / WTM, NWN = BN / WTN, NW = NWM * NWN;
    constexpr int MB = WTM / 16, NB = WTN / 16;
    constexpr int GA = BM / NW / 8;       // DMA instructions per wave per K-step for A (8 rows x 128 B each)
    constexpr int GB = BN / NW / 8;       // ... for B
    constexpr int NDMA = GA + GB;
    // NSTAGE = 2 (128 x 128 tiles, byte-bound short-K layers): 68 KB of LDS, 4 waves -> TWO workgroups per CU
    constexpr int TILE_FLOATS = (BM + BN) * BK;
    constexpr int SLD = WTN + 4;
    constexpr int STAGE_FLOATS = NW * WTM * SLD;
    constexpr int LDS_FLOATS = (NSTAGE * TILE_FLOATS > STAGE_FLOATS) ? NSTAGE * TILE_FLOATS : STAGE_FLOATS;
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
    static_assert(GA >= 1 && GB >= 1 && NDMA < 16, "tile / wave split");
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
#ifdef AMP_STAMP
    const long long st_entry = clock64();
#endif

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;

    const int tile = amp::xcd_remap(blockIdx.x, a.nblk);
    const int tile_n = tile % a.ntn;
    const int tile_m = tile / a.ntn;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;

    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);

    // ---- staging geometry (as conv_glds_kernel): instruction g of this wave fills rows wave*R + 8g + (lane>>3), 16-B position lane&7 ----
    const int srow = dma_row(lane), spos = dma_pos(lane);
    int a_iy0[GA], a_ix0[GA], a_pb[GA], a_chunk[GA];
#pragma unroll
    for (int g = 0; g < GA; ++g) {
        const int r = wave * (BM / NW) + 8 * g + srow;
        a_chunk[g] = dma_chunk(spos, r);
        const int m = m0 + r;
        if (m < a.M) {
            unsigned int b, oy, ox;
            conv_pixel(a, (unsigned int)m, b, oy, ox);
            a_iy0[g] = (int)oy * a.stride - a.pad;
            a_ix0[g] = (int)ox * a.stride - a.pad;
            a_pb[g] = (int)b * a.H * a.W;
        } else {
            a_iy0[g] = -(1 << 28);
            a_ix0[g] = 0;
            a_pb[g] = 0;
        }
    }
    unsigned int b_voff[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int r = wave * (BN / NW) + 8 * g + srow;               // LDS row; its weight row follows swap_channel (see conv_epilogue_direct)
        const int n = n0 + (r & ~63) + swap_channel(r & 63);
        b_voff[g] = (n < a.Cout) ? (unsigned int)(((size_t)n * a.K + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }
    unsigned int a_voff[GA];

    const int csteps = a.Cin / BK;
    int ky = 0, kx = 0, cs = 0, kstep = 0;     // block-uniform state of the tile being STAGED

    constexpr bool chan_major = CHAN;      // compile-time: a run-time flag here cost 12 B of scratch and a vmcnt(0) per step (250 VGPRs, 96 SGPRs in use)
    auto stage = [&](int buf) {
        if (cs == 0 || chan_major) {           // the tap changed: new pixel offsets (channel-major: every step)
#pragma unroll
            for (int g = 0; g < GA; ++g) {
                const int iy = a_iy0[g] + ky, ix = a_ix0[g] + kx;
                const bool v = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                a_voff[g] = v ? (unsigned int)(((a_pb[g] + iy * a.W + ix) * a.Cin + a_chunk[g]) * 4) : OOB_VOFF;
            }
        }
        float* As = lds + buf * TILE_FLOATS;
        float* Bs = As + BM * BK;
        const int a_soff = cs * (BK * 4);
        int b_soff;
        if constexpr (chan_major) b_soff = ((ky * a.KW + kx) * csteps + cs) * (BK * 4);
        else b_soff = kstep * (BK * 4);
#pragma unroll
        for (int g = 0; g < GA; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(As + (wave * (BM / NW) + 8 * g) * BK),
                                                     16, (int)a_voff[g], a_soff, 0, 0);
#pragma unroll
        for (int g = 0; g < GB; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bs + (wave * (BN / NW) + 8 * g) * BK),
                                                     16, (int)b_voff[g], b_soff, 0, 0);
        if constexpr (chan_major) {
            if (++kx == a.KW) {
                kx = 0;
                if (++ky == a.KH) { ky = 0; ++cs; }
            }
        } else {
            ++kstep;
            if (++cs == csteps) {
                cs = 0;
                if (++kx == a.KW) { kx = 0; ++ky; }
            }
        }
    };

    f32x4 acc[MB][NB], acx[MB][NB];            // hi*hi sums; cross-term sums (scaled by 2^11): 128 registers
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[i][j][e] = 0.f; acx[i][j][e] = 0.f; }
    const int l15 = lane & 15, lq = lane >> 4;
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));

    stage(0);
    if (a.nsteps > 1) stage(1);
    // fused mask-head tail only: its predictor rows, requested here -- behind the first two tiles' DMA (the class-id load the row addresses
    // wait for must not delay the staging; younger loads in the queue only make the ring's counted vmcnt waits stricter, never looser)
    PredictPrefetch ppf;
    if constexpr (BM == 128 && BN == 256 && EPI == 3) {
        if (NBP == 1 && a.out_mode == 3) ppf = predict_prefetch(a, wave, lane, m0);
    }
    int cur = 0, nxt = 2;                      // ring positions of the tile being computed / staged
    // (lgkmcnt(0) in ring_open: the staggered half issues its fragment reads of tile step-1 last in its step)
    auto open_step = [&](int step) { ring_open<NDMA>(step + 1 < a.nsteps); };
    auto advance = [&]() { ring_next<NSTAGE>(cur, nxt); };
    // Ping-pong between the two waves of a SIMD (MI355X_MICROARCH.md, "Two waves per SIMD"): waves w and w + NW/2 share a SIMD, and run
    // in lockstep they first both issue LDS-DMA and fragment reads (matrix pipe idle) and then both issue MFMAs (pipe contended) -- the
    // in-kernel stamps (tools/stamp_conv.py) gave 2400-2540 cycles per K-step against 1536 of MFMA work.  So the second half of the
    // workgroup runs its MFMAs one step late: a K-step has two halves separated by a second barrier; in the first the early half
    // stages tile s+2 and reads the fragments of tile s while the late half multiplies the fragments of tile s-1 it holds in registers;
    // in the second the early half multiplies tile s while the late half stages and reads.  The multiplying half runs at raised priority.
    // Same tiles, same sums per accumulator in the same order -- bit-identical results (1930-2010 cycles per K-step; +5..14 % per layer).
    F16x3Frags<MB, NB> fr;
#ifdef AMP_STAMP
    long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long st_rt0 = __builtin_amdgcn_s_memrealtime(), st_mt0 = __builtin_amdgcn_s_memtime();
    const long long st_begin = clock64();
#endif
    const float* As0 = lds + (wm * WTM + l15) * BK;
    const float* Bs0 = lds + BM * BK + (wn * WTN + l15) * BK;
    const bool pp = a.stagger != 0;
    if (!pp || wave < NW / 2) {
        for (int step = 0; step < a.nsteps; ++step) {
            STAMP_T(t0);
            open_step(step);
            STAMP_T(t1);
            // fragment reads first: they return while the DMA requests are being issued (~75 cycles each), not in front of the MFMAs
            f16x3_load16<MB, NB>(As0 + cur * TILE_FLOATS, Bs0 + cur * TILE_FLOATS, fo16_hi, fo16_lo, fr);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t2);
            if constexpr (NSTAGE == 2) {
                // two buffers: tile step+2 goes into the buffer of tile `step` itself, once every wave holds its fragments in registers
                if (step + 2 < a.nsteps) {
                    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wave's fragment reads have returned
                    ring_barrier();
                    stage(cur);
                }
            } else
            if (step + 2 < a.nsteps) stage(nxt);   // into the buffer tile step-1 occupied
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t3);
            if (pp) __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
            f16x3_mfma16<MB, NB, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t4);
            STAMP_ADD(0, t0, t1); STAMP_ADD(2, t1, t2); STAMP_ADD(1, t2, t3); STAMP_ADD(3, t3, t4);
            advance();
        }
    } else {
        for (int step = 0; step < a.nsteps; ++step) {
            STAMP_T(t0);
            open_step(step);
            STAMP_T(t1);
            __builtin_amdgcn_s_setprio(1);
            if (step > 0) f16x3_mfma16<MB, NB, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            STAMP_T(t2);
            f16x3_load16<MB, NB>(As0 + cur * TILE_FLOATS, Bs0 + cur * TILE_FLOATS, fo16_hi, fo16_lo, fr);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t3);
            if (step + 2 < a.nsteps) stage(nxt);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t4);
            STAMP_ADD(0, t0, t1); STAMP_ADD(3, t1, t2); STAMP_ADD(2, t2, t3); STAMP_ADD(1, t3, t4);
            advance();
        }
        f16x3_mfma16<MB, NB, true>(fr, acc, acx);
    }
#ifdef AMP_STAMP
    if (wave == 0 && lane == 0) {
        atomicAdd(&g_stamp_clk[0], __builtin_amdgcn_s_memtime() - st_mt0);
        atomicAdd(&g_stamp_clk[1], __builtin_amdgcn_s_memrealtime() - st_rt0);
    }
    st_acc[4] = clock64() - st_begin;
    st_acc[5] = st_begin - st_entry;
    const long long st_loop_end = clock64();
#endif
    __syncthreads();                           // all operand reads done: the epilogue re-uses the buffers as its staging tile
#ifdef AMP_STAMP
    st_acc[7] = clock64() - st_loop_end;
#endif
    const bool scaled_in = a.out_scale != 1.0f;

#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[i][j][e] = fold(acc[i][j][e], acx[i][j][e]);
                if (scaled_in) acc[i][j][e] *= a.out_scale;      // x arrived as split rows of x * 2^shift (a scaled loss gradient): exact power of two
            }
    if constexpr (BM == 128 && BN == 256 && EPI == 3) {          // the fused tails have an instantiation of their own: no row epilogue, no spills
        if (NBP == 1 && a.out_mode == 3) conv_epilogue_predict(a, acc, lds, wave, lane, m0, n0, ppf);
        else conv_epilogue_rpn<NBP>(a, acc, lds, wave, lane, m0, n0);
        return;
    }
    if (a.y_split && (!a.mask || a.mask_split) && (a.out_mode == 0 || (EPI == 2 && a.out_mode == 1 && !a.mask && a.res_mode == 0)) && (a.res_mode == 0 || a.res_split) && a.direct_epi)
        conv_epilogue_direct<EPI == 2, true>(a, acc, lane, m0 + wm * WTM, n0 + wn * WTN);
    else
        conv_epilogue_swapped<WTM, WTN, EPI == 2, true>(a, acc, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN);
#ifdef AMP_STAMP
    st_acc[6] = clock64() - st_loop_end;
    if (lane == 0)
        for (int q = 0; q < 8; ++q) atomicAdd(&g_stamp[wave * 8 + q], (unsigned long long)st_acc[q]);
#endif
}

}  // namespace
