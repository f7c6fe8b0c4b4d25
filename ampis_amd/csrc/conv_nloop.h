// conv1x1_nloop_kernel: several N tiles per workgroup for short-K 1x1 layers.  EXPERIMENT, default off (AMP_NLOOP).
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// conv1x1_nloop_kernel (round 4): the short-K 1x1 layers that run one 128 x 256 tile per CU (stride-2 shortcuts, conv1 of a stage's first block, their
// data gradients, the mask head's deconv in a training step: K = 64 ... 512, two to sixteen K-steps) with SEVERAL N tiles of a 128-pixel block in one
// workgroup -- mask_tail_kernel's loop with conv_epilogue_direct_rows as the tile epilogue.  A workgroup of conv_split_kernel pays a cold ring, a prologue and
// an epilogue per tile for 5 us of MFMA work (K = 256); here the ring runs on across the tiles (tile t + 1's first weight tiles and the pixel block's rows,
// now in the L2, are requested during tile t's last steps) and a half's epilogue -- loads of residual / mask, 16 stores per wave -- sits between two steps.
// Those stores are YOUNGER than the requests already in flight, so the counted wait in front of a step allows for them exactly where they are in the queue:
//   early half (epilogue after the last MFMAs of step e):   step e + 1 needs D(e+1); younger: D(e+2), E      -> vmcnt(6 + 16)
//                                                            step e + 2 needs D(e+2); younger: E, D(e+3)      -> vmcnt(6 + 16)
//   late half  (epilogue in step e + 1, before its requests): step e + 1 needs D(e+1); younger: D(e+2)         -> vmcnt(6)
//                                                            step e + 2 needs D(e+2); younger: E, D(e+3)      -> vmcnt(6 + 16)
// and vmcnt(6) from then on (which also retires E).  16 is a LOWER bound on a full tile's stores (more younger operations only make the wait stricter);
// a partial tile (rows beyond M: stores skipped) waits with vmcnt(6).  Same products, same order, same epilogue: bit-identical to conv_split_kernel.
// ------------------------------------------------------------------------------------------------------------------
template <bool SPATIAL>
__global__ __launch_bounds__(512, 1) void conv1x1_nloop_kernel(const ConvArgs a, const unsigned int x_bytes, const unsigned int w_bytes, const int NT) {
    constexpr int BM = 128, BN = 256, NW = 8, GA = 2, GB = 4, NDMA = GA + GB, NST = 16;
    constexpr int TILE_FLOATS = (BM + BN) * BK;
    constexpr int NT_MAX = 8;                      // scale + shift of NT_MAX * 256 channels: the 16 KB behind the ring
    __shared__ __attribute__((aligned(16))) float lds[3 * TILE_FLOATS + 2 * NT_MAX * BN];
    float* lsc = lds + 3 * TILE_FLOATS;
    float* lsh = lsc + NT_MAX * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int l15 = lane & 15, lq = lane >> 4;
    const int ngrp = a.ntn / NT;                   // groups of NT consecutive N tiles
    const int wg = amp::xcd_remap(blockIdx.x, a.nblk);
    const int grp = wg % ngrp;
    const int m0 = (wg / ngrp) * BM;
    const int n_first = grp * NT * BN;
    const bool full = m0 + BM <= a.M;
    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);
    const int srow = dma_row(lane), spos = dma_pos(lane);
    unsigned int a_voff[GA], b_voff[GB];
#pragma unroll
    for (int g = 0; g < GA; ++g) {
        const int r = wave * (BM / NW) + 8 * g + srow;
        const int m = m0 + r;
        a_voff[g] = OOB_VOFF;
        if (m < a.M) {                             // 1x1, pad 0: output pixel (b, oy, ox) reads input pixel (oy, ox) * stride
            unsigned int b, oy, ox;
            conv_pixel(a, (unsigned int)m, b, oy, ox);
            a_voff[g] = (unsigned int)((((size_t)(b * a.H + oy * a.stride) * a.W + ox * a.stride) * a.Cin + dma_chunk(spos, r)) * 4);
        }
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int r = wave * (BN / NW) + 8 * g + srow;
        const int n = n_first + (r & ~63) + swap_channel(r & 63);
        b_voff[g] = (unsigned int)(((size_t)n * a.K + dma_chunk(spos, r)) * 4);
    }
    const int csteps = a.Cin / BK;                 // K-steps per tile
    const int total = NT * csteps;
    const int tile_bytes = BN * a.K * 4;           // weight rows of one N tile
    int s_cs = 0, s_tile = 0;                      // the step being STAGED
    auto stage = [&](int buf) {
        float* As = lds + buf * TILE_FLOATS;
        float* Bs = As + BM * BK;
        const int a_soff = s_cs * (BK * 4);
        const int b_soff = s_tile * tile_bytes + s_cs * (BK * 4);
#pragma unroll
        for (int g = 0; g < GA; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(As + (wave * (BM / NW) + 8 * g) * BK), 16, (int)a_voff[g], a_soff, 0, 0);
#pragma unroll
        for (int g = 0; g < GB; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bs + (wave * (BN / NW) + 8 * g) * BK), 16, (int)b_voff[g], b_soff, 0, 0);
        if (++s_cs == csteps) { s_cs = 0; ++s_tile; }
    };
    f32x4 acc[4][4], acx[4][4];
    zero_acc(acc, acx);
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));
    stage(0);
    stage(1);
    // FrozenBN scale / shift (or 1 / bias) of the group's channels: once, into LDS (visible behind the first step's barrier)
    for (int c = tid; c < NT * BN; c += 512) {
        lsc[c] = a.scale ? a.scale[n_first + c] : 1.0f;
        lsh[c] = a.shift ? a.shift[n_first + c] : 0.0f;
    }
    const int mw0 = m0 + wm * 64;
    const bool scaled_in = a.out_scale != 1.0f;
    auto tile_epilogue = [&](int tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[i][j][e] = fold(acc[i][j][e], acx[i][j][e]);
                    if (scaled_in) acc[i][j][e] *= a.out_scale;
                }
        // one 16-row block at a time: the loop's state stays live across this epilogue, and two blocks' hoisted residual / mask rows beside it spill
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mrows[1] = {mw0 + 16 * i + l15};
            conv_epilogue_direct_rows<SPATIAL, true, 1, true, true>(a, reinterpret_cast<f32x4 (&)[1][4]>(acc[i]), lane, mrows, n_first + tile * BN + wn * 64, lsc, lsh, tile * BN + wn * 64);
        }
    };
    int cur = 0, nxt = 2, c_cs = 0, c_tile = 0;    // ring positions; the step being COMPUTED
    const bool early = wave < NW / 2;
    auto open_step = [&](int step) {
        // the stores of the previous tile's epilogue in the queue (see the table above); exact for full tiles only
        const bool behind_epilogue = full && c_tile > 0 && (early ? c_cs <= 1 : c_cs == 1);
        if (step + 1 >= total) __builtin_amdgcn_s_waitcnt(0x0070);
        else if (behind_epilogue) __builtin_amdgcn_s_waitcnt(0x0070 | ((NDMA + NST) & 15) | (((NDMA + NST) >> 4) << 14));
        else __builtin_amdgcn_s_waitcnt(0x0070 | NDMA);
        ring_barrier();
    };
    auto advance = [&]() {
        ring_next<3>(cur, nxt);
        if (++c_cs == csteps) { c_cs = 0; ++c_tile; }
    };
    F16x3Frags<4, 4> fr;
    const float* As0 = lds + (wm * 64 + l15) * BK;
    const float* Bs0 = lds + BM * BK + (wn * 64 + l15) * BK;
    if (early) {
        for (int step = 0; step < total; ++step) {
            open_step(step);
            f16x3_load16<4, 4>(As0 + cur * TILE_FLOATS, Bs0 + cur * TILE_FLOATS, fo16_hi, fo16_lo, fr);
            __builtin_amdgcn_sched_barrier(0);
            if (step + 2 < total) stage(nxt);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
            f16x3_mfma16<4, 4, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            if (c_cs == csteps - 1) { tile_epilogue(c_tile); zero_acc(acc, acx); __builtin_amdgcn_sched_barrier(0); }
            advance();
        }
    } else {
        for (int step = 0; step < total; ++step) {
            open_step(step);
            __builtin_amdgcn_s_setprio(1);
            if (step > 0) f16x3_mfma16<4, 4, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            if (c_cs == 0 && c_tile > 0) { tile_epilogue(c_tile - 1); zero_acc(acc, acx); __builtin_amdgcn_sched_barrier(0); }      // the MFMAs above finished tile c_tile - 1
            __builtin_amdgcn_s_barrier();
            f16x3_load16<4, 4>(As0 + cur * TILE_FLOATS, Bs0 + cur * TILE_FLOATS, fo16_hi, fo16_lo, fr);
            __builtin_amdgcn_sched_barrier(0);
            if (step + 2 < total) stage(nxt);
            __builtin_amdgcn_sched_barrier(0);
            advance();
        }
        f16x3_mfma16<4, 4, true>(fr, acc, acx);
        tile_epilogue(NT - 1);
    }
}

}  // namespace
