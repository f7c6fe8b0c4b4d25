// conv_glds_kernel: the same tiling with operand staging by LDS-DMA; fp32, pre-split f16x3 and grouped (G32) forms.
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// conv_glds_kernel: same tiling and epilogue, operand staging by LDS-DMA (buffer_load_dwordx4 ... lds), for Cin % 32 == 0
// (every layer but the stem).  What the experiments on this kernel family showed (tools/bench_conv_ablate.py and the
// timing variants recorded in DESIGN.md §4, 3x3 256->256 @256^2): MFMA-only floor 151.7 TF; LDS fragment reads and the
// per-step barrier are free (148-150 TF); register-staged operands with predicated global loads 120 TF; LDS-DMA with
// per-lane 64-bit pointers + zero-page selects 134 TF, of which ~3 % is the DMA instructions and ~9 % their address VALU
// (each VALU instruction takes an issue slot the MFMA stream wants).  Hence: buffer addressing.  A row's byte offset
// (voffset, 32-bit) is recomputed only when the tap (ky,kx) changes; the channel offset inside the tap and the K offset
// of the weights are block-uniform and ride in the scalar soffset; out-of-image taps and rows beyond M / Cout get an
// out-of-range voffset, for which the hardware bounds check writes zeros into LDS (probed on gfx950) -- no predication,
// no zero page, no per-step VALU.  One wave-instruction writes 8 rows x 128 B linearly, so the bank-conflict fix is an
// XOR swizzle applied to the per-lane SOURCE chunk and again on the fragment reads (chunk ^ ((row >> 1) & 7):
// conflict-free for the 16-lane groups of ds_read_b128).
// ------------------------------------------------------------------------------------------------------------------
// STEM = true: the 7x7 stride-2 stem on the [B,H,W,4] input with weights [64][7][8][4]: a K-step is one kernel row ky, whose
// 8 taps x 4 channels are 128 contiguous bytes; the 16-B chunk index IS the tap kx, so validity is per chunk.
// EPI: 0 = generic epilogue (any Cout), 1 = fast (Cout % 4 == 0, out_mode 0, res_mode 0/1), 2 = fast with per-row (b,oy,ox).
// F16 = true: AMP_CONV_F16X3 with BOTH operands already in the split hi|lo' row format -- the input tensor was written that way by
// its producer (conv epilogue / RoIAlign with split output; byte offsets equal the fp32 tensor's) -- so activations and weights
// are staged by LDS-DMA with no per-step VALU, and the compute loop is conv_f16x3_kernel's.  BN = 256 runs 8 waves (2 x 4).
// G32 = true (grouped conv with <= 32 channels per group, BN = 64, F16): a tap is ONE K-step.  The 64-channel window of the N tile is
// staged as two planes of 32 channels; wave column wn multiplies plane wn only -- in the block-diagonal window layout the weights of
// outputs [32 wn, 32 wn + 32) are zero outside that plane, so the two-steps-per-tap form spends half its MFMAs on zeros.  The weight
// rows are read from the same split copy (group (n >> 5) & 1 of each tap's 64 channels).  Same sums in the same order, bit for bit.
template <int BN, bool STEM = false, int EPI = 0, bool F16 = false, bool G32 = false>
__global__ __launch_bounds__(BN == 256 ? 512 : 256, BN == 256 ? 1 : 2) void conv_glds_kernel(const ConvArgs a, const unsigned int x_bytes,
                                                                                               const unsigned int w_bytes) {
    static_assert(!G32 || (BN == 64 && F16 && !STEM), "G32 is the grouped form of the 64-wide f16x3 tile");
    constexpr int BM = 128;
    constexpr int WTM = BM / 2, WTN = (BN == 64) ? 32 : 64;
    constexpr int NWN = BN / WTN, NW = 2 * NWN;   // waves across N, waves per workgroup
    constexpr int MT = WTM / 32, NT = WTN / 32;
    constexpr int NPL = G32 ? 2 : 1;      // A planes per tile
    constexpr int GA = BM / NW / 8;       // DMA instructions per wave, step and plane for A: BM/NW rows per wave, 8 rows each
    constexpr int GB = BN / NW / 8;       // ... for B: BN/NW rows per wave
    constexpr int TILE_FLOATS = (NPL * BM + BN) * BK;
    constexpr int SLD = WTN + 4;
    constexpr int STAGE_FLOATS = NW * WTM * SLD;
    // RING (the 64-wide f16x3 tiles: res2's and res5's 3x3 layers, the grouped layers of ResNeXt): three LDS buffers, the DMA of tile s+2
    // issued when tile s starts computing, counted vmcnt and a bare barrier -- conv_split_kernel's ring without the ping-pong.  A K-step of
    // this tile is 384 cycles of MFMA per wave and an LDS-DMA request needs ~2300 from issue to landing: with one tile in flight per
    // workgroup (two workgroups per CU) the matrix pipe waited two thirds of the time (PMC MFMA busy 0.26); 3 x 24.5 KB still fits twice.
    constexpr bool RING = F16 && BN == 64 && !STEM && !G32;      // (G32: two A planes, 3 x 41 KB would leave one workgroup per CU)
    constexpr int NBUF = RING ? 3 : 2;
    constexpr int LDS_FLOATS = (NBUF * TILE_FLOATS > STAGE_FLOATS) ? NBUF * TILE_FLOATS : STAGE_FLOATS;
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int l31 = lane & 31, lh = lane >> 5;

    const int tile = amp::xcd_remap(blockIdx.x, a.nblk);
    const int tile_n = tile % a.ntn;
    const int tile_m = tile / a.ntn;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;
    const int HoWo = a.Ho * a.Wo;

    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);

    // ---- staging geometry: instruction g of this wave fills rows wave*R + 8g + (lane>>3), 16-B position lane&7 ----
    const int srow = dma_row(lane), spos = dma_pos(lane);
    int a_iy0[GA], a_ix0[GA], a_pb[GA], a_chunk[GA];
#pragma unroll
    for (int g = 0; g < GA; ++g) {
        const int r = wave * (BM / NW) + 8 * g + srow;
        a_chunk[g] = dma_chunk(spos, r);      // source chunk (floats) = 4 * (pos ^ swz(row))
        const int m = m0 + r;
        if (m < a.M) {
            const int b = m / HoWo;
            const int rem = m - b * HoWo;
            const int oy = rem / a.Wo;
            const int ox = rem - oy * a.Wo;
            a_iy0[g] = oy * a.stride - a.pad;
            a_ix0[g] = ox * a.stride - a.pad;
            a_pb[g] = b * a.H * a.W;
        } else {
            a_iy0[g] = -(1 << 28);
            a_ix0[g] = 0;
            a_pb[g] = 0;
        }
    }
    unsigned int b_voff[GB];              // byte offset of the weight row (+ swizzled chunk); the K offset rides in soffset
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int r = wave * (BN / NW) + 8 * g + srow;
        const int n = n0 + r;
        b_voff[g] = (n < a.Cout) ? (unsigned int)(((size_t)n * a.K + (G32 ? 32 * ((n >> 5) & 1) : 0) + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }
    unsigned int a_voff[GA];              // byte offset of the input pixel of the current tap (+ swizzled chunk), or OOB

    const int csteps = (STEM || G32) ? 1 : a.cin_win / BK;   // K-steps per tap
    const int nsteps = G32 ? a.nsteps / 2 : a.nsteps;        // (G32: both 32-channel halves of a tap's window in one step)
    const int a_win = a.grouped ? n0 * 4 : 0;   // bytes: first input channel of this N-tile's window (grouped conv)
    const int kw_taps = STEM ? 1 : a.KW;        // STEM: the 8 taps of a row travel inside one K-step
    int ky = 0, kx = 0, cs = 0;           // block-uniform tap state of the tile being STAGED
    int kstep = 0;                        // index of the tile being staged

    auto stage = [&](int buf) {
        if (cs == 0) {                    // new tap: recompute the row offsets (uniform branch, once per Cin/32 steps)
#pragma unroll
            for (int g = 0; g < GA; ++g) {
                const int iy = a_iy0[g] + ky;
                const int ix = a_ix0[g] + (STEM ? (a_chunk[g] >> 2) : kx);
                const bool v = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const int off = STEM ? (a_pb[g] + iy * a.W + ix) * 4 : (a_pb[g] + iy * a.W + ix) * a.Cin + a_chunk[g];
                a_voff[g] = v ? (unsigned int)(off * 4) : OOB_VOFF;
            }
        }
        float* As = lds + buf * TILE_FLOATS;
        float* Bs = As + NPL * BM * BK;
        const int a_soff = cs * (BK * 4) + a_win;   // bytes, block-uniform
        const int b_soff = kstep * (NPL * BK * 4);  // (G32: a tap's weights are two groups of 32 channels, this row's one picked in b_voff)
#pragma unroll
        for (int h = 0; h < NPL; ++h)       // (G32: plane h = channels [32 h, 32 h + 32) of the window: the same rows, 128 B further)
#pragma unroll
            for (int g = 0; g < GA; ++g)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(As + h * BM * BK + (wave * (BM / NW) + 8 * g) * BK),
                                                         16, (int)a_voff[g], a_soff + h * (BK * 4), 0, 0);
#pragma unroll
        for (int g = 0; g < GB; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bs + (wave * (BN / NW) + 8 * g) * BK),
                                                     16, (int)b_voff[g], b_soff, 0, 0);
        ++kstep;
        if (++cs == csteps) {
            cs = 0;
            if (++kx == kw_taps) { kx = 0; ++ky; }
        }
    };

    f32x16 acc[MT][NT];                          // fp32 MFMA (F16 = false)
    constexpr int MB = WTM / 16, NB = WTN / 16;  // F16: blocks of 16 x 16 (f16x3_step16)
    f32x4 acc16[MB][NB], acx16[MB][NB];          // hi*hi sums; cross-term sums (scaled by 2^11)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc16[i][j][e] = 0.f; acx16[i][j][e] = 0.f; }
    const int l15 = lane & 15, lq = lane >> 4;
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));

    // fragment read offsets (floats): row*32 + 4*((2q+lh) ^ swz(row)), swz(row) = (l31>>1)&7 for every 32-row fragment
    const int fswz = (l31 >> 1) & 7;
    int foff[BK / 8];
#pragma unroll
    for (int q = 0; q < BK / 8; ++q) foff[q] = 4 * ((2 * q + lh) ^ fswz);

    if constexpr (RING) {
        constexpr int NDMA = NPL * GA + GB;     // LDS-DMA requests of this wave per tile
        stage(0);
        if (nsteps > 1) stage(1);
        int cur = 0, nxt = 2;
        for (int step = 0; step < nsteps; ++step) {
            ring_open<NDMA>(step + 1 < nsteps);
            if (step + 2 < nsteps) stage(nxt);  // into the buffer tile step-1 occupied
            f16x3_step16<MB, NB>(lds + cur * TILE_FLOATS + (G32 ? wn * BM * BK : 0) + (wm * WTM + l15) * BK,
                                 lds + cur * TILE_FLOATS + NPL * BM * BK + (wn * WTN + l15) * BK, fo16_hi, fo16_lo, acc16, acx16);
            ring_next<3>(cur, nxt);
        }
        __syncthreads();                        // all operand reads done: the epilogue re-uses the buffers as its staging tile
    } else {
    stage(0);
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): the LDS-DMA has landed (explicit: do not rely on the fence lowering)
    __syncthreads();

    for (int step = 0; step < nsteps; ++step) {
        const int cur = step & 1;
        if (step + 1 < nsteps) stage(cur ^ 1);

        const float* As = lds + cur * TILE_FLOATS + (wm * WTM + l31) * BK;
        const float* Bs = lds + cur * TILE_FLOATS + NPL * BM * BK + (wn * WTN + l31) * BK;
        if (F16) {
            f16x3_step16<MB, NB>(lds + cur * TILE_FLOATS + (G32 ? wn * BM * BK : 0) + (wm * WTM + l15) * BK,
                                 lds + cur * TILE_FLOATS + NPL * BM * BK + (wn * WTN + l15) * BK, fo16_hi, fo16_lo, acc16, acx16);
        } else {
#pragma unroll
            for (int q = 0; q < BK / 8; ++q) {
                f32x4 af[MT], bf[NT];
#pragma unroll
                for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const f32x4*>(As + i * 32 * BK + foff[q]);
#pragma unroll
                for (int j = 0; j < NT; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * BK + foff[q]);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][t], bf[j][t], acc[i][j], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the LDS-DMA of the next tile has landed
        __syncthreads();   // everyone is done with `cur`
    }
    }

    if (F16) {
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc16[i][j][e] = fold(acc16[i][j][e], acx16[i][j][e]);
        if (EPI == 0) conv_epilogue16<WTM, WTN, MB, NB, true>(a, acc16, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN, HoWo);
        else conv_epilogue_fast16<WTM, WTN, MB, NB, EPI == 2, true>(a, acc16, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN);
    } else {
        if (EPI == 0) conv_epilogue<WTM, WTN, MT, NT, false>(a, acc, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN, HoWo);
        else conv_epilogue_fast<WTM, WTN, MT, NT, EPI == 2, false>(a, acc, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN);
    }
}

}  // namespace
