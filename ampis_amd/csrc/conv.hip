// Convolution as implicit GEMM on the gfx950 matrix pipe: every kernel family, the launch table (conv_run) and the C entry points, one translation
// unit.  The pieces the families share are headers: conv_args.h (types, ConvArgs), conv_epilogue.h (the epilogues, the f16x3 MFMA step); so are the
// pure kernel selection, conv_plan.h, and the first family cut out, conv_nloop.h.  The other families and the weight-layout kernels stand below in
// the order the listing has them (which orders are part of the machine code); the tiling paragraph that follows describes the fp32
// kernel, conv_mfma_kernel.
//
// Replaces the cuDNN convolutions detectron2 runs for AMPIS:
// ResNet-50 stem+res2..res5, FPN lateral/output convs, the RPN head, the box-head FCs (as 1x1 convs over
// "pixels" = RoIs) and the mask head (3x3 convs, ConvTranspose 2x2 s2, 1x1 predictor).
//
// GEMM view: M = B*Ho*Wo output pixels, N = Cout, K = KH*KW*Cin, activations NHWC so a K-slice of 32 input
// channels of one tap is 128 contiguous bytes.  Block tile BM x BN x 32, 4 waves (2x2), each wave a
// (BM/2)x(BN/2) tile of 32x32 MFMA accumulators.  Both operand tiles sit in LDS as [row][k] with k contiguous
// and rows padded to 36 floats, so a lane fetches 4 consecutive k with one conflict-free ds_read_b128 and
// feeds 4 MFMAs from it (the k order inside a tile is permuted identically for A and B, which a sum over k
// does not see).  Register-staged double buffering: the global loads of K-step s+1 are issued before the MFMAs
// of step s and written to the other LDS buffer after them; one barrier per step.
//
// Epilogue (fused): y = acc*scale[n] + shift[n] (FrozenBN affine or conv bias), optional residual (same shape,
// or nearest-x2-upsampled for the FPN top-down path), optional ReLU, optional ConvTranspose2x2 scatter.
#include "common.h"
#include <type_traits>
#include "lds_ring.h"
#include "conv_args.h"          // types, BK, ConvArgs, fastdiv, conv_pixel
#include "conv_epilogue.h"      // the epilogues and the f16x3 MFMA step
#include "conv_nloop.h"         // conv1x1_nloop_kernel (experiment, default off)
#include "conv_plan.h"          // ConvSwitches, conv_plan (host only)

namespace {

// ABL (ablation, tools/bench_conv_ablate.py only; results wrong for ABL != 0): 1 = no global loads in the K loop,
// 2 = also no LDS writes / barriers, 3 = MFMA only (fragments read once).
template <int BM, int BN, int ABL = 0>
__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(const ConvArgs a) {
    constexpr int WTM = BM / 2, WTN = BN / 2;  // wave tile
    constexpr int MT = WTM / 32, NT = WTN / 32;
    constexpr int RA = BM / 32, RB = BN / 32;  // float4 loads per thread per step
    constexpr int TILE_FLOATS = (BM + BN) * LDS_LD;

    __shared__ __attribute__((aligned(16))) float lds[2 * TILE_FLOATS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const int tile = amp::xcd_remap(blockIdx.x, a.nblk);
    const int tile_n = tile % a.ntn;
    const int tile_m = tile / a.ntn;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;

    // ---- per-thread staging geometry: thread loads float4 #col4 of rows lrow + 32*r ----
    const int col4 = tid & 7;
    const int lrow = tid >> 3;

    int a_iy0[RA], a_ix0[RA], a_pb[RA];
    const int HoWo = a.Ho * a.Wo;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const int m = m0 + lrow + 32 * r;
        if (m < a.M) {
            const int b = m / HoWo;
            const int rem = m - b * HoWo;
            const int oy = rem / a.Wo;
            const int ox = rem - oy * a.Wo;
            a_iy0[r] = oy * a.stride - a.pad;
            a_ix0[r] = ox * a.stride - a.pad;
            a_pb[r] = b * a.H * a.W;
        } else {
            a_iy0[r] = -(1 << 28);
            a_ix0[r] = 0;
            a_pb[r] = 0;
        }
    }

    f32x4 ra[RA], rb[RB];

    auto load_tiles = [&](int step) {
        const int kidx = step * BK + col4 * 4;
        const int t = kidx / a.Cin;
        const int c = kidx - t * a.Cin;
        const int ky = t / a.KW;
        const int kx = t - ky * a.KW;
        const bool kv = kidx < a.K;
#pragma unroll
        for (int r = 0; r < RA; ++r) {
            const int iy = a_iy0[r] + ky;
            const int ix = a_ix0[r] + kx;
            const bool v = kv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (v) {
                const size_t off = (size_t)(a_pb[r] + iy * a.W + ix) * a.Cin + c;
                val = *reinterpret_cast<const f32x4*>(a.x + off);
            }
            ra[r] = val;
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int n = n0 + lrow + 32 * r;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (kv && n < a.Cout) {
                val = *reinterpret_cast<const f32x4*>(a.w + (size_t)n * a.K + kidx);
            }
            rb[r] = val;
        }
    };

    auto store_tiles = [&](int buf) {
        float* As = lds + buf * TILE_FLOATS;
        float* Bs = As + BM * LDS_LD;
#pragma unroll
        for (int r = 0; r < RA; ++r)
            *reinterpret_cast<f32x4*>(As + (lrow + 32 * r) * LDS_LD + col4 * 4) = ra[r];
#pragma unroll
        for (int r = 0; r < RB; ++r)
            *reinterpret_cast<f32x4*>(Bs + (lrow + 32 * r) * LDS_LD + col4 * 4) = rb[r];
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    load_tiles(0);
    store_tiles(0);
    __syncthreads();

    for (int step = 0; step < a.nsteps; ++step) {
        const int cur = step & 1;
        const bool more = step + 1 < a.nsteps;
        if (more && ABL == 0) load_tiles(step + 1);

        const float* As = lds + cur * TILE_FLOATS + (wm * WTM + l31) * LDS_LD + 4 * lh;
        const float* Bs = lds + cur * TILE_FLOATS + BM * LDS_LD + (wn * WTN + l31) * LDS_LD + 4 * lh;
#pragma unroll
        for (int q = 0; q < BK / 8; ++q) {
            f32x4 af[MT], bf[NT];
            if (ABL < 3 || step == 0) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    af[i] = *reinterpret_cast<const f32x4*>(As + i * 32 * LDS_LD + 8 * q);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    bf[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LDS_LD + 8 * q);
            } else {
#pragma unroll
                for (int i = 0; i < MT; ++i) af[i] = f32x4{acc[i][0][0], 1.f, 2.f, 3.f};
#pragma unroll
                for (int j = 0; j < NT; ++j) bf[j] = f32x4{acc[0][j][1], 1.f, 2.f, 3.f};
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][t], bf[j][t], acc[i][j], 0, 0, 0);
        }

        if (ABL < 2) {
            if (more) store_tiles(cur ^ 1);
            __syncthreads();
        }
    }
    if (ABL >= 2) __syncthreads();

    static_assert(4 * (BM / 2) * (BN / 2 + 4) <= 2 * TILE_FLOATS, "staging tile must fit in the operand buffers");
    conv_epilogue<WTM, WTN, MT, NT>(a, acc, lds, wave, lane, m0 + wm * WTM, n0 + wn * WTN, HoWo);
}

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


// ------------------------------------------------------------------------------------------------------------------
// mask_tail_kernel (round 4): the mask head's tail -- ConvTranspose 2x2 s2 as a GEMM to (tap, co) = 4 x 256 columns, ReLU, the predictor row of the
// detection's class, sigmoid -- with the FOUR taps of a 128-pixel block in ONE workgroup.  conv_split_kernel<128, 256, 3> ran one (pixel block, tap) tile
// per workgroup: K = 256 is eight K-steps, so every workgroup paid a cold ring (3300 cycles per step against 1950 in steady state: each step waits for
// its DMA), a prologue and an epilogue as long as the ideal loop for 5 us of MFMA work -- 17 us per tile (tools/stamp_conv.py deconv.gemm).  Here the ring
// runs through all 32 K-steps: tap t + 1's first tiles are requested during tap t's last steps (the activation rows come out of the L2 the second time),
// and a tap's epilogue needs no LDS staging: with the role-swapped MFMA a lane holds 16 channels of ONE pixel per row block -- the four 4-column groups
// 8 (j >> 1) + 2 lq + (j & 1) of conv_epilogue_predict's lanes -- so its sums are that epilogue's sums in that epilogue's order (4 columns in turn, then the
// xor tree 8, 4, 2, 1 over the groups: in-lane, lanes ^ 32, lanes ^ 16, in-lane; then the four N-waves in wave order through 2 KB of LDS behind the ring):
// BIT-IDENTICAL probabilities.  The two halves of the workgroup (tile rows 0-63 / 64-127) exchange only within themselves, at the loop's own barriers.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void mask_tail_kernel(const ConvArgs a, const unsigned int x_bytes, const unsigned int w_bytes) {
    constexpr int BM = 128, BN = 256, NW = 8, GA = 2, GB = 4, NDMA = GA + GB, NTAP = 4;
    constexpr int TILE_FLOATS = (BM + BN) * BK;
    // behind the ring: the N-waves' partial sums, the predictor rows of the (at most two) RoIs of the 128 pixels, their biases, the deconv's bias
    __shared__ __attribute__((aligned(16))) float lds[3 * TILE_FLOATS + 4 * BM + 2 * 256 + 4 + NTAP * BN];
    float* red = lds + 3 * TILE_FLOATS;                                   // [N-wave][128 rows]
    float* wps = red + 4 * BM;                                            // [RoI slot][256 columns]
    float* pbs = wps + 2 * 256;                                           // [RoI slot]
    float* dbias = pbs + 4;                                               // [tap][256 columns]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int l15 = lane & 15, lq = lane >> 4;
    const int m0 = amp::xcd_remap(blockIdx.x, a.nblk) * BM;
    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);
    const int srow = dma_row(lane), spos = dma_pos(lane);
    unsigned int a_voff[GA], b_voff[GB];
#pragma unroll
    for (int g = 0; g < GA; ++g) {
        const int r = wave * (BM / NW) + 8 * g + srow;
        const int m = m0 + r;
        a_voff[g] = (m < a.M) ? (unsigned int)(((size_t)m * a.Cin + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int r = wave * (BN / NW) + 8 * g + srow;
        const int n = (r & ~63) + swap_channel(r & 63);
        b_voff[g] = (unsigned int)(((size_t)n * a.K + dma_chunk(spos, r)) * 4);
    }
    const int csteps = a.Cin / BK;                 // K-steps per tap (8)
    const int total = NTAP * csteps;
    const int tap_bytes = BN * a.K * 4;            // weight rows of one tap
    int s_cs = 0, s_tap = 0;                       // the step being STAGED
    auto stage = [&](int buf) {
        float* As = lds + buf * TILE_FLOATS;
        float* Bs = As + BM * BK;
        const int a_soff = s_cs * (BK * 4);
        const int b_soff = s_tap * tap_bytes + s_cs * (BK * 4);
#pragma unroll
        for (int g = 0; g < GA; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(As + (wave * (BM / NW) + 8 * g) * BK), 16, (int)a_voff[g], a_soff, 0, 0);
#pragma unroll
        for (int g = 0; g < GB; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bs + (wave * (BN / NW) + 8 * g) * BK), 16, (int)b_voff[g], b_soff, 0, 0);
        if (++s_cs == csteps) { s_cs = 0; ++s_tap; }
    };
    f32x4 acc[4][4], acx[4][4];
    zero_acc(acc, acx);
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));
    stage(0);
    stage(1);
    // the predictor rows of the block's RoIs (128 consecutive pixels of 196-pixel RoIs: at most two) and the deconv's bias go into LDS once, requested
    // behind the first two tiles' DMA (the class-id load the row addresses wait for must not delay the staging)
    const int mw0 = m0 + wm * 64;
    const unsigned int b_first = fastdiv(min((unsigned int)m0, (unsigned int)(a.M - 1)), a.div_howo_mul, a.div_howo_shr);
    {
        const unsigned int b_last = fastdiv(min((unsigned int)(m0 + BM - 1), (unsigned int)(a.M - 1)), a.div_howo_mul, a.div_howo_shr);
        const int slot = tid >> 8, col = tid & 255;
        int c = a.pred_cls[slot ? b_last : b_first];
        c = (c >= 0 && c < a.pred_K) ? c : 0;
        wps[tid] = a.pred_w[(size_t)c * 256 + col];
        if (col == 0) pbs[slot] = a.pred_b[c];
        dbias[tid] = a.shift ? a.shift[tid] : 0.f;
        dbias[512 + tid] = a.shift ? a.shift[512 + tid] : 0.f;
    }
    bool bad = false;
    // a tap's sums of this wave: per tile row, the 64 columns of the wave against the RoI's predictor row -> red[wn][row]
    auto partial_sums = [&](int tap) {
        f32x4 bias[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bias[j] = *reinterpret_cast<const f32x4*>(dbias + tap * BN + wn * 64 + 32 * (j >> 1) + 8 * lq + 4 * (j & 1));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned int m = min((unsigned int)(mw0 + i * 16 + l15), (unsigned int)(a.M - 1));
            const unsigned int b = fastdiv(m, a.div_howo_mul, a.div_howo_shr);
            const float* wrow = wps + ((b == b_first) ? 0 : 256) + wn * 64 + 8 * lq;
            float sj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 wp = *reinterpret_cast<const f32x4*>(wrow + 32 * (j >> 1) + 4 * (j & 1));
                float sg = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = fold(acc[i][j][e], acx[i][j][e]);
                    bad = bad || !(fabsf(v) <= 3.0e38f);
                    const float o = fmaxf(__fadd_rn(v, bias[j][e]), 0.f);
                    sg = __fadd_rn(sg, __fmul_rn(o, wp[e]));
                }
                sj[j] = sg;
            }
            float u0 = __fadd_rn(sj[0], sj[2]), u1 = __fadd_rn(sj[1], sj[3]);      // xor 8 of the group index: j ^ 2, in the lane
            u0 = __fadd_rn(u0, __shfl_xor(u0, 32)); u1 = __fadd_rn(u1, __shfl_xor(u1, 32));      // xor 4: lq ^ 2
            u0 = __fadd_rn(u0, __shfl_xor(u0, 16)); u1 = __fadd_rn(u1, __shfl_xor(u1, 16));      // xor 2: lq ^ 1
            const float sres = __fadd_rn(u0, u1);                                   // xor 1: j ^ 1, in the lane
            if (lq == 0) red[wn * BM + wm * 64 + i * 16 + l15] = sres;
        }
    };
    // ... and the end of a tap for the 64 rows of this half: one row per lane of its N-wave 0
    auto finish_rows = [&](int tap) {
        const int rl = wm * 64 + lane;
        const int m = m0 + rl;
        if (m < a.M) {
            unsigned int b, oy, ox;
            conv_pixel(a, (unsigned int)m, b, oy, ox);
            float x = __fadd_rn(__fadd_rn(__fadd_rn(red[rl], red[BM + rl]), red[2 * BM + rl]), red[3 * BM + rl]);
            x = __fadd_rn(x, pbs[(b == b_first) ? 0 : 1]);
            const float p = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x)));
            a.prob[((size_t)b * 2 * a.Ho + 2 * oy + (tap >> 1)) * (2 * a.Wo) + 2 * ox + (tap & 1)] = p;
        }
    };
    int cur = 0, nxt = 2, c_cs = 0, c_tap = 0;      // ring positions; the step being COMPUTED
    auto open_step = [&](int step) { ring_open<NDMA>(step + 1 < total); };
    auto advance = [&]() {
        ring_next<3>(cur, nxt);
        if (++c_cs == csteps) { c_cs = 0; ++c_tap; }
    };
    F16x3Frags<4, 4> fr;
    const float* As0 = lds + (wm * 64 + l15) * BK;
    const float* Bs0 = lds + BM * BK + (wn * 64 + l15) * BK;
    if (wave < NW / 2) {
        for (int step = 0; step < total; ++step) {
            open_step(step);
            if (c_cs == 0 && c_tap > 0 && wn == 0) finish_rows(c_tap - 1);       // the previous tap's sums of this half: written before this barrier
            f16x3_load16<4, 4>(As0 + cur * TILE_FLOATS, Bs0 + cur * TILE_FLOATS, fo16_hi, fo16_lo, fr);
            __builtin_amdgcn_sched_barrier(0);
            if (step + 2 < total) stage(nxt);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
            f16x3_mfma16<4, 4, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            if (c_cs == csteps - 1) { partial_sums(c_tap); zero_acc(acc, acx); }
            advance();
        }
    } else {
        for (int step = 0; step < total; ++step) {
            open_step(step);
            __builtin_amdgcn_s_setprio(1);
            if (step > 0) f16x3_mfma16<4, 4, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            const bool tap_done = c_cs == 0 && c_tap > 0;                         // the MFMAs above finished tap c_tap - 1
            if (tap_done) { partial_sums(c_tap - 1); zero_acc(acc, acx); __builtin_amdgcn_s_waitcnt(0xc07f); }
            __builtin_amdgcn_s_barrier();
            if (tap_done && wn == 0) finish_rows(c_tap - 1);
            f16x3_load16<4, 4>(As0 + cur * TILE_FLOATS, Bs0 + cur * TILE_FLOATS, fo16_hi, fo16_lo, fr);
            __builtin_amdgcn_sched_barrier(0);
            if (step + 2 < total) stage(nxt);
            __builtin_amdgcn_sched_barrier(0);
            advance();
        }
        f16x3_mfma16<4, 4, true>(fr, acc, acx);
        partial_sums(NTAP - 1);
    }
    __syncthreads();
    if (wn == 0) finish_rows(NTAP - 1);
    if (bad) atomicOr(a.range_flag, 1);
}

// ------------------------------------------------------------------------------------------------------------------
// conv3x3_patch_kernel (round 4): the 3x3 stride-1 pad-1 convolutions of the FPN / RPN / res4 / res5 (Cin % 32 == 0, Cout % 256 == 0) with both
// operands in the split row format -- conv_split_kernel<128, 256>'s loop (ring of three weight tiles filled by LDS-DMA two steps ahead, counted
// vmcnt, bare barriers, the two halves of the workgroup one half-step apart), but the 128 GEMM rows of a workgroup are an 8 x 16 PIXEL tile and
// the activation operand is not staged per K-step: the K order is channel-major (32-channel chunk c outside, tap inside) and the (8 + 2) x (16 + 2)
// pixel patch of chunk c (180 pixels x 128 B, out-of-image pixels zero-filled by the buffer load) is staged ONCE for its nine taps -- tap (ky, kx)
// of tile row y is the same fragment read at patch pixel (y + ky) * 18 + kx + column.  Per K-step a workgroup now moves 32 KB of weights plus a
// ninth of 23 KB instead of 48 KB through the L2 -> LDS path, and an input pixel crosses it 1.4 times per N tile instead of nine: the implicit-GEMM
// kernel's counter traffic was 2.6 x its algorithmic bytes on these layers (profiles/r04/traffic_per_launch_tap_major.txt), on a chip that holds
// 1.84 GHz under this loop (tools/stamp_conv.py) because of the energy it draws.  LDS: 3 x 32 KB weight tiles + 2 x 23 KB patch chunks = 142 KB.
// The patch of chunk c + 1 goes into the other patch buffer during the first three steps of chunk c (one 1-KB piece per wave and step, issued
// behind the step's weight requests; the counted vmcnt in front of a step allows for them).
// Same exact products as every AMP_CONV_F16X3 kernel, summed in conv_split_kernel<.., CHAN = true>'s order (bit-identical to it: AMP_KORDER=1).
// ------------------------------------------------------------------------------------------------------------------
template <int EPI>      // 1: split rows through conv_epilogue_direct_rows; 3 / 4 / 5: the fused RPN tail with 16 / 32 / 48 predictor rows (conv_epilogue_rpn_rows)
__global__ __launch_bounds__(512, 1) void conv3x3_patch_kernel(const ConvArgs a, const unsigned int x_bytes, const unsigned int w_bytes, const int tiles_x, const int tiles_y) {
    constexpr int TH = 8, TW = 16, PW = TW + 2, NPIX = (TH + 2) * PW;            // 180 patch pixels
    constexpr int NPIECE = 24;                                                      // DMA pieces of 8 rows x 128 B: 3 per wave (the last 12 rows are zero-filled padding: every wave issues the same number of requests)
    constexpr int BT = 256 * BK;                                                    // floats per weight tile (32 KB)
    constexpr int PT = NPIECE * 8 * BK;                                             // floats per patch chunk (23 KB)
    constexpr int GB = 4;                                                           // weight DMA instructions per wave and step
    static_assert(BK == 32, "128-B rows");
    __shared__ __attribute__((aligned(16))) float lds[3 * BT + 2 * PT];
    float* patch = lds + 3 * BT;
#ifdef AMP_STAMP
    const long long st_entry = clock64();
#endif
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int l15 = lane & 15, lq = lane >> 4;
    int t = amp::xcd_remap(blockIdx.x, a.nblk);
    const int tile_n = t % a.ntn; t /= a.ntn;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW, n0 = tile_n * 256;
    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);
    const int srow = dma_row(lane), spos = dma_pos(lane);      // weight DMA: lane = (row of 8, 16-B position)
    // ---- patch layout in LDS: CHUNK-MAJOR -- the 16-B piece p (0..7: hi 0-7, .., hi 24-31, lo' 0-7, ..) of patch pixel q at p * 3072 + q * 16 bytes
    // (192 pixel slots per plane).  The 16 consecutive pixels a lane group reads for one fragment are then 256 contiguous bytes -- every bank once,
    // whatever the alignment of the first pixel -- and a lane's address is (its own base) + (tap, tile row) * constant: the nine taps and four tile
    // rows are immediate offsets of ds_read_b128, where a row-major swizzled patch cost ~8 VALU instructions per fragment, issued in the half-step
    // in which the SIMD's other wave owns the vector issue with its MFMAs (stamps: 540 cycles of fragment reads per step against 251).
    // DMA piece (wave w, j): plane p = w, pixels 64 j .. 64 j + 63 -- a lane fetches 16 B of its own pixel's row (the 8 waves read the same 64 rows).
    unsigned int p_voff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int q = 64 * j + lane;
        const int py = q / PW, px = q - py * PW;
        const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
        const bool v = q < NPIX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        p_voff[j] = v ? (unsigned int)(((size_t)(b * a.H + iy) * a.W + ix) * a.Cin * 4 + (size_t)(wave * 16)) : OOB_VOFF;
    }
    auto stage_patch = [&](int j, int c) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(patch + (c & 1) * PT + wave * 768 + j * 256), 16, (int)p_voff[j], c * (BK * 4), 0, 0);
    };
    unsigned int b_voff[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int r = wave * 32 + 8 * g + srow;
        const int n = n0 + (r & ~63) + swap_channel(r & 63);
        b_voff[g] = (n < a.Cout) ? (unsigned int)(((size_t)n * a.K + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }
    const int csteps = a.Cin / BK;
    int s_c = 0, s_tap = 0;                  // the step being STAGED
    auto stage_w = [&](int buf) {
        const int soff = (s_tap * csteps + s_c) * (BK * 4);      // (reading the weights as [Cout][chunk][tap][32], consecutive lines step after step: no difference, measured)
#pragma unroll
        for (int g = 0; g < GB; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(lds + buf * BT + (wave * 32 + 8 * g) * BK), 16, (int)b_voff[g], soff, 0, 0);
        if (++s_tap == 9) { s_tap = 0; ++s_c; }
    };
    f32x4 acc[4][4], acx[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[i][j][e] = 0.f; acx[i][j][e] = 0.f; }
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));
    const int qb = (4 * wm) * PW + l15;      // patch row of (tile row 4 wm, column l15) at tap (0, 0)

#pragma unroll
    for (int j = 0; j < 3; ++j) stage_patch(j, 0);
    stage_w(0);
    stage_w(1);
    int cur = 0, nxt = 2;
    int c_c = 0, c_tap = 0, c_toff = 0;      // the step being COMPUTED: chunk, tap, patch-row offset of the tap (ky * 18 + kx)
#ifdef AMP_STAMP
    long long st_vm = 0;
#endif
    auto open_step = [&](int step) {
        // weight tile `step` (requested two steps ago) has landed once everything younger is all that is outstanding: the patch piece of step - 2
        // (issued behind that tile's requests), the 4 weight requests of step - 1 and its patch piece -- counted exactly, an LDS-DMA request needs
        // more than one step to land (the patch itself is requested six steps or more before its chunk begins)
        if (step + 1 < a.nsteps) {
            const int extra = (c_c + 1 < csteps) ? ((c_tap >= 1 && c_tap <= 3) ? 1 : 0) + ((c_tap >= 2 && c_tap <= 4) ? 1 : 0) : 0;
            if (extra == 0) __builtin_amdgcn_s_waitcnt(0x0070 | GB);
            else if (extra == 1) __builtin_amdgcn_s_waitcnt(0x0070 | (GB + 1));
            else __builtin_amdgcn_s_waitcnt(0x0070 | (GB + 2));
        } else {
            __builtin_amdgcn_s_waitcnt(0x0070);
        }
#ifdef AMP_STAMP
        st_vm = clock64();
#endif
        ring_barrier();
    };
    F16x3Frags<4, 4> fr;
    const float* Pl = patch + qb * 4 + lq * 768;
    auto load_frags = [&]() {
        const float* P = Pl + ((c_c & 1) * PT + c_toff * 4);
        const float* Bs = lds + cur * BT + (wn * 64 + l15) * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fr.ah[i] = *reinterpret_cast<const f16x8*>(P + i * (PW * 4));
            fr.al[i] = *reinterpret_cast<const f16x8*>(P + i * (PW * 4) + 4 * 768);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fr.bh[j] = *reinterpret_cast<const f16x8*>(Bs + j * 16 * BK + fo16_hi);
            fr.bl[j] = *reinterpret_cast<const f16x8*>(Bs + j * 16 * BK + fo16_lo);
        }
    };
    auto stage_next = [&](int step) {        // in compute step `step`: weight tile step + 2, then one piece of the next chunk's patch
        if (step + 2 < a.nsteps) stage_w(nxt);
        if (c_tap < 3 && c_c + 1 < csteps) stage_patch(c_tap, c_c + 1);
    };
    auto advance = [&]() {
        ring_next<3>(cur, nxt);
        ++c_tap; ++c_toff;
        if (c_tap == 3 || c_tap == 6) c_toff += PW - 3;
        if (c_tap == 9) { c_tap = 0; c_toff = 0; ++c_c; }
    };
#ifdef AMP_STAMP
    long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long st_rt0 = __builtin_amdgcn_s_memrealtime(), st_mt0 = __builtin_amdgcn_s_memtime();
    const long long st_begin = clock64();
#endif
    if (wave < 4) {
        for (int step = 0; step < a.nsteps; ++step) {
            STAMP_T(t0);
            open_step(step);
            STAMP_T(t1);
            // the DMA requests in front of the fragment reads (the other way round in conv_split_kernel): this half reaches the second barrier ~200
            // cycles before the multiplying half does, and every request issued earlier is a shorter vmcnt wait two steps on (-2 % on the layer)
            stage_next(step);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t2);
            load_frags();
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t3);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
            f16x3_mfma16<4, 4, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t4);
            STAMP_ADD(0, t0, t1); STAMP_ADD(1, t1, t2); STAMP_ADD(2, t2, t3); STAMP_ADD(3, t3, t4);
#ifdef AMP_STAMP
            st_acc[7] += st_vm - t0;
            if (c_tap >= 3 && c_tap <= 5) st_acc[6] += t1 - t0;
#endif
            advance();
        }
    } else {
        for (int step = 0; step < a.nsteps; ++step) {
            STAMP_T(t0);
            open_step(step);
            STAMP_T(t1);
            __builtin_amdgcn_s_setprio(1);
            if (step > 0) f16x3_mfma16<4, 4, true>(fr, acc, acx);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            STAMP_T(t2);
            stage_next(step);
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t3);
            load_frags();
            __builtin_amdgcn_sched_barrier(0);
            STAMP_T(t4);
            STAMP_ADD(0, t0, t1); STAMP_ADD(3, t1, t2); STAMP_ADD(1, t2, t3); STAMP_ADD(2, t3, t4);
#ifdef AMP_STAMP
            st_acc[7] += st_vm - t0;
            if (c_tap >= 3 && c_tap <= 5) st_acc[6] += t1 - t0;
#endif
            advance();
        }
        f16x3_mfma16<4, 4, true>(fr, acc, acx);
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
    __syncthreads();

    const bool scaled_in = a.out_scale != 1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[i][j][e] = fold(acc[i][j][e], acx[i][j][e]);
                if (scaled_in) acc[i][j][e] *= a.out_scale;
            }
    const int oyw = oy0 + 4 * wm;
    if constexpr (EPI >= 3) {
        const int Ho = a.Ho, Wo = a.Wo, M = a.M;
        conv_epilogue_rpn_rows<EPI - 2>(a, acc, lds, wave, lane, n0, [=](int i, int r) {
            const int oy = oyw + i, ox = ox0 + r;
            return (oy < Ho && ox < Wo) ? (b * Ho + oy) * Wo + ox : M;
        });
    } else {
        // two tile rows at a time: the rows of an 8 x 16 tile are not consecutive GEMM rows, and four rows' hoisted residual + mask loads with
        // their own addresses do not fit the 256 registers of a wave (312 B of scratch in the epilogue)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int mrows[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int oy = oyw + 2 * h + i, ox = ox0 + l15;
                mrows[i] = (oy < a.Ho && ox < a.Wo) ? (b * a.Ho + oy) * a.Wo + ox : a.M;
            }
            conv_epilogue_direct_rows<false, true, 2>(a, reinterpret_cast<f32x4 (&)[2][4]>(acc[2 * h]), lane, mrows, n0 + wn * 64);
        }
    }
#ifdef AMP_STAMP
    if (lane == 0)
        for (int q = 0; q < 8; ++q) atomicAdd(&g_stamp[wave * 8 + q], (unsigned long long)st_acc[q]);
#endif
}

// ------------------------------------------------------------------------------------------------------------------
// conv3x3_c64_kernel (round 4): the 3x3 stride-1 convolution over a 64-channel WINDOW -- res2's dense 64 -> 64 layers and the grouped conv2
// of a ResNeXt (every 64-wide N tile reads its own 64 input channels) -- with both operands in the split row format.
// The implicit-GEMM kernels stage, per tap and K-step, the tile's (shifted) input pixels again: 18 K-steps re-read a 256-pixel tile's
// 64 channels nine times over, 1.2 GB of L2 -> LDS traffic per res2 layer for 134 MB of input, and that DMA stream, not the matrix pipe
// (0.31 of its peak), is their bound.  Here a workgroup stages the (8 + 2) x (16 + 2) pixel PATCH under its 8 x 16 output pixels once (180 pixels
// x 256 B = 46 KB, out-of-image pixels zero-filled by the buffer load) and all nine taps read their MFMA operands out of it: a 16 x 16
// MFMA block is one tile row of 16 pixels, so tap (ky, kx) is the same fragment read at patch pixel (row + ky) * 18 + kx + column.  Only the
// weights travel per tap (64 rows x 256 B, two buffers).  4 waves x (2 tile rows x 64 channels), two workgroups per CU (78 KB of LDS each).
// LDS rows are 256 B = 16 chunks of 16 B ([hi 0-31 | lo' 0-31 | hi 32-63 | lo' 32-63]); chunk c of row r sits at position c ^ (r & 15), applied
// to the SOURCE chunk of the LDS-DMA, so the 16 consecutive pixels (or weight rows) a lane group reads hit 16 different positions: conflict-free.
// Same products as every other AMP_CONV_F16X3 kernel (f16x3_mfma16), summed tap by tap (ky, kx, then the two 32-channel halves: the K order of
// the implicit-GEMM kernels), epilogue = conv_epilogue_direct_rows (FrozenBN / bias, ReLU, split ReLU mask for data gradients, split rows out).
// ------------------------------------------------------------------------------------------------------------------
// DIAG (groups of at most 32 channels): the 64 x 64 weight window is two 32 x 32 diagonal blocks -- LDS row blocks 0, 1 (channels 0-31 under swap_channel)
// see only the first 32-channel half of the window, blocks 2, 3 only the second: the other half of the products is exactly zero and is not computed
// (half the MFMAs and weight fragment reads; adding exact zeros changes no sum, so the result is the full product's bit for bit).
// FUSE3 (dense 64 -> 64 only: res2's conv2): the block's conv3 (1x1, 64 -> C3, FrozenBN, + residual, ReLU) runs in the same workgroup.  With the role-swapped MFMA
// a lane holds, per tile row, channels [8 lq, 8 lq + 8) of each 32-channel half of conv2's output -- after FrozenBN, ReLU and the split exactly the B fragment
// (pixel l15, k group lq) of a v_mfma_f32_16x16x32_f16 over that half: conv3's activation operand never leaves the registers, the 64-channel tensor t2 is
// neither written nor read back (2 x 134 MB per res2 block at B = 8) and a launch disappears.  conv3's weights (C3 rows of 256 B) are staged once into the LDS the
// patch and the tap buffers no longer need; every 64-channel chunk of the output goes through conv_epilogue_direct_rows (split residual, ReLU, split rows).
// The halves are the ones the two-launch chain stores and reloads, the products and their order conv_split_kernel's: bit-identical to the chain.
struct Fuse3Args {
    const float* w3;        // [C3][64] split rows
    const float* scale3;
    const float* shift3;
    const float* res;       // [M][C3] split rows
    float* y;               // [M][C3] split rows
    int C3;
    unsigned int w3_bytes;
};
template <bool DIAG, bool FUSE3 = false>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_kernel(const ConvArgs a, const unsigned int x_bytes, const unsigned int w_bytes, const int tiles_x, const int tiles_y, const Fuse3Args f3) {
    constexpr int TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, NPIX = PH * PW;      // 180 patch pixels
    constexpr int ROWF = 64;                                                        // floats per LDS row (256 B)
    constexpr int NINST = NPIX / 4;                                                 // 45 DMA instructions of 4 pixels x 16 chunks
    static_assert(NPIX % 4 == 0, "patch pixels per DMA instruction");
    __shared__ __attribute__((aligned(16))) float lds[NPIX * ROWF + 2 * 64 * ROWF];
    float* patch = lds;
    float* wbuf = lds + NPIX * ROWF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    int t = amp::xcd_remap(blockIdx.x, a.nblk);
    const int tile_n = t % a.ntn; t /= a.ntn;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW, n0 = tile_n * 64;
    const int cwin = a.grouped ? n0 : 0;                                            // first input channel of the window
    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);
    const int sub = lane >> 4, chunk = lane & 15;                                   // DMA: lane = (row sub of 4, 16-B chunk)
    // ---- the patch, once ----
    for (int it = wave; it < NINST; it += 4) {
        const int q = it * 4 + sub;
        const int py = q / PW, px = q - py * PW;
        const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
        const bool v = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        const unsigned int voff = v ? (unsigned int)((((size_t)(b * a.H + iy) * a.W + ix) * a.Cin + cwin) * 4 + (size_t)((chunk ^ (q & 15)) * 16)) : OOB_VOFF;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(patch + it * 4 * ROWF), 16, (int)voff, 0, 0, 0);
    }
    // ---- weights of one tap: 64 rows (LDS row r = output channel n0 + swap_channel(r)) x 256 B ----
    auto stage_w = [&](int tap, int buf) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int r = (wave * 4 + g) * 4 + sub;
            const int n = n0 + swap_channel(r);
            const unsigned int voff = (n < a.Cout) ? (unsigned int)(((size_t)n * a.K + (size_t)tap * 64) * 4 + (size_t)((chunk ^ (r & 15)) * 16)) : OOB_VOFF;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(wbuf + buf * 64 * ROWF + (wave * 4 + g) * 4 * ROWF), 16, (int)voff, 0, 0, 0);
        }
    };
    stage_w(0, 0);
    f32x4 acc[2][4], acx[2][4];
    zero_acc(acc, acx);
    for (int tap = 0; tap < 9; ++tap) {
        __syncthreads();                        // (vmcnt(0) + barrier) the patch and this tap's weights have landed; everyone is done with the other weight buffer
        if (tap + 1 < 9) stage_w(tap + 1, (tap + 1) & 1);
        const int ky = tap / 3, kx = tap - 3 * ky;
        const float* wb = wbuf + (tap & 1) * 64 * ROWF;
#pragma unroll
        for (int g = 0; g < 2; ++g) {           // the two 32-channel halves of the window
            F16x3Frags<2, 4> f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q = (2 * wave + i + ky) * PW + kx + l15;
                const float* row = patch + q * ROWF;
                f.ah[i] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + lq) ^ (q & 15)));
                f.al[i] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + 4 + lq) ^ (q & 15)));
            }
            if constexpr (DIAG) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const float* row = wb + ((2 * g + jj) * 16 + l15) * ROWF;
                    f.bh[jj] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + lq) ^ l15));
                    f.bl[jj] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + 4 + lq) ^ l15));
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {     // f16x3_mfma16<.., SWAP>'s order per accumulator: lo'*hi, hi*lo', hi*hi
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) acx[i][2 * g + jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.bh[jj], f.al[i], acx[i][2 * g + jj], 0, 0, 0);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) acx[i][2 * g + jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.bl[jj], f.ah[i], acx[i][2 * g + jj], 0, 0, 0);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) acc[i][2 * g + jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.bh[jj], f.ah[i], acc[i][2 * g + jj], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* row = wb + (j * 16 + l15) * ROWF;
                    f.bh[j] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + lq) ^ l15));
                    f.bl[j] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + 4 + lq) ^ l15));
                }
                f16x3_mfma16<2, 4, true>(f, acc, acx);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = fold(acc[i][j][e], acx[i][j][e]);
    int mrows[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int oy = oy0 + 2 * wave + i, ox = ox0 + l15;
        mrows[i] = (oy < a.Ho && ox < a.Wo) ? (b * a.Ho + oy) * a.Wo + ox : a.M;
    }
    if constexpr (!FUSE3) {
        conv_epilogue_direct_rows<false, true, 2>(a, acc, lane, mrows, n0);
    } else {
        // ---- conv2's epilogue in registers: FrozenBN, ReLU, split -> the B fragments of conv3 (what conv_epilogue_direct would have stored) ----
        f16x8 t2h[2][2], t2l[2][2];
        f32x2 chk = {0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x2 sc[4], sh[4];
            const int n = 32 * g + 8 * lq;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                sc[p] = a.scale ? f32x2{a.scale[n + 2 * p], a.scale[n + 2 * p + 1]} : f32x2{1.f, 1.f};
                sh[p] = a.shift ? f32x2{a.shift[n + 2 * p], a.shift[n + 2 * p + 1]} : f32x2{0.f, 0.f};
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const f32x4& blk = acc[i][2 * g + (p >> 1)];
                    const f32x2 v = {blk[2 * (p & 1)], blk[2 * (p & 1) + 1]};
                    chk = __builtin_elementwise_fma(v, f32x2{0.f, 0.f}, chk);
                    f32x2 o = v * sc[p] + sh[p];
                    if (a.relu) { o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f); }
                    const f16x2 h = __builtin_convertvector(o, f16x2);
                    const f32x2 hf = {(float)h[0], (float)h[1]};
                    const f32x2 l = __builtin_elementwise_fma(hf, f32x2{-LO_SCALE, -LO_SCALE}, o * LO_SCALE);
                    const f16x2 lh = __builtin_convertvector(l, f16x2);
                    t2h[i][g][2 * p] = h[0]; t2h[i][g][2 * p + 1] = h[1];
                    t2l[i][g][2 * p] = lh[0]; t2l[i][g][2 * p + 1] = lh[1];
                }
            }
        }
        if (!(chk[0] == 0.f) || !(chk[1] == 0.f)) atomicOr(a.range_flag, 1);
        // ---- conv3's weights: C3 rows x 256 B into the LDS of the patch + tap buffers (everyone is past its last tap) ----
        __syncthreads();
        const __amdgpu_buffer_rsrc_t rsrc_w3 = buffer_rsrc(f3.w3, f3.w3_bytes);
        float* w3s = lds;
        const int ninst3 = f3.C3 / 4;                    // 4 rows per DMA instruction
        for (int it = wave; it < ninst3; it += 4) {
            const int r = it * 4 + sub;
            const int n = (r & ~63) + swap_channel(r & 63);
            const unsigned int voff = (unsigned int)((size_t)n * 256 + (size_t)((chunk ^ (r & 15)) * 16));
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w3, (__attribute__((address_space(3))) void*)(w3s + it * 4 * ROWF), 16, (int)voff, 0, 0, 0);
        }
        __syncthreads();
        ConvArgs a3 = a;
        a3.scale = f3.scale3; a3.shift = f3.shift3; a3.res = f3.res; a3.mask = nullptr; a3.y = f3.y;
        a3.Cout = f3.C3; a3.relu = 1; a3.res_mode = 1; a3.res_split = 1; a3.y_split = 1; a3.out_mode = 0; a3.mask_split = 0;
        for (int c = 0; c < f3.C3 / 64; ++c) {
            f32x4 acc3[2][4], acx3[2][4];
            zero_acc(acc3, acx3);
            const float* wc = w3s + c * 64 * ROWF;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                F16x3Frags<2, 4> f;
#pragma unroll
                for (int i = 0; i < 2; ++i) { f.ah[i] = t2h[i][g]; f.al[i] = t2l[i][g]; }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* row = wc + (j * 16 + l15) * ROWF;
                    f.bh[j] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + lq) ^ l15));
                    f.bl[j] = *reinterpret_cast<const f16x8*>(row + 4 * ((8 * g + 4 + lq) ^ l15));
                }
                f16x3_mfma16<2, 4, true>(f, acc3, acx3);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc3[i][j][e] = fold(acc3[i][j][e], acx3[i][j][e]);
            conv_epilogue_direct_rows<false, true, 2>(a3, acc3, lane, mrows, 64 * c);
        }
    }
}

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

// stem_pool_f16x3_kernel: the 7x7 stride-2 stem (conv_f16x3_kernel<64, ., STEM>) and the 3x3 stride-2 max-pool behind it in ONE kernel.
// Separately the stem writes its [B, H/2, W/2, 64] fp32 output (537 MB for a batch of 8 at 1024^2) and the pool reads it back: 1.07 GB
// through HBM and a launch for a tensor nobody else reads.  Here a workgroup owns a tile of SP_PH x SP_PW pooled pixels: its M tile is
// the (2 SP_PH + 1) x (2 SP_PW + 1) = 17 x 15 = 255 convolution outputs under that tile (256 rows of A, 8 waves as 4 x 2 wave tiles of
// 64 x 32), the accumulators take scale / shift / ReLU as in conv_epilogue_rows, land in LDS as the patch, and 448 threads take the
// maximum of the nine patch pixels of a pooled pixel, 8 channels each, and write it -- in the split hi | lo' row format when the trunk
// runs on it.  Every convolution output is the same sum in the same order as in the unfused kernel (7 K-steps of one kernel row each), so the
// pooled tensor is bit-identical; the halo costs 256 / 224 = 1.14 x the MFMA work of the stem.
constexpr int SP_PH = 8, SP_PW = 7, SP_CH = 2 * SP_PH + 1, SP_CW = 2 * SP_PW + 1;      // pooled tile, conv patch
struct StemPoolArgs {
    float* pool;            // [B][Hq][Wq][64] (fp32 rows or split rows)
    int Hq, Wq;             // pooled size
    int tiles_x, tiles_y;
    int pool_split;
};

template <bool X_SPLIT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void stem_pool_f16x3_kernel(const ConvArgs a, const StemPoolArgs sp, const unsigned int x_bytes,
                                                                 const unsigned int w_bytes) {
    constexpr int BM = 256, BN = 64;
    constexpr int WTM = 64, WTN = 32, NWN = 2;      // 8 waves: 4 x 2 wave tiles
    constexpr int RPT = 2;                // activation rows per lane: 256 rows x 4 lanes per row over 512 threads
    constexpr int TILE_FLOATS = (BM + BN) * BK;
    constexpr int SLD = BN + 4;           // patch row in LDS: 64 channels + pad
    static_assert(2 * TILE_FLOATS >= BM * SLD, "the patch reuses the operand buffers");
    static_assert(SP_CH * SP_CW <= BM, "the patch is the M tile");
    __shared__ __attribute__((aligned(16))) float lds[2 * TILE_FLOATS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;

    const int tx = blockIdx.x % sp.tiles_x;
    const int tyb = blockIdx.x / sp.tiles_x;
    const int ty = tyb % sp.tiles_y, b = tyb / sp.tiles_y;
    const int oy_first = 2 * ty * SP_PH - 1, ox_first = 2 * tx * SP_PW - 1;      // conv pixel of patch row 0 / column 0

    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);

    // ---- A: lane = 4 * (row in a 16-row group) + kg; a lane owns 8 consecutive k (two taps x 4 channels) of rows ra[0], ra[1] ----
    const int arow = lane >> 2, akg = lane & 3;
    int a_iy0[RPT], a_ix0[RPT], a_row[RPT];
    const int a_pb = b * a.H * a.W;
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        const int r = p * 128 + wave * 16 + arow;
        a_row[p] = r;
        const int pr = r / SP_CW, pc = r - pr * SP_CW;
        const int oy = oy_first + pr, ox = ox_first + pc;
        const bool v = pr < SP_CH && (unsigned)oy < (unsigned)a.Ho && (unsigned)ox < (unsigned)a.Wo;
        a_iy0[p] = v ? oy * a.stride - a.pad : -(1 << 28);
        a_ix0[p] = v ? ox * a.stride - a.pad : 0;
    }
    // ---- B (split weights): LDS-DMA, 8 rows x 128 B per wave-instruction, source chunk XOR-swizzled ----
    const int srow = dma_row(lane), spos = dma_pos(lane);
    unsigned int b_voff;
    {
        const int r = wave * 8 + srow;
        b_voff = (r < a.Cout) ? (unsigned int)(((size_t)r * a.K + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }
    int kstep = 0;
    u32x4 ra[RPT][2];
    auto fetch = [&](int buf) {                 // A(kstep) -> registers, B(kstep) -> LDS[buf]
#pragma unroll
        for (int p = 0; p < RPT; ++p) {
            const int iy = a_iy0[p] + kstep;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ix = a_ix0[p] + 2 * akg + h;
                const bool v = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const unsigned int vo = v ? (unsigned int)((a_pb + iy * a.W + ix) * 16) : OOB_VOFF;
                ra[p][h] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)vo, 0, 0);
            }
        }
        float* Bs = lds + buf * TILE_FLOATS + BM * BK;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bs + (wave * 8) * BK), 16, (int)b_voff,
                                                 kstep * (BK * 4), 0, 0);
        ++kstep;
    };
    auto commit = [&](int buf) {                // split the fetched A registers into LDS[buf]
        float* As = lds + buf * TILE_FLOATS;
#pragma unroll
        for (int p = 0; p < RPT; ++p) {
            const int r = a_row[p], sw = (r >> 1) & 7;
            if (X_SPLIT) {      // the pixels arrive split (preprocess_run): a lane's two taps are {hi4 | lo4} twice -- regroup, no arithmetic
                const u32x4 hi = {ra[p][0][0], ra[p][0][1], ra[p][1][0], ra[p][1][1]};
                const u32x4 lo = {ra[p][0][2], ra[p][0][3], ra[p][1][2], ra[p][1][3]};
                *reinterpret_cast<u32x4*>(As + r * BK + 4 * (akg ^ sw)) = hi;
                *reinterpret_cast<u32x4*>(As + r * BK + 4 * ((4 + akg) ^ sw)) = lo;
            } else {
                f16x8 hi, lo;
                split8<false>(__builtin_bit_cast(f32x4, ra[p][0]), __builtin_bit_cast(f32x4, ra[p][1]), hi, lo, 1.0f);
                *reinterpret_cast<f16x8*>(As + r * BK + 4 * (akg ^ sw)) = hi;
                *reinterpret_cast<f16x8*>(As + r * BK + 4 * ((4 + akg) ^ sw)) = lo;
            }
        }
    };

    constexpr int MB = WTM / 16, NB = WTN / 16;
    f32x4 acc[MB][NB], acx[MB][NB];
    zero_acc(acc, acx);

    const int l15 = lane & 15, lq = lane >> 4;
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));

    fetch(0);
    commit(0);
    __builtin_amdgcn_s_waitcnt(0x0F70);     // B(0) has landed
    __syncthreads();
    if (a.nsteps > 1) fetch(1);
    for (int step = 0; step < a.nsteps; ++step) {
        const int cur = step & 1;
        f16x3_step16<MB, NB>(lds + cur * TILE_FLOATS + (wm * WTM + l15) * BK, lds + cur * TILE_FLOATS + BM * BK + (wn * WTN + l15) * BK,
                             fo16_hi, fo16_lo, acc, acx);
        if (step + 1 < a.nsteps) commit(cur ^ 1);
        __builtin_amdgcn_s_waitcnt(0x0F70);     // the weight DMA into LDS[cur^1] has landed (see conv_f16x3_kernel)
        __syncthreads();
        if (step + 2 < a.nsteps) fetch(cur);
    }

    // ---- the patch: fold the cross terms, scale / shift / ReLU (conv_epilogue_rows' arithmetic), -1 for pixels outside the image ----
    float* patch = lds;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = wn * WTN + j * 16 + l15;
        const float sc = (a.scale && n < a.Cout) ? a.scale[n] : 1.f, sh = (a.shift && n < a.Cout) ? a.shift[n] : 0.f;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = wm * WTM + i * 16 + 4 * lq + e;
                const int pr = r / SP_CW, pc = r - pr * SP_CW;
                const bool v = pr < SP_CH && (unsigned)(oy_first + pr) < (unsigned)a.Ho && (unsigned)(ox_first + pc) < (unsigned)a.Wo;
                const float s = fold(acc[i][j][e], acx[i][j][e]);
                bad = bad || !(fabsf(s) <= 3.0e38f);
                float t = __fadd_rn(__fmul_rn(s, sc), sh);
                if (a.relu) t = fmaxf(t, 0.f);
                patch[r * SLD + n] = v ? t : -1.0f;
            }
    }
    if (bad) atomicOr(a.range_flag, 1);
    __syncthreads();

    // ---- pool: thread = (pooled pixel q, 8 channels) ----
    if (tid < SP_PH * SP_PW * 8) {
        const int q = tid >> 3, c8 = tid & 7;
        const int ppy = q / SP_PW, ppx = q - ppy * SP_PW;
        const int py = ty * SP_PH + ppy, px = tx * SP_PW + ppx;
        if (py < sp.Hq && px < sp.Wq) {
            float m[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) m[c] = -1.0f;         // (the centre of a window is always inside the image and ReLU output is >= 0)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float* src = patch + ((2 * ppy + dy) * SP_CW + 2 * ppx + dx) * SLD + 8 * c8;
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { m[c] = fmaxf(m[c], v0[c]); m[4 + c] = fmaxf(m[4 + c], v1[c]); }
                }
            float* orow = sp.pool + ((size_t)(b * sp.Hq + py) * sp.Wq + px) * 64;
            if (sp.pool_split) {
                f16x8 hi, lo;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const _Float16 h = (_Float16)m[c];
                    hi[c] = h;
                    lo[c] = (_Float16)((m[c] - (float)h) * LO_SCALE);
                }
                const int ch = 8 * c8;
                char* base = reinterpret_cast<char*>(orow) + (ch >> 5) * 128 + (ch & 31) * 2;
                *reinterpret_cast<f16x8*>(base) = hi;
                *reinterpret_cast<f16x8*>(base + 64) = lo;
            } else {
                reinterpret_cast<f32x4*>(orow)[2 * c8] = f32x4{m[0], m[1], m[2], m[3]};
                reinterpret_cast<f32x4*>(orow)[2 * c8 + 1] = f32x4{m[4], m[5], m[6], m[7]};
            }
        }
    }
}

// w [rows][K] fp32 -> split rows: per K-step of 32, 32 f16 hi halves (64 B) then 32 f16 lo' halves (64 B)
__global__ void split_weights_kernel(const float* __restrict__ w, size_t rows, int K, unsigned int* __restrict__ out) {
    const size_t total = rows * (size_t)(K / 2);     // one thread per pair of consecutive k
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (K / 2);
        const int kp = (int)(i - r * (K / 2));       // pair index in the row
        const int step = kp / 16, j = kp % 16;       // 16 pairs per K-step
        unsigned int hw = 0, lw = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float x = w[r * K + 2 * kp + q];
            const _Float16 h = (_Float16)x;
            const _Float16 l = (_Float16)((x - (float)h) * LO_SCALE);
            hw |= (unsigned int)__builtin_bit_cast(unsigned short, h) << (16 * q);
            lw |= (unsigned int)__builtin_bit_cast(unsigned short, l) << (16 * q);
        }
        unsigned int* o = out + r * K + step * 32;
        o[j] = hw;
        o[16 + j] = lw;
    }
}

// The split copies of MANY weight tensors in one launch (a training step re-makes them all after the SGD update: one launch instead of
// one per layer, twice).  A job is one tensor; a chunk is (job, first pair) and covers up to 8192 pairs of consecutive K elements.
//   transpose = 0: out = split rows of w [N][KH*KW*C] (what split_weights_kernel writes)
//   transpose = 1: out = split rows of the data-gradient form Wt[c][KH-1-ky][KW-1-kx][n] = w[n][ky][kx][c] * scale[n] (dgrad_weight_kernel
//                  followed by split_weights_kernel, same roundings), N % 32 == 0
//   transpose = 2: the same tensor as 1 for N % 64 == 0 and C % 64 == 0; a chunk is one 64 (n) x 64 (c) tile of one tap, transposed through
//                  LDS so that both the reads (along c) and the writes (along n) are whole cache lines (the pairwise form reads one float
//                  per 4 * KH * KW * C bytes: 0.75 ms for the R50-FPN heads + trunk against 0.1 ms of traffic)
__global__ __launch_bounds__(256) void weight_jobs_kernel(const amp::WeightJob* __restrict__ jobs, const uint2* __restrict__ chunks) {
    const uint2 ch = chunks[blockIdx.x];
    const amp::WeightJob L = jobs[ch.x];
    if (L.transpose == 2) {
        __shared__ float tile[64][65];
        const int ntc = L.C / 64, ntn = L.N / 64;
        int id = (int)ch.y;
        const int tc = id % ntc; id /= ntc;
        const int tn = id % ntn;
        const int tap = id / ntn;
        const int ky = tap / L.KW, kx = tap - ky * L.KW;
        const int n0 = tn * 64, c0 = tc * 64;
        const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            const int nn = it * 4 + lr;
            float v = L.w[(((size_t)(n0 + nn) * L.KH + ky) * L.KW + kx) * L.C + c0 + lc];
            if (L.scale) v = __fmul_rn(v, L.scale[n0 + nn]);
            tile[nn][lc] = v;
        }
        __syncthreads();
        const int kyp = L.KH - 1 - ky, kxp = L.KW - 1 - kx;
#pragma unroll 4
        for (int it = 0; it < 8; ++it) {
            const int p = it * 256 + (int)threadIdx.x;
            const int cc = p >> 5, nn = (p & 31) * 2;
            unsigned int hw = 0, lw = 0;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float x = tile[nn + q][cc];
                const _Float16 h = (_Float16)x;
                const _Float16 l = (_Float16)((x - (float)h) * LO_SCALE);
                hw |= (unsigned int)__builtin_bit_cast(unsigned short, h) << (16 * q);
                lw |= (unsigned int)__builtin_bit_cast(unsigned short, l) << (16 * q);
            }
            const size_t i = (((size_t)(c0 + cc) * L.KH + kyp) * L.KW + kxp) * L.N + n0 + nn;
            unsigned int* o = L.out + (i & ~(size_t)31);
            const int j = (int)(i & 31) >> 1;
            o[j] = hw;
            o[16 + j] = lw;
        }
        return;
    }
    const size_t npairs = (size_t)L.N * L.KH * L.KW * L.C / 2;
    for (int t = threadIdx.x; t < 8192; t += 256) {
        const size_t pi = (size_t)ch.y + t;
        if (pi >= npairs) break;
        const size_t i = 2 * pi;                       // index of the pair's first element in the output tensor
        float x[2];
        if (L.transpose) {
            const int n = (int)(i % L.N);
            size_t r = i / L.N;
            const int kxp = (int)(r % L.KW); r /= L.KW;
            const int kyp = (int)(r % L.KH);
            const int c = (int)(r / L.KH);
            const int ky = L.KH - 1 - kyp, kx = L.KW - 1 - kxp;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                x[q] = L.w[(((size_t)(n + q) * L.KH + ky) * L.KW + kx) * L.C + c];
                if (L.scale) x[q] = __fmul_rn(x[q], L.scale[n + q]);
            }
        } else {
            x[0] = L.w[i]; x[1] = L.w[i + 1];
        }
        unsigned int hw = 0, lw = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const _Float16 h = (_Float16)x[q];
            const _Float16 l = (_Float16)((x[q] - (float)h) * LO_SCALE);
            hw |= (unsigned int)__builtin_bit_cast(unsigned short, h) << (16 * q);
            lw |= (unsigned int)__builtin_bit_cast(unsigned short, l) << (16 * q);
        }
        unsigned int* o = L.out + (i & ~(size_t)31);   // rows are multiples of 32: a K-step's 32 values are 32 consecutive elements
        const int j = (int)(i & 31) >> 1;
        o[j] = hw;
        o[16 + j] = lw;
    }
}

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

namespace {
__global__ void unsplit_rows_kernel(const unsigned int* __restrict__ in, size_t rows, int C, float* __restrict__ out) {
    const size_t total = rows * (size_t)(C / 2);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (C / 2);
        const int kp = (int)(i - r * (C / 2));
        const int step = kp / 16, j = kp % 16;
        const unsigned int hw = in[r * C + step * 32 + j], lw = in[r * C + step * 32 + 16 + j];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const _Float16 h = __builtin_bit_cast(_Float16, (unsigned short)(hw >> (16 * q)));
            const _Float16 l = __builtin_bit_cast(_Float16, (unsigned short)(lw >> (16 * q)));
            out[r * C + 2 * kp + q] = fold((float)h, (float)l);
        }
    }
}
}  // namespace

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

namespace {
__global__ void group_expand_kernel(const float* __restrict__ w, int Cout, int taps, int cpg, float* __restrict__ out) {
    const size_t total = (size_t)Cout * taps * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 63);
        const size_t nt = i >> 6;
        const int t = (int)(nt % taps), n = (int)(nt / taps);
        const int c = (n & ~63) + j;                  // input channel of window slot j
        const int g = n / cpg;
        out[i] = (c / cpg == g) ? w[((size_t)n * taps + t) * cpg + (c - g * cpg)] : 0.f;
    }
}
}  // namespace

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

// stem_pool_u8_kernel: the fused stem + pool straight from the uint8 image.  stem_pool_f16x3_kernel fetches its A tile from the
// preprocessed [B,H,W,4] tensor once per kernel row: 2.1 GB of L2 -> LDS traffic per batch for 134 MB of pixels (every input pixel is
// the tap of ~12 convolution outputs of a tile, seven K-steps over), after a kernel that wrote those 134 MB.  Here a workgroup reads the
// 39 x 36 input pixels under its 17 x 15 convolution patch ONCE -- three bytes each, normalised and split exactly as preprocess_kernel<true>
// does -- into two LDS planes (hi halves, lo' halves: 8 B per pixel each), and the MFMA A fragments are read straight out of the planes:
// a lane's 8 consecutive k of kernel row ky are taps 2 lq, 2 lq + 1 x 4 channels = the 16 bytes at pixel (2 pr + ky, 2 pc + 2 lq) of a
// plane (stride-2 pixels: 16 lanes cover 256 contiguous bytes, conflict-free).  No A staging, no preprocess pass, only the 8-KB weight
// tile per K-step by LDS-DMA.  Same products, same 7 K-steps in the same order: the pooled tensor is bit-identical.
constexpr int SP_IH = 2 * (SP_CH - 1) + 7, SP_IW = 2 * (SP_CW - 1) + 8;      // 39 x 36 input pixels (the 8th tap of a row has zero weights)
struct StemU8Args {
    const uint8_t* img;       // [B][H][W][3] BGR
    int H, W;                 // image size (the padded size the conv sees is a.H x a.W; beyond the valid size everything is 0)
    const int* img_hw;        // optional device [B][2]: per-image valid size
    float m0, m1, m2, s0, s1, s2;
};
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void stem_pool_u8_kernel(const ConvArgs a, const StemPoolArgs sp, const StemU8Args u,
                                                                                                       const unsigned int w_bytes) {
    constexpr int BM = 256, BN = 64;
    constexpr int WTM = 64, WTN = 32, NWN = 2;      // 8 waves: 4 x 2 wave tiles
    constexpr int SLD = BN + 4;
    constexpr int PLANE_BYTES = SP_IH * SP_IW * 8;                 // 11 232
    constexpr int BT_FLOATS = BN * BK;                              // one weight tile: 64 rows x 128 B
    constexpr int NKS = 7;                                          // kernel rows = K-steps: ALL weight tiles are resident (57 KB), so the K loop
    constexpr int OPER_BYTES = 2 * PLANE_BYTES + NKS * BT_FLOATS * 4;   // has no barrier and no wait (a K-step is 0.2 us of MFMAs, a weight DMA 1.1 us)
    constexpr int LDS_BYTES = (OPER_BYTES > BM * SLD * 4) ? OPER_BYTES : BM * SLD * 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    unsigned char* plane_hi = lds_raw;
    unsigned char* plane_lo = lds_raw + PLANE_BYTES;
    float* Bt = reinterpret_cast<float*>(lds_raw + 2 * PLANE_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int tx = blockIdx.x % sp.tiles_x;
    const int tyb = blockIdx.x / sp.tiles_x;
    const int ty = tyb % sp.tiles_y, b = tyb / sp.tiles_y;
    const int oy_first = 2 * ty * SP_PH - 1, ox_first = 2 * tx * SP_PW - 1;      // conv pixel of patch row 0 / column 0
    const int iy_first = 2 * oy_first - 3, ix_first = 2 * ox_first - 3;           // input pixel of plane row 0 / column 0

    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, w_bytes);
    const int srow = dma_row(lane), spos = dma_pos(lane);
    unsigned int b_voff;
    {
        const int r = wave * 8 + srow;
        b_voff = (r < a.Cout) ? (unsigned int)(((size_t)r * a.K + dma_chunk(spos, r)) * 4) : OOB_VOFF;
    }
    // (no lambda here: AMP_NO_PK changes the kernel's target features, and a closure compiled with the default ones is then CALLED, not inlined)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(Bt + ks * BT_FLOATS + (wave * 8) * BK), 16, (int)b_voff,
                                                 ks * (BK * 4), 0, 0);

    // ---- the input patch: normalise (preprocess_kernel's operations) and split into the two planes ----
    {
        const int vh = u.img_hw ? u.img_hw[2 * b] : u.H, vw = u.img_hw ? u.img_hw[2 * b + 1] : u.W;
        const uint8_t* ib = u.img + (size_t)b * u.H * u.W * 3;
        constexpr int NPX = (SP_IH * SP_IW + 511) / 512;            // pixels per thread: all their byte loads are issued before the first use
        unsigned char pxb[NPX][3];
        bool pv[NPX];
#pragma unroll
        for (int t = 0; t < NPX; ++t) {
            const int q = tid + 512 * t;
            const int r = q / SP_IW, cidx = q - r * SP_IW;
            const int iy = iy_first + r, ix = ix_first + cidx;
            pv[t] = q < SP_IH * SP_IW && (unsigned)iy < (unsigned)vh && (unsigned)ix < (unsigned)vw;
            const uint8_t* px = ib + ((size_t)(pv[t] ? iy : 0) * u.W + (pv[t] ? ix : 0)) * 3;
            pxb[t][0] = px[0]; pxb[t][1] = px[1]; pxb[t][2] = px[2];
        }
#pragma unroll
        for (int t = 0; t < NPX; ++t) {
            const int q = tid + 512 * t;
            f16x4 hi = {0, 0, 0, 0}, lo = {0, 0, 0, 0};
            if (pv[t]) {
                float v[3];
                v[0] = __fdiv_rn(__fsub_rn((float)pxb[t][0], u.m0), u.s0);
                v[1] = __fdiv_rn(__fsub_rn((float)pxb[t][1], u.m1), u.s1);
                v[2] = __fdiv_rn(__fsub_rn((float)pxb[t][2], u.m2), u.s2);
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const _Float16 h = (_Float16)v[e];
                    hi[e] = h;
                    lo[e] = (_Float16)((v[e] - (float)h) * LO_SCALE);
                }
            }
            if (q < SP_IH * SP_IW) {
                *reinterpret_cast<f16x4*>(plane_hi + q * 8) = hi;
                *reinterpret_cast<f16x4*>(plane_lo + q * 8) = lo;
            }
        }
    }

    constexpr int MB = WTM / 16, NB = WTN / 16;
    f32x4 acc[MB][NB], acx[MB][NB];
    zero_acc(acc, acx);
    const int l15 = lane & 15, lq = lane >> 4;
    const int fo16_hi = 4 * (lq ^ (l15 >> 1)), fo16_lo = 4 * ((4 + lq) ^ (l15 >> 1));
    int a_off[MB];                                   // byte offset of this lane's A fragment inside a plane, kernel row 0
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        const int r = wm * WTM + i * 16 + l15;
        const int pr = min(r / SP_CW, SP_CH - 1), pc = r - (r / SP_CW) * SP_CW;      // (row 255 is no patch pixel: it reads patch row 16, its result is dropped)
        a_off[i] = ((2 * pr) * SP_IW + 2 * pc + 2 * lq) * 8;
    }

    __builtin_amdgcn_s_waitcnt(0x0F70);     // the weight tiles have landed
    AMP_SYNCTHREADS();                        // planes and weights complete
#pragma unroll
    for (int step = 0; step < NKS; ++step) {
        const int cur = step;
        F16x3Frags<MB, NB> f;
        const int krow = step * (SP_IW * 8);
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            f.ah[i] = *reinterpret_cast<const f16x8*>(plane_hi + a_off[i] + krow);
            f.al[i] = *reinterpret_cast<const f16x8*>(plane_lo + a_off[i] + krow);
        }
        const float* Bs = Bt + cur * BT_FLOATS + (wn * WTN + l15) * BK;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            f.bh[j] = *reinterpret_cast<const f16x8*>(Bs + j * 16 * BK + fo16_hi);
            f.bl[j] = *reinterpret_cast<const f16x8*>(Bs + j * 16 * BK + fo16_lo);
        }
        f16x3_mfma16<MB, NB>(f, acc, acx);
    }
    AMP_SYNCTHREADS();                        // every wave is done with the planes and the weights: the patch takes their place

    // ---- the patch: fold the cross terms, scale / shift / ReLU (conv_epilogue_rows' arithmetic), -1 for pixels outside the image ----
    float* patch = reinterpret_cast<float*>(lds_raw);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = wn * WTN + j * 16 + l15;
        const float sc = (a.scale && n < a.Cout) ? a.scale[n] : 1.f, sh = (a.shift && n < a.Cout) ? a.shift[n] : 0.f;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = wm * WTM + i * 16 + 4 * lq + e;
                const int pr = r / SP_CW, pc = r - pr * SP_CW;
                const bool v = pr < SP_CH && (unsigned)(oy_first + pr) < (unsigned)a.Ho && (unsigned)(ox_first + pc) < (unsigned)a.Wo;
                const float s_ = fold(acc[i][j][e], acx[i][j][e]);
                bad = bad || !(fabsf(s_) <= 3.0e38f);
                float t = __fadd_rn(__fmul_rn(s_, sc), sh);
                if (a.relu) t = fmaxf(t, 0.f);
                patch[r * SLD + n] = v ? t : -1.0f;
            }
    }
    if (bad) (void)__hip_atomic_fetch_or(a.range_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (the builtin: atomicOr() would be a call here, see AMP_SYNCTHREADS)
    AMP_SYNCTHREADS();

    // ---- pool: thread = (pooled pixel q, 8 channels) ----
    if (tid < SP_PH * SP_PW * 8) {
        const int q = tid >> 3, c8 = tid & 7;
        const int ppy = q / SP_PW, ppx = q - ppy * SP_PW;
        const int py = ty * SP_PH + ppy, px = tx * SP_PW + ppx;
        if (py < sp.Hq && px < sp.Wq) {
            float m[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) m[c] = -1.0f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float* src = patch + ((2 * ppy + dy) * SP_CW + 2 * ppx + dx) * SLD + 8 * c8;
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { m[c] = fmaxf(m[c], v0[c]); m[4 + c] = fmaxf(m[4 + c], v1[c]); }
                }
            float* orow = sp.pool + ((size_t)(b * sp.Hq + py) * sp.Wq + px) * 64;
            if (sp.pool_split) {
                f16x8 hi, lo;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const _Float16 h = (_Float16)m[c];
                    hi[c] = h;
                    lo[c] = (_Float16)((m[c] - (float)h) * LO_SCALE);
                }
                const int ch = 8 * c8;
                char* base = reinterpret_cast<char*>(orow) + (ch >> 5) * 128 + (ch & 31) * 2;
                *reinterpret_cast<f16x8*>(base) = hi;
                *reinterpret_cast<f16x8*>(base + 64) = lo;
            } else {
                reinterpret_cast<f32x4*>(orow)[2 * c8] = f32x4{m[0], m[1], m[2], m[3]};
                reinterpret_cast<f32x4*>(orow)[2 * c8 + 1] = f32x4{m[4], m[5], m[6], m[7]};
            }
        }
    }
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
