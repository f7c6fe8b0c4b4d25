// conv3x3_c64_kernel: 3x3 stride-1 convolution over a 64-channel window (res2, grouped conv2), conv3 optionally fused.
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"

namespace {

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

}  // namespace
