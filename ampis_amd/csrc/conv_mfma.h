// conv_mfma_kernel: the fp32 implicit-GEMM convolution, operands staged through registers (any Cin).
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"

namespace {

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

}  // namespace
