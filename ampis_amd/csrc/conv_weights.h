// The weight-layout kernels: split_weights, weight_jobs, unsplit_rows, group_expand.  Not templates: their order is the listing's.
#pragma once
#include "common.h"
#include "lds_ring.h"

namespace {

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
