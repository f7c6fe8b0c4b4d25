// Convolution kernels: vector types, the K-step, ConvArgs and the GEMM row -> pixel decomposition.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;      // K-slice per step (floats)
constexpr int LDS_LD = 36;  // padded row length in LDS (floats): 144 B rows -> conflict-free ds_read_b128

struct ConvArgs {
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    const float* res;
    const float* mask;   // optional, indexed like y: y = mask > 0 ? y : 0 (ReLU backward of the tensor the gradient belongs to)
    float* y;
    int B, H, W, Cin;
    int Ho, Wo, Cout;
    int KH, KW, stride, pad;
    int M, K, nsteps;
    int relu, res_mode, out_mode;
    int ntn;  // number of N tiles
    float in_scale, out_scale;   // f16x3 kernels: activations are multiplied by in_scale (a power of two) before the split, the sum by out_scale
    int y_split;            // 1: y is written in the split hi|lo' row format (out_mode 0, Cout % 32 == 0): the next conv's operand
    // out_mode 3 (conv_split_kernel<128,256> only): the ConvTranspose 2x2 of the mask head with its consumers fused into the epilogue --
    // ReLU, the 1x1 predictor row of the detection's class, sigmoid -- so the [N,28,28,256] tensor never exists (see conv_epilogue_predict)
    const float* pred_w;    // [K][C2] predictor weights (fp32), C2 = Cout / 4 = 256
    const float* pred_b;    // [K]
    const int* pred_cls;    // [B] class of each RoI (row b of the input)
    int pred_K;
    // out_mode 4 (conv_split_kernel<128,256> only): the RPN head's tail -- ReLU, then the 16 predictor rows (3 objectness + 12 deltas + pad) as a
    // second f16x3 product in the epilogue (conv_epilogue_rpn); the 256-channel hidden tensor is never written
    const float* rpn_w;     // [16][Cout] split rows
    const float* rpn_b;     // [16]
    float* rpn_pred;        // [M][16 NBP], NBP = 1, 2, 3 blocks of 16 predictor rows (the epilogue's template argument; amp::rpn_ld)
    float* prob;            // [B][2Ho][2Wo] mask probabilities
    int res_split;          // 1: res is in that format too (decoded in the epilogue: hi + lo' * 2^-11, exact in fp32)
    int mask_split;         // 1: the ReLU mask tensor (training: the forward activation) is in that format (AMP_FMT_MASK_SPLIT)
    int direct_epi;         // conv_split_kernel: split rows written straight from the accumulators (0: staged through LDS, the form before it; always 1 now)
    int stagger;            // conv_split_kernel: the two halves of the workgroup ping-pong between loading and multiplying (0: lockstep; EXPERIMENT switch AMP_STAGGER)
    int* range_flag;        // f16x3 kernels: set to 1 when an accumulator is not finite (operand beyond fp16 range)
    int cin_win, grouped;   // K runs over KH*KW*cin_win input channels; grouped: the window of N-tile n0 starts at channel n0
    int nblk;
    int korder;             // conv_split_kernel: 0 = K runs tap-major (ky, kx, then the 32-channel slices), 1 = channel-major (slice, then the KH*KW taps:
                            // the nine taps of a slice re-read the same cache lines within nine K-steps, while they are still in the XCD's L2)
    unsigned int div_howo_mul, div_wo_mul;   // x / d == (x * mul) >> shr for every x < 2^29 (Granlund-Montgomery, mul = ceil(2^shr / d))
    int div_howo_shr, div_wo_shr;
};

__device__ __forceinline__ unsigned int fastdiv(unsigned int x, unsigned int mul, int shr) {
    return (unsigned int)(((unsigned long long)x * mul) >> shr);
}

// GEMM row m -> output pixel (image b, row oy, column ox) through the two multiply-shift divisions conv_run prepared
__device__ __forceinline__ void conv_pixel(const ConvArgs& a, unsigned int m, unsigned int& b, unsigned int& oy, unsigned int& ox) {
    b = fastdiv(m, a.div_howo_mul, a.div_howo_shr);
    const unsigned int rem = m - b * (unsigned int)(a.Ho * a.Wo);
    oy = fastdiv(rem, a.div_wo_mul, a.div_wo_shr);
    ox = rem - oy * (unsigned int)a.Wo;
}

}  // namespace
