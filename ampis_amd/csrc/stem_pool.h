// The fused stem + max-pool kernels: stem_pool_f16x3_kernel (preprocessed input) and stem_pool_u8_kernel (uint8 image).
#pragma once
#include "common.h"
#include "lds_ring.h"
#include "conv_args.h"
#include "conv_epilogue.h"
#include "conv_f16x3.h"        // split8

namespace {

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

}  // namespace

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
