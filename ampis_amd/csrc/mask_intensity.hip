// amp_mask_intensity on the device: the grey-level sums, extremes and histograms of the micrograph under every mask of a pool in one call,
// without a dense mask.  A COCO run list is a list of spans over the column-major flattening of the image, so in a column-major plane every
// run of ones [a, b) is one contiguous range of bytes or halfwords, also where it goes on across a column end.  The launches, whatever the
// number of masks:
//   1. mi_fill_kernel       the per-(mask, channel) words (zeros, all ones in the minimum's slot) and the histograms (zeros);
//   2. mi_transpose_kernel  the uploaded row-major interleaved image into one column-major plane per channel: a 64 x 64 tile of every channel
//                           goes through LDS at a stride of 65 elements, read along the rows, written along the columns; pixel (r, c) lands
//                           at c * h + r of its plane, the COCO position;
//   3. mi_reduce_kernel     one workgroup of 256 per (mask, MI_CHUNK pixel ranks of the mask): a lane finds the run of each of its ranks by a
//                           binary search on the exclusive prefix of the run lengths, consecutive lanes read consecutive elements; per channel
//                           the wave reduces mi_add's sums and issues one 64-bit atomic add per sum and one atomic min and max; the bins of a
//                           histogram gather in an LDS table of nbins words and the non-zero ones are flushed with 32-bit atomic adds.
// The host writes the outputs from those words and the plan's areas (mask_intensity_write, shared with the host path).  No buffer has a size
// fixed at compile time; memory is linear in image + runs + outputs.  Integer arithmetic only; the atomics are integer add / min / max whose
// order cannot show.  So the bytes repeat and equal the host's (mask_intensity_host.hip).  Every loop in the kernels states why it ends; none
// waits for another lane.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "mask_intensity.h"

namespace {

using amp::u64;

constexpr int MI_TILE = 64, MI_PITCH = 65;        // the transpose tile and its odd LDS stride, in elements

struct MiItem { unsigned int mask, rank0; };      // ranks [rank0, rank0 + MI_CHUNK) of the mask's pixels, cut at its area

__global__ __launch_bounds__(256) void mi_fill_kernel(u64* __restrict__ raw, size_t nraw, unsigned int* __restrict__ hist, size_t nhist) {
    const size_t step = (size_t)gridDim.x * 256u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nraw; i += step) raw[i] = (i & 7u) == 5u ? ~0ull : 0ull;       // ends: i grows to nraw
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nhist; i += step) hist[i] = 0u;                                  // ends: i grows to nhist
}

// x / C for the channel counts of the call: constant divisors, no runtime division
__device__ __forceinline__ int mi_div_channels(int x, int C) { return C == 1 ? x : C == 2 ? x >> 1 : C == 3 ? x / 3 : x >> 2; }

// img: [h][w][C] as uploaded; planes: [C][w][h].  Grid (ceil(w / 64), ceil(h / 64)).
template <typename T>
__global__ __launch_bounds__(256) void mi_transpose_kernel(const T* __restrict__ img, T* __restrict__ planes, int h, int w, int C) {
    __shared__ T tile[4 * MI_TILE * MI_PITCH];
    const int r0 = (int)blockIdx.y * MI_TILE, c0 = (int)blockIdx.x * MI_TILE, row = MI_TILE * C;
    for (int idx = (int)threadIdx.x; idx < MI_TILE * row; idx += 256) {                    // ends: idx grows; consecutive lanes read consecutive elements of an image row
        const int r = mi_div_channels(idx, C) >> 6, e = idx - r * row, c = mi_div_channels(e, C), ch = e - c * C;
        if (r0 + r < h && c0 + c < w) tile[(ch * MI_TILE + r) * MI_PITCH + c] = img[((size_t)(r0 + r) * (size_t)w + (size_t)(c0 + c)) * (size_t)C + (size_t)ch];
    }
    __syncthreads();
    for (int idx = (int)threadIdx.x; idx < C * MI_TILE * MI_TILE; idx += 256) {            // ends: idx grows; consecutive lanes write consecutive rows of a plane column
        const int ch = idx >> 12, c = (idx >> 6) & 63, r = idx & 63;
        if (r0 + r < h && c0 + c < w) planes[(size_t)ch * (size_t)h * (size_t)w + (size_t)(c0 + c) * (size_t)h + (size_t)(r0 + r)] = tile[(ch * MI_TILE + r) * MI_PITCH + c];
    }
}

__device__ __forceinline__ unsigned int wave_min(unsigned int v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned int x = __shfl_down(v, o, 64); v = x < v ? x : v; }       // ends: six steps
    return v;
}
__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned int x = __shfl_down(v, o, 64); v = x > v ? x : v; }       // ends: six steps
    return v;
}

// S: the run starts, P: the pixels of the mask's runs before each, both indexed like the plan (mask.ro + k; P[ro + n] = the area).
// Dynamic LDS: nbins words (none without a histogram).
template <typename T>
__global__ __launch_bounds__(256) void mi_reduce_kernel(const T* __restrict__ planes, size_t plane, int h, int C, const unsigned int* __restrict__ S,
                                                        const unsigned int* __restrict__ P, const amp::RunMask* __restrict__ masks,
                                                        const MiItem* __restrict__ items, int hist_shift, unsigned int nbins, u64* __restrict__ raw,
                                                        unsigned int* __restrict__ hist) {
    extern __shared__ unsigned int bins[];
    const MiItem it = items[blockIdx.x];
    const amp::RunMask mk = masks[it.mask];
    const unsigned int *s = S + mk.ro, *p = P + mk.ro;
    const unsigned int tid = threadIdx.x;
    unsigned int pos[amp::MI_PER_LANE], row[amp::MI_PER_LANE], col[amp::MI_PER_LANE];      // of the lane's pixels; pos all ones: none
#pragma unroll
    for (int j = 0; j < amp::MI_PER_LANE; ++j) {
        const unsigned int rank = it.rank0 + (unsigned)j * 256u + tid;
        pos[j] = 0xffffffffu; row[j] = 0u; col[j] = 0u;
        if (rank < mk.area) {
            int lo = 0, hi = mk.n;                                                         // p[lo] <= rank < p[hi]: p[0] = 0, p[n] = the area
            while (hi - lo > 1) {                                                          // ends: hi - lo halves
                const int mid = (lo + hi) >> 1;
                if (p[mid] <= rank) lo = mid; else hi = mid;
            }
            pos[j] = s[lo] + (rank - p[lo]);                                               // inside run lo: below h * w
            col[j] = pos[j] / (unsigned)h;
            row[j] = pos[j] - col[j] * (unsigned)h;
        }
    }
    for (int ch = 0; ch < C; ++ch) {                                                       // ends: C <= 4; uniform over the workgroup, as is nbins
        const T* pl = planes + (size_t)ch * plane;
        if (nbins) {
            for (unsigned int b = tid; b < nbins; b += 256u) bins[b] = 0u;                 // ends: b grows to nbins
            __syncthreads();
        }
        amp::MiSums a = amp::mi_none();
#pragma unroll
        for (int j = 0; j < amp::MI_PER_LANE; ++j)
            if (pos[j] != 0xffffffffu) {
                const unsigned int v = pl[pos[j]];
                amp::mi_add(a, v, row[j], col[j]);
                if (nbins) atomicAdd(&bins[v >> hist_shift], 1u);                          // v < 2^depth: below nbins
            }
        const u64 sv = amp::wave_sum(a.sv), svv = amp::wave_sum(a.svv), srv = amp::wave_sum(a.srv), scv = amp::wave_sum(a.scv);
        const unsigned int mn = wave_min(a.mn), mx = wave_max(a.mx);
        if ((tid & 63u) == 0u && mn != 0xffffffffu) {                                      // a wave with a pixel: v < 2^16 never is all ones
            u64* o = raw + ((size_t)it.mask * (size_t)C + (size_t)ch) * amp::MI_RAW;
            if (sv) { atomicAdd(&o[1], sv); atomicAdd(&o[2], svv); }
            if (srv) atomicAdd(&o[3], srv);
            if (scv) atomicAdd(&o[4], scv);
            atomicMin(&o[5], (u64)mn);
            atomicMax(&o[6], (u64)mx);
        }
        if (nbins) {
            __syncthreads();
            unsigned int* g = hist + ((size_t)it.mask * (size_t)C + (size_t)ch) * (size_t)nbins;
            for (unsigned int b = tid; b < nbins; b += 256u) {                             // ends: b grows to nbins
                const unsigned int k = bins[b];
                if (k) atomicAdd(&g[b], k);
            }
            __syncthreads();                                                               // the table is cleared again for the next channel
        }
    }
}

template <typename T>
void mi_launch(hipStream_t st, const void* d_img, void* d_planes, int h, int w, int C, const unsigned int* S, const unsigned int* P,
               const amp::RunMask* masks, const MiItem* items, unsigned int nitems, int hist_shift, unsigned int nbins, u64* raw, unsigned int* hist) {
    hipLaunchKernelGGL(mi_transpose_kernel<T>, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 63) / 64)), dim3(256), 0, st,
                       static_cast<const T*>(d_img), static_cast<T*>(d_planes), h, w, C);
    hipLaunchKernelGGL(mi_reduce_kernel<T>, dim3(nitems), dim3(256), (size_t)nbins * 4, st, static_cast<const T*>(d_planes), (size_t)h * (size_t)w, h,
                       C, S, P, masks, items, hist_shift, nbins, raw, hist);
}

int mask_intensity_device(amp_ctx* ctx, const amp::RunPlan& plan, int h, int w, const void* image, int C, int depth, int hist_shift, u64 nbins,
                          std::vector<u64>& raw, uint32_t* hist) {
    const size_t n = plan.m.size(), nraw = n * (size_t)C * amp::MI_RAW, nhist = n * (size_t)C * (size_t)nbins;
    std::vector<uint32_t> P(plan.S.size(), 0);
    std::vector<MiItem> items;
    for (size_t i = 0; i < n; ++i) {
        const amp::RunMask& mk = plan.m[i];
        uint32_t before = 0;
        for (int k = 0; k < mk.n; ++k) {
            P[mk.ro + (size_t)k] = before;
            before += plan.E[mk.ro + (size_t)k] - plan.S[mk.ro + (size_t)k];
        }
        P[mk.ro + (size_t)mk.n] = before;                                                // the closing entry: the area
        for (uint32_t a = 0; a < mk.area; a += (uint32_t)amp::MI_CHUNK) items.push_back(MiItem{(unsigned int)i, a});      // ends: a grows to the area <= 2^30
    }
    AMP_REQUIRE(items.size() < (1ull << 31), "amp_mask_intensity: the masks of one call have %llu work items of %d pixels (at most 2^31 - 1)",
                (unsigned long long)items.size(), amp::MI_CHUNK);
    if (items.empty()) {                                                                 // no mask has a pixel: the words the fill would leave
        raw.assign(nraw, 0);
        for (size_t i = 5; i < nraw; i += amp::MI_RAW) raw[i] = ~0ull;
        if (nhist) std::fill(hist, hist + nhist, 0u);
        return AMP_OK;
    }
    raw.resize(nraw);
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t elem = depth == 8 ? 1 : 2, img_bytes = (size_t)h * (size_t)w * (size_t)C * elem;
    amp::DevBuf d_img, d_planes, d_S, d_P, d_m, d_items, d_raw, d_hist;
    AMP_TRY_STATUS(amp::dev_alloc(d_img, img_bytes));
    AMP_TRY_STATUS(amp::dev_alloc(d_planes, img_bytes));
    AMP_HIP_CHECK(hipMemcpyAsync(d_img.p, image, img_bytes, hipMemcpyHostToDevice, st));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_S, plan.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_P, P));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_m, plan.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_items, items));
    AMP_TRY_STATUS(amp::dev_alloc(d_raw, nraw * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_hist, nhist * 4));
    const size_t words = std::max(nraw, nhist);
    hipLaunchKernelGGL(mi_fill_kernel, dim3((unsigned)std::min<size_t>((words + 255) / 256, 4096)), dim3(256), 0, st, d_raw.as<u64>(), nraw,
                       d_hist.as<unsigned int>(), nhist);
    AMP_HIP_CHECK(hipGetLastError());
    if (depth == 8)
        mi_launch<uint8_t>(st, d_img.p, d_planes.p, h, w, C, d_S.as<unsigned int>(), d_P.as<unsigned int>(), d_m.as<amp::RunMask>(), d_items.as<MiItem>(),
                           (unsigned int)items.size(), hist_shift, (unsigned int)nbins, d_raw.as<u64>(), d_hist.as<unsigned int>());
    else
        mi_launch<uint16_t>(st, d_img.p, d_planes.p, h, w, C, d_S.as<unsigned int>(), d_P.as<unsigned int>(), d_m.as<amp::RunMask>(), d_items.as<MiItem>(),
                            (unsigned int)items.size(), hist_shift, (unsigned int)nbins, d_raw.as<u64>(), d_hist.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    AMP_HIP_CHECK(hipMemcpyAsync(raw.data(), d_raw.p, nraw * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    if (nhist) {
        AMP_HIP_CHECK(hipMemcpyAsync(hist, d_hist.p, nhist * 4, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipStreamSynchronize(st));
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_intensity(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                                  const void* image, int channels, int depth, int hist_shift, unsigned long long* vals, uint32_t* hist,
                                  unsigned long long hist_cap, unsigned long long* need) {
    amp::RunPlan plan;
    u64 nbins = 0;
    AMP_TRY_STATUS(amp::mask_intensity_check(pool, off, len, n, h, w, image, channels, depth, hist_shift, vals, hist, need, plan, nbins));
    if (nbins) AMP_TRY_STATUS(amp::mask_intensity_capacity(n, channels, nbins, hist_cap, need));
    if (n == 0) return AMP_OK;
    std::vector<u64> raw;
    if (ctx) AMP_TRY_STATUS(mask_intensity_device(ctx, plan, h, w, image, channels, depth, hist_shift, nbins, raw, hist));
    else amp::mask_intensity_host(plan, h, w, image, channels, depth, hist_shift, nbins, raw, hist);
    amp::mask_intensity_write(plan, channels, raw, vals);
    return AMP_OK;
}
