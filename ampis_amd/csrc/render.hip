// Instance overlays on the device (ampis_amd/utils/visualizer.py, Visualizer.overlay_instances: per instance a full-image blend, the four shifted
// ANDs of the edge rule and a box frame, about ten NumPy passes over the image each).  Here the masks stay run lists: the result at a pixel
// depends only on the ordered list of instances that cover it, so one workgroup of one wave owns a tile of 64 rows x 64 columns -- one word row
// of the column-major bit planes of run_list.h -- and replays every instance that meets the tile, in draw order, on the tile's pixels in LDS:
//   * the lanes test 64 instances at a time (the tight box of the plan, the four outline rectangles of the check) and a ballot leaves the hits,
//     walked in order; a tile nothing meets is neither read nor written;
//   * for a mask that meets the tile lane c builds the 64-row word of its column from the run ends (one binary search, then the runs in order)
//     together with the mask one row above and below; the words left and right come from the neighbouring lanes, the two outer columns of the
//     tile are built by lanes 0 and 63; render_inner (mask_analysis.h, shared with the host) applies the edge rule and the image border;
//   * the instance's 768-byte fill table is staged in LDS and every mask pixel of the lane's column is looked up or set to the edge colour;
//     the outline rectangles become one 64-row word per lane and are set to the box colour.
// LDS: pixel (r, c) of the tile at c * 196 + 3 r -- a lane walks its own column, the odd dword stride keeps the lanes on distinct banks.
// One launch per call whatever n is, no atomics, every byte of the image written once by the workgroup of its tile: the bytes repeat and
// equal the host's (mask_analysis_host.hip).
#include <string.h>

#include <vector>

#include "common.h"
#include "mask_analysis.h"

namespace {

using amp::RunMask;
using amp::u64;

constexpr int RN_STRIDE = 196;                    // bytes of one tile column in LDS: 64 rows x 3 channels + 4

__global__ __launch_bounds__(64) void render_kernel(uint8_t* __restrict__ img, int h, int w, int tiles_x, const RunMask* __restrict__ rm,
                                                    const unsigned int* __restrict__ S, const unsigned int* __restrict__ E, int n,
                                                    const uint8_t* __restrict__ tab, const uint8_t* __restrict__ edge,
                                                    const int* __restrict__ rects, const uint8_t* __restrict__ box_rgb) {
    __shared__ uint8_t px[64 * RN_STRIDE];
    __shared__ unsigned int tb[192];
    const int lane = threadIdx.x;
    const int row0 = (int)(blockIdx.x / (unsigned)tiles_x) << 6, col0 = (int)(blockIdx.x % (unsigned)tiles_x) << 6;
    const int rows = min(64, h - row0), cols = min(64, w - col0), col = col0 + lane;
    uint8_t* mine = px + lane * RN_STRIDE;
    const uint8_t* t8 = reinterpret_cast<const uint8_t*>(tb);
    bool loaded = false;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool mhit = false, bhit = false;
        if (i < n) {
            if (rm) {
                const RunMask k = rm[i];
                mhit = k.n > 0 && k.r0 < row0 + rows && k.r1 > row0 && k.c0 < col0 + cols && k.c1 > col0;
            }
            for (int q = 0; rects && q < 4; ++q) {
                const int* r = rects + 16 * (size_t)i + 4 * q;
                bhit |= r[0] < r[1] && r[2] < r[3] && r[0] < row0 + rows && r[1] > row0 && r[2] < col0 + cols && r[3] > col0;
            }
        }
        const u64 mm = __ballot(mhit), bm = __ballot(bhit);
        for (u64 any = mm | bm; any; any &= any - 1) {                           // uniform over the wave
            const int j = amp::ctz(any), ii = base + j;
            if (!loaded) {
                for (int r = 0; r < rows; ++r) {
                    const uint8_t* src = img + ((size_t)(row0 + r) * w + col0) * 3;
                    for (int b = lane; b < cols * 3; b += 64) px[(b / 3) * RN_STRIDE + r * 3 + b % 3] = src[b];
                }
                loaded = true;
            }
            __syncthreads();                                                     // the tile is there; the last instance is done with the table
            if ((mm >> j) & 1) {
                const RunMask k = rm[ii];
                const unsigned int* t32 = reinterpret_cast<const unsigned int*>(tab + 768 * (size_t)ii);
                for (int q = lane; q < 192; q += 64) tb[q] = t32[q];
                __syncthreads();
                const unsigned int *Sk = S + k.ro, *Ek = E + k.ro;
                u64 m = 0, up = 0, down = 0;
                if (lane < cols && col >= k.c0 && col < k.c1) {
                    const unsigned int cb = (unsigned)col * (unsigned)h, a = cb + (unsigned)row0;
                    m = amp::mask_word_halo(Sk, Ek, k.n, cb, cb + (unsigned)h, a, min(a + 64u, cb + (unsigned)h), &up, &down);
                }
                u64 e = 0;
                if (edge) {
                    u64 left = __shfl_up(m, 1, 64), right = __shfl_down(m, 1, 64);
                    if (lane == 0 || lane == 63) {                               // the tile's outer columns
                        const int nc = lane ? col + 1 : col - 1;
                        u64 side = 0;
                        if (m && nc >= 0 && nc < w) {
                            const unsigned int a = (unsigned)nc * (unsigned)h + (unsigned)row0;
                            side = amp::mask_word(Sk, Ek, k.n, a, min(a + 64u, ((unsigned)nc + 1u) * (unsigned)h));
                        }
                        if (lane) right = side; else left = side;
                    }
                    e = m & ~amp::render_inner(m, (m << 1) | up, (m >> 1) | (down << 63), left, right, row0, col, h, w);
                }
                const uint8_t er = edge ? edge[3 * (size_t)ii] : 0, eg = edge ? edge[3 * (size_t)ii + 1] : 0, eb = edge ? edge[3 * (size_t)ii + 2] : 0;
                for (u64 x = m; x; x &= x - 1) {
                    const int r = amp::ctz(x);
                    uint8_t* p = mine + 3 * r;
                    if ((e >> r) & 1) {
                        p[0] = er; p[1] = eg; p[2] = eb;
                    } else {
                        p[0] = t8[3 * p[0]]; p[1] = t8[3 * p[1] + 1]; p[2] = t8[3 * p[2] + 2];
                    }
                }
            }
            if ((bm >> j) & 1) {
                u64 bw = 0;
                for (int q = 0; q < 4; ++q) {
                    const int* r = rects + 16 * (size_t)ii + 4 * q;
                    const int lo = max(r[0] - row0, 0), hi = min(r[1] - row0, 64);
                    if (col >= r[2] && col < r[3] && lo < hi) bw |= amp::word_span(lo, hi);
                }
                const uint8_t br = box_rgb[3 * (size_t)ii], bg = box_rgb[3 * (size_t)ii + 1], bb = box_rgb[3 * (size_t)ii + 2];
                for (u64 x = bw; x; x &= x - 1) {
                    uint8_t* p = mine + 3 * amp::ctz(x);
                    p[0] = br; p[1] = bg; p[2] = bb;
                }
            }
        }
    }
    if (!loaded) return;
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
        uint8_t* dst = img + ((size_t)(row0 + r) * w + col0) * 3;
        for (int b = lane; b < cols * 3; b += 64) dst[b] = px[(b / 3) * RN_STRIDE + r * 3 + b % 3];
    }
}

static int render_device(amp_ctx* ctx, const amp::RunPlan& runs, const uint8_t* fill_tab, const uint8_t* edge_rgb, const std::vector<int>& rects,
                         const uint8_t* box_rgb, int n, int h, int w, const uint8_t* image, uint8_t* out) {
    const bool masks = !runs.m.empty(), boxes = !rects.empty();
    const size_t bytes = (size_t)h * w * 3;
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_img, d_rm, d_S, d_E, d_tab, d_edge, d_rects, d_box;
    AMP_TRY_STATUS(amp::dev_alloc(d_img, bytes));
    AMP_HIP_CHECK(hipMemcpyAsync(d_img.p, image, bytes, hipMemcpyHostToDevice, st));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_rm, runs.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_S, runs.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_E, runs.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_rects, rects));
    if (masks) {
        AMP_TRY_STATUS(amp::dev_alloc(d_tab, (size_t)n * 768));
        AMP_HIP_CHECK(hipMemcpyAsync(d_tab.p, fill_tab, (size_t)n * 768, hipMemcpyHostToDevice, st));
    }
    if (masks && edge_rgb) {
        AMP_TRY_STATUS(amp::dev_alloc(d_edge, (size_t)n * 3));
        AMP_HIP_CHECK(hipMemcpyAsync(d_edge.p, edge_rgb, (size_t)n * 3, hipMemcpyHostToDevice, st));
    }
    if (boxes) {
        AMP_TRY_STATUS(amp::dev_alloc(d_box, (size_t)n * 3));
        AMP_HIP_CHECK(hipMemcpyAsync(d_box.p, box_rgb, (size_t)n * 3, hipMemcpyHostToDevice, st));
    }
    const int tiles_x = (w + 63) >> 6, tiles_y = (h + 63) >> 6;                  // at most 2^24 tiles: h * w <= 2^30
    hipLaunchKernelGGL(render_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(64), 0, st, d_img.as<uint8_t>(), h, w, tiles_x,
                       masks ? d_rm.as<RunMask>() : nullptr, d_S.as<unsigned int>(), d_E.as<unsigned int>(), n, d_tab.as<uint8_t>(),
                       d_edge.as<uint8_t>(), boxes ? d_rects.as<int>() : nullptr, d_box.as<uint8_t>());
    AMP_HIP_CHECK(hipGetLastError());
    AMP_HIP_CHECK(hipMemcpyAsync(out, d_img.p, bytes, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    return AMP_OK;
}

}  // namespace

extern "C" int amp_render_instances(amp_ctx* ctx, const uint8_t* image, int h, int w, const uint32_t* pool, const unsigned long long* off,
                                    const int* len, int n, const uint8_t* fill_tab, const uint8_t* edge_rgb, const int* boxes,
                                    const uint8_t* box_rgb, int lw, uint8_t* out) {
    amp::RunPlan runs;
    std::vector<int> rects;
    AMP_TRY_STATUS(amp::render_check(image, h, w, pool, off, len, n, fill_tab, edge_rgb, boxes, box_rgb, lw, out, runs, rects));
    if (ctx && n > 0 && (pool || boxes)) return render_device(ctx, runs, fill_tab, edge_rgb, rects, box_rgb, n, h, w, image, out);
    if (out != image) memmove(out, image, (size_t)h * w * 3);
    return amp::render_host(runs, fill_tab, edge_rgb, rects, box_rgb, n, h, w, out);
}
