// amp_mask_distance on the device: the exact squared distance of every mask pixel to the nearest pixel outside its mask, the per-mask
// statistics and the erosion curve of every mask of a pool in one call, without a dense mask or a bit plane.  mask_distance.h restated for
// lanes: the host cuts the masks into pieces (mask_parts.h's items with their first-piece-of-column index, one entry per column of a tight
// box) and the pieces into TILES of 64 rows, so a mask that fills the image spreads over the chip like many small ones.  The launches,
// whatever the number of masks:
//   1. one memset         of the totals (and of the map, when it is asked for);
//   2. md_tile_kernel     one wave per tile, lane = row: md_pixel, the walk outwards from the lane's own column with one binary search in the
//                         mask's column slice per column visited.  Per mask the deepest pixel by one 64-bit atomic max of md_best_key after a
//                         wave reduction, the sum of d2 and the area by one 64-bit atomic add each, the erosion curve as a histogram of md_bin
//                         with one aggregated add per wave and distinct bin; every word of the map is written once by the lane that owns it.
// The host turns the histogram into the curve by a suffix sum (mask_distance_write, shared with the host path).  A lane's work grows with its
// own distance: O(pixels x inscribed radius) in the worst case, and the lanes of a wave wait for the deepest of them; nothing is refused for
// that reason.  No buffer has a size fixed at compile time; memory is linear in pieces + box widths + tiles, and nothing per pixel is allocated
// unless the map is asked for.  Integer arithmetic only; the atomics are integer max / add whose order cannot show.  So the bytes repeat and
// equal the host's (mask_distance_host.hip).  Every loop in the kernel states why it ends; none waits for another lane.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "mask_distance.h"

namespace {

using amp::u64;

struct MdTile { unsigned int item, row0, mask, pad; };      // rows [row0, row0 + 64) of the column of piece `item`, cut at the piece's end

struct MdOut {
    u64 *best, *sum, *area;       // [n]
    unsigned int* hist;           // [n][ncurve + 1], null without a curve
    unsigned int* map;            // the crops back to back, null without a map
    const u64* map_off;           // [n]
};

__global__ __launch_bounds__(256) void md_tile_kernel(amp::MdView v, const amp::MpMask* __restrict__ masks, const MdTile* __restrict__ tiles,
                                                      unsigned int ntiles, int ncurve, MdOut o) {
    const unsigned int t = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (t >= ntiles) return;                                                             // the whole wave
    const MdTile tl = tiles[t];
    const amp::MpMask mk = masks[tl.mask];
    const unsigned int S = v.S[tl.item], E = v.E[tl.item], c = S / (unsigned)v.h, cb = c * (unsigned)v.h;
    const int s = (int)(S - cb), e = (int)(E - cb), r = (int)(tl.row0 + lane);
    const bool active = r < e;
    unsigned int d2 = 0;
    if (active) d2 = amp::md_pixel(v, mk, r, (int)c, s, e);
    u64 key = active ? amp::md_best_key(d2, cb + (unsigned)r) : 0ull;
    for (int k = 32; k > 0; k >>= 1) {                                                   // ends: six steps
        const u64 other = __shfl_down(key, k, 64);
        key = other > key ? other : key;
    }
    const u64 total = amp::wave_sum(active && d2 != AMP_DIST_NONE ? (u64)d2 : 0ull);
    const u64 live = __ballot(active);
    if (lane == 0) {
        atomicMax(&o.best[tl.mask], key);
        if (total) atomicAdd(&o.sum[tl.mask], total);
        atomicAdd(&o.area[tl.mask], (u64)amp::popc(live));
    }
    if (o.hist) {
        const int bin = active ? amp::md_bin(d2, ncurve) : -1;
        u64 pending = live;
        while (pending) {                                                                // ends: every turn clears the leader's bit; uniform over the wave
            const int leader = amp::ctz(pending);
            const int b = __shfl(bin, leader, 64);
            const u64 same = __ballot(bin == b);
            if ((int)lane == leader) atomicAdd(&o.hist[(size_t)tl.mask * (size_t)(ncurve + 1) + (size_t)b], (unsigned int)amp::popc(same));
            pending &= ~same;
        }
    }
    if (o.map && active) o.map[o.map_off[tl.mask] + (u64)(r - mk.r0) * (u64)mk.W + (u64)((int)c - mk.c0)] = d2;
}

// one allocation cut into aligned pieces
struct MdArena {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

int mask_distance_device(amp_ctx* ctx, const amp::MpItems& it, int h, int w, int border_value, int ncurve, const std::vector<u64>& offs,
                         uint32_t* map, amp::MdTotals& t) {
    const size_t n = it.m.size(), bins = (size_t)ncurve + 1;
    std::vector<MdTile> tiles;
    for (size_t i = 0; i < n; ++i)
        for (size_t j = (size_t)it.first[i]; j + 1 < (size_t)it.first[i + 1]; ++j) {      // the pieces; the last item is the END item
            const unsigned int s = it.S[j] % (unsigned)h, len = it.E[j] - it.S[j];
            for (unsigned int a = 0; a < len; a += 64) tiles.push_back(MdTile{(unsigned int)j, s + a, (unsigned int)i, 0u});      // ends: a grows to len
        }
    AMP_REQUIRE(tiles.size() < (1ull << 31), "amp_mask_distance: the masks of one call have %llu tiles of 64 rows (at most 2^31 - 1)",
                (unsigned long long)tiles.size());
    t.best.assign(n, 0); t.sum.assign(n, 0); t.area.assign(n, 0);
    t.hist.assign(ncurve ? n * bins : 0, 0);
    if (tiles.empty()) return AMP_OK;                                                    // no mask has a pixel: the crops are empty too
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_S, d_E, d_col, d_m, d_tiles, d_off, d_out;
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_S, it.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_E, it.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_col, it.col));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_m, it.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_tiles, tiles));
    if (map) AMP_TRY_STATUS(amp::dev_upload(ctx, d_off, offs));
    MdArena a;
    const size_t o_best = a.add(n * 8), o_sum = a.add(n * 8), o_area = a.add(n * 8), o_hist = a.add(ncurve ? n * bins * 4 : 0),
                 o_map = a.add(map ? (size_t)offs[n] * 4 : 0);
    AMP_TRY_STATUS(amp::dev_alloc(d_out, a.total));
    char* A = d_out.as<char>();
    AMP_HIP_CHECK(hipMemsetAsync(A, 0, a.total, st));
    MdOut o;
    o.best = (u64*)(A + o_best); o.sum = (u64*)(A + o_sum); o.area = (u64*)(A + o_area);
    o.hist = ncurve ? (unsigned int*)(A + o_hist) : nullptr;
    o.map = map ? (unsigned int*)(A + o_map) : nullptr;
    o.map_off = map ? d_off.as<u64>() : nullptr;
    const amp::MdView v{d_S.as<uint32_t>(), d_E.as<uint32_t>(), d_col.as<uint32_t>(), h, w, border_value};
    const unsigned int ntiles = (unsigned int)tiles.size();
    hipLaunchKernelGGL(md_tile_kernel, dim3((ntiles + 3u) / 4u), dim3(256), 0, st, v, d_m.as<amp::MpMask>(), d_tiles.as<MdTile>(), ntiles, ncurve, o);
    AMP_HIP_CHECK(hipGetLastError());
    std::vector<unsigned int> hist(t.hist.size());
    AMP_HIP_CHECK(hipMemcpyAsync(t.best.data(), o.best, n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(t.sum.data(), o.sum, n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(t.area.data(), o.area, n * 8, hipMemcpyDeviceToHost, st));
    if (ncurve) AMP_HIP_CHECK(hipMemcpyAsync(hist.data(), o.hist, hist.size() * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    if (map && offs[n]) {
        AMP_HIP_CHECK(hipMemcpyAsync(map, o.map, (size_t)offs[n] * 4, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipStreamSynchronize(st));
    }
    std::copy(hist.begin(), hist.end(), t.hist.begin());
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_distance(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                                 int border_value, unsigned long long* stats, long long* boxes, unsigned long long* curve, int ncurve,
                                 uint32_t* map, unsigned long long map_cap, unsigned long long* map_off, unsigned long long* need) {
    amp::RunPlan plan;
    amp::MpItems items;
    std::vector<u64> offs;
    AMP_TRY_STATUS(amp::mask_distance_check(pool, off, len, n, h, w, border_value, stats, boxes, curve, ncurve, map, map_cap, map_off, need, plan,
                                            items, offs));
    if (map) AMP_TRY_STATUS(amp::mask_distance_capacity(offs, map_cap, need));
    if (n == 0) return AMP_OK;
    amp::MdTotals t;
    if (ctx) AMP_TRY_STATUS(mask_distance_device(ctx, items, h, w, border_value, ncurve, offs, map, t));
    else amp::mask_distance_host(items, h, w, border_value, ncurve, offs, map, t);
    amp::mask_distance_write(plan, t, ncurve, offs, map != nullptr, stats, boxes, curve, map_off);
    return AMP_OK;
}
