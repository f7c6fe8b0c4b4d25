// amp_mask_morphology on the device: the masks of one pool dilated, eroded, opened, closed or reduced to a boundary band in one call, without
// a dense mask or a plane per mask.  morphology.h restated for lanes: a mask's result is the class of an integer cover, the cover is the prefix
// sum of +weight / -weight events at positions col * h + row, and a boundary lies where the class changes.  The technique is that of stages
// 9 - 16 of polygon_runs.hip with other events and another threshold; the last two stages are the kernels both share.  The launches of one PASS, whatever the
// call holds (R runs, T items = pieces x offsets, C events, n masks):
//   1. mo_len_kernel      one lane per run: its items, the columns it crosses times the D offsets of a piece;
//   2. exclusive scan     of the items (rocprim): where the items of every run start among the T;
//   3. mo_event_kernel    COUNT: a fixed grid, every workgroup a contiguous slice of the items, one lane per (piece, offset): two events or none;
//   4. exclusive scan     of the workgroup sums.  The host reads C, refuses 2^31 or more and sizes the arrays;
//   5. mo_event_kernel    EMIT: the same walk with a workgroup scan (compaction.h): the keys (mask, position, own, closes) of every event;
//   6. radix sort         of the keys (rocprim): equal keys are indistinguishable, so any order among them gives the same array;
//   7. mo_delta_kernel    the weight of every sorted key, and where every mask starts;
//   8. inclusive scan     of the weights: the cover of the pixels behind each event (64-bit: morphology.h says why);
//   9. mo_bound_kernel    one lane per group of equal (mask, position): a boundary where the class of the cover in front of the group differs
//                         from the class behind it, each with the threshold of its own column; never at h * w;
//  10. exclusive scan     of the boundary flags;
//  11. count_offsets_kernel  (compaction.h) where every mask's counts start (its boundaries and the closing count).  The host reads them;
//  12. mo_place_kernel    the boundary positions, in order;
//  13. run_counts_kernel  (compaction.h) the last pass: one lane per count, boundary minus the boundary before; the runs of ones give box and
//                         area by atomic min / max / add.  The host reports the need and refuses a capacity that is too small before this launch;
//      mo_runs_kernel     the first pass of an opening or closing: one lane per run of the intermediate result, which stays on the device.
// No buffer has a size fixed at compile time, and memory is linear in runs + events + counts.  Integer arithmetic only; the atomics are integer
// min / max / add whose order cannot show; every other word is written once by the lane that owns it.  So the bytes repeat and equal the
// host's (morphology_host.hip).  Every loop in a kernel states why it ends; none waits for another lane.
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "common.h"
#include "compaction.h"
#include "mask_analysis.h"
#include "morphology.h"

namespace {

using amp::u64;

constexpr unsigned int MO_GRID = 2048;            // the workgroups of the walk over the items, whatever T is
constexpr int MO_POS_SHIFT = 2;                   // key = mask << 33 | position << 2 | own << 1 | closes; a position is at most h * w <= 2^30
constexpr int MO_MASK_SHIFT = 33;

struct MoPass {
    int h, w, pass, r, rr, border, D;             // rr = min(r, w - 1): the offsets that can stay inside the image; D = 2 rr + 1 (+ 1 in a band)
    const int* hh;                                // [r + 1]
};

// the first of the n ascending keys that is >= x (n when there is none)
__device__ __forceinline__ unsigned int mo_lower_bound(const u64* __restrict__ a, unsigned int n, u64 x) {
    unsigned int lo = 0, hi = n;
    while (lo < hi) {                                                                    // ends: hi - lo halves
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// elen[R] = 0 closes the array the scan reads
__global__ __launch_bounds__(256) void mo_len_kernel(const unsigned int* __restrict__ S, const unsigned int* __restrict__ E, unsigned int R, int h,
                                                     int D, u64* __restrict__ elen) {
    for (unsigned int j = blockIdx.x * 256 + threadIdx.x; j <= R; j += gridDim.x * 256)  // ends: j grows by the grid (R < 2^31)
        elen[j] = j == R ? 0ull : (u64)((E[j] - 1) / (unsigned)h - S[j] / (unsigned)h + 1) * (u64)D;
}

// Workgroup b walks items [b * slice, (b + 1) * slice) of the T = eoff[R], slice a multiple of 256 that depends on T only.  COUNT: bsum[b] = its
// events (bsum[gridDim.x] = 0 closes the array the scan reads).  EMIT (boff = the exclusive scan of bsum): the keys, in item order.
template <bool EMIT>
__global__ __launch_bounds__(256) void mo_event_kernel(const unsigned int* __restrict__ S, const unsigned int* __restrict__ E,
                                                       const u64* __restrict__ eoff, unsigned int R, const u64* __restrict__ roff, int n, MoPass g,
                                                       u64* __restrict__ bsum, const u64* __restrict__ boff, u64* __restrict__ keys) {
    __shared__ unsigned int wtot[4];
    const u64 T = eoff[R], chunks = (T + 255) / 256, slice = ((chunks + gridDim.x - 1) / gridDim.x) * 256;
    const u64 first = min((u64)blockIdx.x * slice, T), last = min(first + slice, T);
    u64 at = EMIT ? boff[blockIdx.x] : 0ull;
    for (u64 t0 = first; t0 < last; t0 += 256) {                                         // ends: t0 grows to last; uniform over the workgroup
        const u64 t = t0 + threadIdx.x;
        bool hit = false;
        u64 open = 0, close = 0;
        if (t < last) {
            const int run = amp::owner_of(eoff, (int)R, t);                              // eoff[run] <= t < eoff[run + 1]: a run with items
            const u64 q = t - eoff[run];
            const int ci = (int)(q / (u64)g.D), k = (int)(q % (u64)g.D);
            const unsigned int s = S[run], e = E[run], cf = s / (unsigned)g.h, cl = (e - 1) / (unsigned)g.h, col = cf + (unsigned)ci;
            const int srow = ci == 0 ? (int)(s - cf * (unsigned)g.h) : 0, erow = col == cl ? (int)(e - cl * (unsigned)g.h) : g.h;
            const bool own = k == 2 * g.rr + 1;                                          // only a band has this item
            const int dx = own ? 0 : k - g.rr, xo = (int)col + dx;
            int a = srow, b = erow;
            hit = own || (xo >= 0 && xo < g.w && amp::mo_interval(g.pass, g.border, g.h, srow, erow, g.hh[dx < 0 ? -dx : dx], &a, &b));
            if (hit) {
                const u64 mask = (u64)amp::owner_of(roff, n, (u64)run), base = (u64)xo * (u64)g.h;
                open = (mask << MO_MASK_SHIFT) | ((base + (u64)a) << MO_POS_SHIFT) | (own ? 2ull : 0ull);
                close = (mask << MO_MASK_SHIFT) | ((base + (u64)b) << MO_POS_SHIFT) | (own ? 2ull : 0ull) | 1ull;
            }
        }
        unsigned int total;
        const unsigned int before = block_before_256(hit ? 2u : 0u, wtot, &total);
        if (EMIT && hit) { keys[at + before] = open; keys[at + before + 1] = close; }
        at += total;
    }
    if (!EMIT && threadIdx.x == 0) {
        bsum[blockIdx.x] = at;
        if (blockIdx.x == 0) bsum[gridDim.x] = 0;
    }
}

__global__ __launch_bounds__(256) void mo_delta_kernel(const u64* __restrict__ skeys, unsigned int C, int n, long long* __restrict__ delta,
                                                       unsigned int* __restrict__ ioff) {
    const unsigned int items = max(C, (unsigned)n + 1u);
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < items; i += gridDim.x * 256) {   // ends: i grows by the grid
        if (i < C) {
            const long long wt = (skeys[i] & 2ull) ? amp::MO_OWN : 1ll;
            delta[i] = (skeys[i] & 1ull) ? -wt : wt;
        }
        if (i <= (unsigned)n) ioff[i] = mo_lower_bound(skeys, C, (u64)i << MO_MASK_SHIFT);
    }
}

// cover[i] = the sum of the weights up to and including i.  The events of a mask sum to 0, so every mask starts from a cover of 0.
__global__ __launch_bounds__(256) void mo_bound_kernel(const u64* __restrict__ skeys, unsigned int C, const long long* __restrict__ cover,
                                                       const unsigned int* __restrict__ ioff, MoPass g, unsigned int area,
                                                       unsigned int* __restrict__ flags) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i <= C; i += gridDim.x * 256) { // ends: i grows by the grid
        unsigned int flag = 0;
        if (i < C) {
            const u64 grp = skeys[i] >> MO_POS_SHIFT;
            const unsigned int pos = (unsigned int)(grp & 0x7fffffffull);
            if (pos < area && (i == 0 || (skeys[i - 1] >> MO_POS_SHIFT) != grp)) {
                const unsigned int s0 = ioff[(unsigned int)(skeys[i] >> MO_MASK_SHIFT)], tail = mo_lower_bound(skeys, C, (grp + 1ull) << MO_POS_SHIFT) - 1u;
                const long long before = i == s0 ? 0ll : cover[i - 1], after = cover[tail];
                const bool was = pos > 0 && amp::mo_class(g.pass, before, amp::mo_threshold((int)((pos - 1u) / (unsigned)g.h), g.r, g.w, g.border));
                const bool is = amp::mo_class(g.pass, after, amp::mo_threshold((int)(pos / (unsigned)g.h), g.r, g.w, g.border));
                flag = was != is ? 1u : 0u;
            }
        }
        flags[i] = flag;                                                                 // flags[C] = 0 closes the array the scan reads
    }
}

__global__ __launch_bounds__(256) void mo_place_kernel(const u64* __restrict__ skeys, unsigned int C, const unsigned int* __restrict__ flags,
                                                       const unsigned int* __restrict__ bidx, unsigned int* __restrict__ bnd) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < C; i += gridDim.x * 256)   // ends: i grows by the grid
        if (flags[i]) bnd[bidx[i]] = (unsigned int)((skeys[i] >> MO_POS_SHIFT) & 0x7fffffffull);
}

// The runs of an intermediate result: run j of mask i, roff2[i] <= j < roff2[i + 1], is the pixels between its boundaries 2 jj and 2 jj + 1;
// the last run of a mask with an odd number of boundaries reaches h * w.
__global__ __launch_bounds__(256) void mo_runs_kernel(const unsigned int* __restrict__ bnd, const u64* __restrict__ coff, const u64* __restrict__ roff2,
                                                      int n, unsigned int R2, unsigned int area, unsigned int* __restrict__ S2,
                                                      unsigned int* __restrict__ E2) {
    for (unsigned int j = blockIdx.x * 256 + threadIdx.x; j < R2; j += gridDim.x * 256) { // ends: j grows by the grid
        const int i = amp::owner_of(roff2, n, (u64)j);                                   // a mask with runs
        const u64 jj = (u64)j - roff2[i], nb = coff[i + 1] - coff[i] - 1, b0 = coff[i] - (u64)i;
        S2[j] = bnd[b0 + 2 * jj];
        E2[j] = 2 * jj + 1 < nb ? bnd[b0 + 2 * jj + 1] : area;
    }
}

// one allocation cut into aligned pieces
struct MoArena {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

int bit_length(unsigned long long v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }      // ends: v loses a bit each time

// What a pass leaves on the device: the boundaries of every mask and where its counts start; empty: no mask has a pixel.
struct MoResult {
    amp::DevBuf mem, bnd;
    bool empty = true;
    u64* g_coff = nullptr;
    int *g_mins = nullptr, *g_maxs = nullptr;
    unsigned int* g_areas = nullptr;
    std::vector<u64> coff;                        // [n + 1], on the host
};

// One pass over the runs (g_S, g_E: R of them on the device; g_roff [n + 1]: where every mask's runs start, on the device)
int run_pass(amp_ctx* ctx, const unsigned int* g_S, const unsigned int* g_E, unsigned int R, const u64* g_roff, int n, const MoPass& g,
             int pass_index, MoResult& res) {
    hipStream_t st = ctx->stream;
    const unsigned int area = (unsigned int)((u64)g.h * (u64)g.w);
    res.empty = true;
    if (R == 0) return AMP_OK;

    // ---- the items and the events' number
    size_t tmp_a = 0, q = 0;
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, q, (u64*)nullptr, (u64*)nullptr, 0ull, (size_t)R + 1, rocprim::plus<u64>(), st));
    tmp_a = std::max(tmp_a, q);
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, q, (u64*)nullptr, (u64*)nullptr, 0ull, (size_t)MO_GRID + 1, rocprim::plus<u64>(), st));
    tmp_a = std::max(tmp_a, q);
    MoArena aa;
    const size_t o_elen = aa.add(((size_t)R + 1) * 8), o_eoff = aa.add(((size_t)R + 1) * 8), o_bsum = aa.add(((size_t)MO_GRID + 1) * 8),
                 o_boff = aa.add(((size_t)MO_GRID + 1) * 8), o_tmpa = aa.add(tmp_a);
    amp::DevBuf d_a;
    AMP_TRY_STATUS(amp::dev_alloc(d_a, aa.total));
    char* A = d_a.as<char>();
    u64 *g_elen = (u64*)(A + o_elen), *g_eoff = (u64*)(A + o_eoff), *g_bsum = (u64*)(A + o_bsum), *g_boff = (u64*)(A + o_boff);
    hipLaunchKernelGGL(mo_len_kernel, grid_256((u64)R + 1), dim3(256), 0, st, g_S, g_E, R, g.h, g.D, g_elen);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_a;
    AMP_HIP_CHECK(rocprim::exclusive_scan(A + o_tmpa, q, g_elen, g_eoff, 0ull, (size_t)R + 1, rocprim::plus<u64>(), st));
    hipLaunchKernelGGL(mo_event_kernel<false>, dim3(MO_GRID), dim3(256), 0, st, g_S, g_E, g_eoff, R, g_roff, n, g, g_bsum, (const u64*)nullptr,
                       (u64*)nullptr);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_a;
    AMP_HIP_CHECK(rocprim::exclusive_scan(A + o_tmpa, q, g_bsum, g_boff, 0ull, (size_t)MO_GRID + 1, rocprim::plus<u64>(), st));
    unsigned long long events = 0;
    AMP_HIP_CHECK(hipMemcpyAsync(&events, g_boff + MO_GRID, 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    AMP_TRY_STATUS(amp::morphology_events(events, pass_index));
    if (events == 0) return AMP_OK;                                  // an erosion that leaves nothing
    const unsigned int C = (unsigned int)events;

    // ---- the events of every mask and the boundaries among them
    const unsigned int bits = (unsigned)(MO_MASK_SHIFT + bit_length((unsigned long long)n));
    size_t tmp_b = 0;
    AMP_HIP_CHECK(rocprim::radix_sort_keys(nullptr, q, (u64*)nullptr, (u64*)nullptr, (size_t)C, 0u, bits, st));
    tmp_b = std::max(tmp_b, q);
    AMP_HIP_CHECK(rocprim::inclusive_scan(nullptr, q, (long long*)nullptr, (long long*)nullptr, (size_t)C, rocprim::plus<long long>(), st));
    tmp_b = std::max(tmp_b, q);
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, q, (unsigned int*)nullptr, (unsigned int*)nullptr, 0u, (size_t)C + 1, rocprim::plus<unsigned int>(), st));
    tmp_b = std::max(tmp_b, q);
    MoArena ab;
    const size_t o_k1 = ab.add((size_t)C * 8), o_k2 = ab.add((size_t)C * 8), o_delta = ab.add((size_t)C * 8), o_cover = ab.add((size_t)C * 8),
                 o_flags = ab.add(((size_t)C + 1) * 4), o_bidx = ab.add(((size_t)C + 1) * 4), o_ioff = ab.add(((size_t)n + 1) * 4),
                 o_coff = ab.add(((size_t)n + 1) * 8), o_mins = ab.add((size_t)n * 8), o_maxs = ab.add((size_t)n * 8), o_areas = ab.add((size_t)n * 4),
                 o_tmpb = ab.add(tmp_b);
    AMP_TRY_STATUS(amp::dev_alloc(res.mem, ab.total));
    char* B = res.mem.as<char>();
    u64 *g_k1 = (u64*)(B + o_k1), *g_k2 = (u64*)(B + o_k2);
    long long *g_delta = (long long*)(B + o_delta), *g_cover = (long long*)(B + o_cover);
    unsigned int *g_flags = (unsigned int*)(B + o_flags), *g_bidx = (unsigned int*)(B + o_bidx), *g_ioff = (unsigned int*)(B + o_ioff);
    res.g_coff = (u64*)(B + o_coff); res.g_mins = (int*)(B + o_mins); res.g_maxs = (int*)(B + o_maxs); res.g_areas = (unsigned int*)(B + o_areas);
    hipLaunchKernelGGL(mo_event_kernel<true>, dim3(MO_GRID), dim3(256), 0, st, g_S, g_E, g_eoff, R, g_roff, n, g, (u64*)nullptr, g_boff, g_k1);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::radix_sort_keys(B + o_tmpb, q, g_k1, g_k2, (size_t)C, 0u, bits, st));               // g_k2: the events by (mask, position)
    hipLaunchKernelGGL(mo_delta_kernel, grid_256(std::max<u64>(C, (u64)n + 1)), dim3(256), 0, st, g_k2, C, n, g_delta, g_ioff);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::inclusive_scan(B + o_tmpb, q, g_delta, g_cover, (size_t)C, rocprim::plus<long long>(), st));
    hipLaunchKernelGGL(mo_bound_kernel, grid_256((u64)C + 1), dim3(256), 0, st, g_k2, C, g_cover, g_ioff, g, area, g_flags);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::exclusive_scan(B + o_tmpb, q, g_flags, g_bidx, 0u, (size_t)C + 1, rocprim::plus<unsigned int>(), st));
    hipLaunchKernelGGL(count_offsets_kernel, grid_256((u64)n + 1), dim3(256), 0, st, g_bidx, g_ioff, n, res.g_coff, res.g_mins, res.g_maxs, res.g_areas);
    AMP_HIP_CHECK(hipGetLastError());
    res.coff.assign((size_t)n + 1, 0);
    AMP_HIP_CHECK(hipMemcpyAsync(res.coff.data(), res.g_coff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long total = res.coff[(size_t)n];
    if (total < (unsigned long long)n || total > (unsigned long long)n + C) {            // cannot happen: a group of events is at most one boundary
        amp::set_error("amp_mask_morphology: %llu counts from %u events of %d masks on the device", total, C, n);
        return AMP_ERR_HIP;
    }
    AMP_TRY_STATUS(amp::dev_alloc(res.bnd, (size_t)(total - (unsigned long long)n) * 4));
    hipLaunchKernelGGL(mo_place_kernel, grid_256(C), dim3(256), 0, st, g_k2, C, g_flags, g_bidx, res.bnd.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    res.empty = false;
    return AMP_OK;
}

int morphology_device(amp_ctx* ctx, const amp::MoRuns& runs, int n, int h, int w, int op, int shape, int radius, int border_value,
                      uint32_t* out_pool, unsigned long long out_cap, unsigned long long* out_off, int* out_len, long long* boxes,
                      unsigned long long* areas, unsigned long long* need) {
    const unsigned int area = (unsigned int)((u64)h * (u64)w);
    std::vector<int> hh;
    amp::mo_half_heights(shape, radius, hh);
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_S, d_E, d_roff, d_hh;
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_S, runs.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_E, runs.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_roff, runs.first));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_hh, hh));
    MoPass g;
    g.h = h; g.w = w; g.r = radius; g.rr = std::min(radius, w - 1); g.border = border_value; g.hh = d_hh.as<int>();
    g.pass = amp::mo_first_pass(op);
    g.D = 2 * g.rr + 1 + (amp::mo_is_band(g.pass) ? 1 : 0);
    MoResult first, second;
    AMP_TRY_STATUS(run_pass(ctx, d_S.as<unsigned int>(), d_E.as<unsigned int>(), (unsigned int)runs.S.size(), d_roff.as<u64>(), n, g, 1, first));
    MoResult* res = &first;
    amp::DevBuf d_S2, d_E2, d_roff2;
    if (amp::mo_second_pass(op) >= 0 && !first.empty) {
        std::vector<u64> roff2((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) roff2[(size_t)i + 1] = roff2[(size_t)i] + (first.coff[(size_t)i + 1] - first.coff[(size_t)i]) / 2;     // nb boundaries: (nb + 1) / 2 runs
        const unsigned long long R2 = roff2[(size_t)n];
        AMP_REQUIRE(R2 < (1ull << 31), "amp_mask_morphology: the first pass leaves %llu runs (at most 2^31 - 1)", R2);
        AMP_TRY_STATUS(amp::dev_upload(ctx, d_roff2, roff2));
        AMP_TRY_STATUS(amp::dev_alloc(d_S2, (size_t)R2 * 4));
        AMP_TRY_STATUS(amp::dev_alloc(d_E2, (size_t)R2 * 4));
        hipLaunchKernelGGL(mo_runs_kernel, grid_256(R2), dim3(256), 0, st, first.bnd.as<unsigned int>(), first.g_coff, d_roff2.as<u64>(), n,
                           (unsigned int)R2, area, d_S2.as<unsigned int>(), d_E2.as<unsigned int>());
        AMP_HIP_CHECK(hipGetLastError());
        g.pass = amp::mo_second_pass(op);
        AMP_TRY_STATUS(run_pass(ctx, d_S2.as<unsigned int>(), d_E2.as<unsigned int>(), (unsigned int)R2, d_roff2.as<u64>(), n, g, 2, second));
        res = &second;
    }
    if (res->empty) {                                                // every result is empty: one run of h * w zeros each
        AMP_TRY_STATUS(amp::morphology_capacity((unsigned long long)n, out_cap, need));
        for (int i = 0; i < n; ++i) {
            out_pool[i] = area; out_off[i] = (unsigned long long)i; out_len[i] = 1; areas[i] = 0;
            boxes[4 * i] = boxes[4 * i + 1] = boxes[4 * i + 2] = boxes[4 * i + 3] = 0;
        }
        return AMP_OK;
    }
    const unsigned long long total = res->coff[(size_t)n];
    AMP_TRY_STATUS(amp::morphology_capacity(total, out_cap, need));

    // ---- the counts, the boxes and the areas
    amp::DevBuf d_counts;
    AMP_TRY_STATUS(amp::dev_alloc(d_counts, (size_t)total * 4));
    hipLaunchKernelGGL(run_counts_kernel, grid_256(total), dim3(256), 0, st, res->bnd.as<unsigned int>(), res->g_coff, n, (u64)total, h, area,
                       d_counts.as<unsigned int>(), res->g_mins, res->g_maxs, res->g_areas);
    AMP_HIP_CHECK(hipGetLastError());
    std::vector<int> mins(2 * (size_t)n), maxs(2 * (size_t)n);
    std::vector<unsigned int> ar((size_t)n);
    AMP_HIP_CHECK(hipMemcpyAsync(mins.data(), res->g_mins, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(maxs.data(), res->g_maxs, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(ar.data(), res->g_areas, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    AMP_HIP_CHECK(hipMemcpyAsync(out_pool, d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < (size_t)n; ++i) {
        const bool any = ar[i] != 0;
        boxes[4 * i] = any ? mins[2 * i] : 0; boxes[4 * i + 1] = any ? mins[2 * i + 1] : 0;
        boxes[4 * i + 2] = any ? maxs[2 * i] : 0; boxes[4 * i + 3] = any ? maxs[2 * i + 1] : 0;
        areas[i] = ar[i];
        out_off[i] = res->coff[i];
        out_len[i] = (int)(res->coff[i + 1] - res->coff[i]);
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_morphology(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int op,
                                   int shape, int radius, int border_value, uint32_t* out_pool, unsigned long long out_cap,
                                   unsigned long long* out_off, int* out_len, long long* boxes, unsigned long long* areas,
                                   unsigned long long* need) {
    amp::MoRuns runs;
    AMP_TRY_STATUS(amp::morphology_check(pool, off, len, n, h, w, op, shape, radius, border_value, out_pool, out_off, out_len, boxes, areas, need, runs));
    if (n == 0) return amp::morphology_capacity(0, out_cap, need);
    return ctx ? morphology_device(ctx, runs, n, h, w, op, shape, radius, border_value, out_pool, out_cap, out_off, out_len, boxes, areas, need)
               : amp::morphology_host(runs, n, h, w, op, shape, radius, border_value, out_pool, out_cap, out_off, out_len, boxes, areas, need);
}
