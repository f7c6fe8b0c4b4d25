// amp_mask_parts on the device: the connected components of the ones (colour 1: parts) or of the zeros inside the tight box (colour 0: holes)
// of every mask of a pool in one call, the components a rule picks flipped, the results as canonical COCO run lists -- what
// skimage.morphology.remove_small_objects / remove_small_holes, scipy.ndimage.binary_fill_holes and regionprops' euler_number / filled_area
// do on one decoded full-image array per mask.  The masks stay run lists: the host cuts the plan into the ITEMS of mask_parts.h (vertical
// pieces of one column, all masks in one array, every size known before the first launch).  The launches, whatever the number of masks:
//   1. mp_init_kernel     parent[i] = i, the per-root sums cleared;
//   2. mp_union_kernel    one lane per COMPONENT item, against the COMPONENT items of the column before it in the SAME mask whose rows meet
//                         its own (one row wider on each side where diagonal neighbours count): lock-free union-find, the larger root hooked
//                         under the smaller by compare-and-swap (union_find.h, shared with label_runs.hip);
//   3. mp_flatten_kernel  every item's root; per root the area (atomic add) and, colour 0, whether a piece touches the border of the tight
//                         box (atomic or): such a set is the outside, not a hole;
//   4. mp_roots_kernel    one lane per root that counts: per mask the components, their pixels (atomic adds, one per wave where the wave
//                         holds one mask) and the best one as (area, ~root) in one word (atomic max: the largest area, then the smallest
//                         root, which is the set's first item and so the tie rule of the definition);
//   5. mp_count_kernel    one lane per item: is its component flipped, its value in the result and those of its neighbours, the boundaries
//                         it writes (none where it meets a neighbour of the same value); the flipped pixels per mask; a workgroup sum each;
//   6. scan_sums_kernel   one workgroup: the exclusive scan of the sums.  The host reads the total, reports the need and refuses a capacity
//                         that is too small;
//   7. mp_emit_kernel     as 5 with a workgroup scan: the boundary positions and where every mask's list starts;
//   8. diff_counts_kernel one lane per count: boundary minus the boundary before it (0 in front of a mask's first).
// The workgroup sums and scans, 6 and 8 are compaction.h's; the items reach the device through MpItemsDev (mask_parts_dev.h).
// A stats-only call (out_pool NULL) ends after 5.  Integer arithmetic only.  The atomics are integer add / or / max and the compare-and-swap
// on the parents: the partition into sets does not depend on the order of the unions, nothing is placed through a counter.  So the bytes
// repeat and equal the host's (mask_parts_host.hip).  Every loop in a kernel states why it ends; none waits for another lane.
#include <vector>

#include "common.h"
#include "compaction.h"
#include "mask_parts.h"
#include "mask_parts_dev.h"
#include "union_find.h"

namespace {

using amp::MpMask;
using amp::u64;
using amp::wave_sum;

struct MpArgs : amp::MpItemsView {
    int h, colour, keep_largest;
    unsigned int threshold;
};

__global__ __launch_bounds__(256) void mp_init_kernel(unsigned int R, unsigned int* __restrict__ parent, unsigned int* __restrict__ area,
                                                      unsigned int* __restrict__ touch) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < R; i += gridDim.x * 256) { // ends: i grows by the grid (R < 2^31, the grid < 2^25 lanes)
        parent[i] = i; area[i] = 0u; touch[i] = 0u;
    }
}

__global__ __launch_bounds__(256) void mp_union_kernel(MpArgs g, int d, unsigned int* parent) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < g.R; i += gridDim.x * 256) {       // ends: i grows by the grid
        if (g.T[i] != amp::MP_COMPONENT) continue;
        const MpMask mk = g.masks[amp::owner_of(g.first, g.n, (u64)i)];                  // every mask has an item: no empty range
        const int q = (int)(g.S[i] / (unsigned)g.h) - mk.c0;
        if (q == 0) continue;
        const int s = (int)g.S[i], e = (int)g.E[i], shift = g.h;                         // a piece of column q - 1 moved one column right
        int lo = (int)g.col[mk.col0 + q - 1], hi = (int)g.col[mk.col0 + q];
        const int jend = hi;
        while (lo < hi) {                                                                // ends: hi - lo halves; the first piece that ends below s - d
            const int mid = (lo + hi) >> 1;
            if ((int)g.E[mid] + shift + d <= s) lo = mid + 1; else hi = mid;
        }
        for (int j = lo; j < jend && (int)g.S[j] + shift < e + d; ++j)                   // ends: j grows to jend
            if (g.T[j] == amp::MP_COMPONENT) amp::uf_unite(parent, i, (unsigned)j);
    }
}

__global__ __launch_bounds__(256) void mp_flatten_kernel(MpArgs g, unsigned int* parent, unsigned int* __restrict__ root_of,
                                                         unsigned int* __restrict__ area, unsigned int* __restrict__ touch) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < g.R; i += gridDim.x * 256) {       // ends: i grows by the grid
        if (g.T[i] != amp::MP_COMPONENT) { root_of[i] = i; continue; }
        const unsigned int root = amp::uf_find<false>(parent, i);                        // no parent is written in this launch
        root_of[i] = root;
        atomicAdd(&area[root], g.E[i] - g.S[i]);
        if (g.colour == 0 && amp::mp_touches(g.masks[amp::owner_of(g.first, g.n, (u64)i)], g.h, g.S[i], g.E[i])) atomicOr(&touch[root], 1u);
    }
}

// stats [n][4]: {components, their pixels, -, flipped pixels}; best [n]: mp_best_key of the best component
__global__ __launch_bounds__(256) void mp_roots_kernel(MpArgs g, const unsigned int* __restrict__ root_of, const unsigned int* __restrict__ area,
                                                       const unsigned int* __restrict__ touch, unsigned long long* __restrict__ stats,
                                                       unsigned long long* __restrict__ best) {
    const unsigned int rounds = (g.R + gridDim.x * 256 - 1) / (gridDim.x * 256);
    for (unsigned int it = 0; it < rounds; ++it) {                                       // every lane of a wave makes every round: the wave votes below
        const unsigned int i = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        int m = -1;
        u64 cnt = 0, px = 0;
        if (i < g.R) {
            m = amp::owner_of(g.first, g.n, (u64)i);
            if (g.T[i] == amp::MP_COMPONENT && root_of[i] == i && !touch[i]) {
                cnt = 1; px = area[i];
                atomicMax(&best[m], amp::mp_best_key(area[i], i));
            }
        }
        const int m0 = __shfl(m, 0, 64);
        if (__all(m == m0)) {                                                            // one mask in the wave (or none): one add per sum
            const u64 c = wave_sum(cnt), p = wave_sum(px);
            if ((threadIdx.x & 63) == 0 && c && m0 >= 0) { atomicAdd(&stats[4 * (size_t)m0], c); atomicAdd(&stats[4 * (size_t)m0 + 1], p); }
        } else if (cnt) {
            atomicAdd(&stats[4 * (size_t)m], cnt); atomicAdd(&stats[4 * (size_t)m + 1], px);
        }
    }
}

struct MpRoots {
    const unsigned int *root_of, *area, *touch;
    const unsigned long long* best;
};

// is item j's component flipped?  false for an item that belongs to none
__device__ __forceinline__ bool mp_item_flip(const MpArgs& g, const MpRoots& r, unsigned int j, int m) {
    if (g.T[j] != amp::MP_COMPONENT) return false;
    const unsigned int root = r.root_of[j];
    return amp::mp_flip(g.colour, !r.touch[root], r.area[root], root, r.best[m], g.threshold, g.keep_largest);
}

// the boundaries item j writes; *m = its mask, *flip = whether its component is flipped.  Items j - 1 and j + 1 are read only inside the mask.
__device__ __forceinline__ amp::MpBounds mp_item_bounds(const MpArgs& g, const MpRoots& r, unsigned int j, int* m, bool* flip) {
    *m = amp::owner_of(g.first, g.n, (u64)j);
    const int kind = g.T[j];
    *flip = mp_item_flip(g, r, j, *m);
    const bool has_prev = (u64)j > g.first[*m], has_next = kind != amp::MP_END;          // the END item is the mask's last
    const int v_prev = has_prev ? amp::mp_value(g.T[j - 1], g.colour, mp_item_flip(g, r, j - 1, *m)) : 0;
    const int v_next = has_next ? amp::mp_value(g.T[j + 1], g.colour, mp_item_flip(g, r, j + 1, *m)) : 0;
    return amp::mp_bounds(kind, amp::mp_value(kind, g.colour, *flip), g.S[j], g.E[j], has_prev, v_prev, has_prev ? g.E[j - 1] : 0u, v_next,
                          has_next ? g.S[j + 1] : 0u);
}

// workgroup b owns items [256 b, 256 b + 256): sums[b] = the boundaries they write
__global__ __launch_bounds__(256) void mp_count_kernel(MpArgs g, MpRoots r, unsigned int nblk, unsigned long long* __restrict__ sums,
                                                       unsigned long long* __restrict__ stats) {
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const unsigned int j = blk * 256 + threadIdx.x;
        unsigned int nb = 0;
        if (j < g.R) {
            int m;
            bool flip;
            const amp::MpBounds b = mp_item_bounds(g, r, j, &m, &flip);
            nb = (unsigned)b.s + (unsigned)b.e;
            if (flip && r.root_of[j] == j) atomicAdd(&stats[4 * (size_t)m + 3], (unsigned long long)r.area[j]);
        }
        block_sums_256<1>(1, nblk, blk, sums, [&](int) { return nb; });
    }
}

__global__ __launch_bounds__(256) void mp_emit_kernel(MpArgs g, MpRoots r, unsigned int nblk, const unsigned long long* __restrict__ sums,
                                                      unsigned long long* __restrict__ off, unsigned int* __restrict__ bnd) {
    __shared__ unsigned int wtot[4];
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const unsigned int j = blk * 256 + threadIdx.x;
        int m = 0;
        bool flip;
        amp::MpBounds b{false, false};
        if (j < g.R) b = mp_item_bounds(g, r, j, &m, &flip);
        unsigned long long at = sums[blk] + block_before_256((unsigned)b.s + (unsigned)b.e, wtot);
        if (j >= g.R) continue;                                                          // after the barriers
        if ((u64)j == g.first[m]) off[m] = at;
        if (b.s) bnd[at++] = g.S[j];
        if (b.e) bnd[at++] = g.E[j];
    }
}

int mask_parts_device(amp_ctx* ctx, const amp::MpItems& it, int h, int colour, int connectivity, unsigned int threshold, int keep_largest,
                      unsigned long long* stats, uint32_t* out_pool, unsigned long long out_cap, unsigned long long* out_off, int* out_len,
                      unsigned long long* need) {
    const int n = (int)it.m.size();
    const unsigned int R = (unsigned int)it.S.size(), nblk = (R + 255) / 256;
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    amp::MpItemsDev d_items;
    amp::DevBuf d_parent, d_root, d_area, d_touch, d_stats, d_best, d_sums, d_total;
    AMP_TRY_STATUS(d_items.upload(ctx, it));
    AMP_TRY_STATUS(amp::dev_alloc(d_parent, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_root, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_area, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_touch, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_stats, (size_t)n * 32));
    AMP_TRY_STATUS(amp::dev_alloc(d_best, (size_t)n * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_sums, (size_t)nblk * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_total, 2 * 8));
    AMP_HIP_CHECK(hipMemsetAsync(d_stats.p, 0, (size_t)n * 32, st));
    AMP_HIP_CHECK(hipMemsetAsync(d_best.p, 0, (size_t)n * 8, st));
    const MpArgs g{d_items.view(), h, colour, keep_largest, threshold};
    const MpRoots r{d_root.as<unsigned int>(), d_area.as<unsigned int>(), d_touch.as<unsigned int>(), d_best.as<unsigned long long>()};
    unsigned int* parent = d_parent.as<unsigned int>();
    unsigned long long *dstats = d_stats.as<unsigned long long>(), *sums = d_sums.as<unsigned long long>();
    hipLaunchKernelGGL(mp_init_kernel, grid_256(R), dim3(256), 0, st, R, parent, d_area.as<unsigned int>(), d_touch.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mp_union_kernel, grid_256(R), dim3(256), 0, st, g, amp::mp_reach(colour, connectivity), parent);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mp_flatten_kernel, grid_256(R), dim3(256), 0, st, g, parent, d_root.as<unsigned int>(), d_area.as<unsigned int>(),
                       d_touch.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mp_roots_kernel, grid_256(R), dim3(256), 0, st, g, r.root_of, r.area, r.touch, dstats, d_best.as<unsigned long long>());
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mp_count_kernel, grid_256(R), dim3(256), 0, st, g, r, nblk, sums, dstats);
    AMP_HIP_CHECK(hipGetLastError());

    std::vector<unsigned long long> hstats(4 * (size_t)n), hbest((size_t)n);
    auto finish_stats = [&]() {
        for (size_t p = 0; p < (size_t)n; ++p) hstats[4 * p + 2] = hbest[p] >> 32;
        std::copy(hstats.begin(), hstats.end(), stats);
    };
    AMP_HIP_CHECK(hipMemcpyAsync(hstats.data(), dstats, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(hbest.data(), d_best.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (!out_pool) {
        AMP_HIP_CHECK(hipStreamSynchronize(st));
        finish_stats();
        return AMP_OK;
    }
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, sums, nblk, 1, d_total.as<unsigned long long>());      // {0, the total}
    AMP_HIP_CHECK(hipGetLastError());
    unsigned long long total = 0;
    AMP_HIP_CHECK(hipMemcpyAsync(&total, d_total.as<unsigned long long>() + 1, 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    if (total < (unsigned long long)n || total > 2ull * R) {         // cannot happen: a mask has a count, an item writes at most two boundaries
        amp::set_error("amp_mask_parts: %llu counts from %u items of %d masks on the device", total, R, n);
        return AMP_ERR_HIP;
    }
    AMP_TRY_STATUS(amp::mask_parts_capacity(total, out_cap, need));

    amp::DevBuf d_off, d_bnd, d_counts;
    AMP_TRY_STATUS(amp::dev_alloc(d_off, (size_t)n * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_bnd, (size_t)total * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_counts, (size_t)total * 4));
    hipLaunchKernelGGL(mp_emit_kernel, grid_256(R), dim3(256), 0, st, g, r, nblk, sums, d_off.as<unsigned long long>(), d_bnd.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(diff_counts_kernel, grid_256(total), dim3(256), 0, st, d_bnd.as<unsigned int>(), d_off.as<unsigned long long>(), n, total,
                       d_counts.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> hoff((size_t)n);
    AMP_HIP_CHECK(hipMemcpyAsync(hoff.data(), d_off.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    AMP_HIP_CHECK(hipMemcpyAsync(out_pool, d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    finish_stats();
    for (size_t p = 0; p < (size_t)n; ++p) {
        out_off[p] = hoff[p];
        out_len[p] = (int)((p + 1 < (size_t)n ? hoff[p + 1] : total) - hoff[p]);
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_parts(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int colour,
                              int connectivity, unsigned int threshold, int keep_largest, unsigned long long* stats, uint32_t* out_pool,
                              unsigned long long out_cap, unsigned long long* out_off, int* out_len, unsigned long long* need) {
    amp::RunPlan plan;
    AMP_TRY_STATUS(amp::mask_parts_check(pool, off, len, n, h, w, colour, connectivity, keep_largest, stats, out_pool, out_off, out_len, need, plan));
    if (n == 0) {
        if (out_pool) need[0] = 0;
        return AMP_OK;
    }
    amp::MpItems items;
    AMP_REQUIRE(amp::mp_build_items(plan, h, w, colour, items), "amp_mask_parts: the masks of one call have more than 2^31 pieces");
    return ctx ? mask_parts_device(ctx, items, h, colour, connectivity, threshold, keep_largest, stats, out_pool, out_cap, out_off, out_len, need)
               : amp::mask_parts_host(items, h, colour, connectivity, threshold, keep_largest, stats, out_pool, out_cap, out_off, out_len, need);
}
