// Region properties on the device (ampis/structures.py:474-514, InstanceSet.compute_rprops: skimage.measure.regionprops on one full-image label
// array per mask).  Per mask 13 exact integers {N, sum r, sum c, sum r^2, sum r c, sum c^2, P1, P2, P3, convex area, 0, 0, 0}; every float of
// the table is derived from them on the host (ampis_amd/analyze.py).  The masks stay run lists until they are bit planes of their tight boxes:
//   1. rp_moments_kernel   one lane per run of ones: the run's six sums in closed form (first partial column, the full columns between, last
//                          partial column: O(1) whatever the run's length), a wave and a workgroup reduction, one 64-bit integer atomic per sum
//                          and tile;
//   2. rp_decode_kernel    decodes every run list into a COLUMN-major bit plane of the mask's tight box, 64 rows a word, like ed_decode_kernel of
//                          edge_distance.hip.  The box is tight, so everything around the plane is 0 and no halo is stored: a neighbour outside
//                          the plane reads as 0 (rp_word);
//   3. rp_words_kernel<0>  one lane per word: border = m & ~(up & down & left & right), the carries across the 64-row boundary from the words
//                          above and below;
//   4. rp_words_kernel<1>  one lane per word: the 3 x 3 border words around it, the eight shifted neighbour boards, bit-sliced counts of the 4-
//                          and the diagonal neighbours, three predicate boards, three popcounts; a wave whose words all belong to one mask adds
//                          once per class, a wave across masks per lane;
//   5. rp_hull_kernel      one wave per mask.  Lanes: the extreme hull candidates at every half-pixel X (first / last set bit of the columns by
//                          ctz / clz).  Lane 0 / lane 1: the lower / upper monotone chain in half-pixel integers, stacks in global scratch.
//                          Lanes again: one chain edge each, the bound on the centre rows it sets in every column it spans (integer floor / ceil
//                          division), summed by the wave.  The chain is sequential: 2 W + 1 points, each pushed and popped at most once, a few
//                          dependent cached loads per step.  Worst case, a mask as wide as w = 32768: 65537 points per chain, ~2.6e5 stack steps
//                          in one wave; the whole call on the 32768 x 32768 full image took 0.09 s in the GPU test.
// Five launches and two memsets per call whatever the number of masks.  Integer arithmetic only; the only atomics are 64-bit integer adds and
// ORs, whose results do not depend on the order, so the bytes repeat.  The word arithmetic is region_props.h, shared with the host evaluation
// (mask_analysis_host.hip); the runs and the tight boxes come from the plan the argument checks build, the painter is run_list.h's.  Scratch:
// two planes per tight box and 4 (2 W + 1) ints per mask.
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "region_props.h"

namespace {

using amp::RpMask;
using amp::u64;
using amp::wave_sum;

// tile = {mask, first run of ones}: thread t takes run first + t.  runs[k] = pixels [x, y) of the column-major image
__global__ __launch_bounds__(256) void rp_moments_kernel(const RpMask* __restrict__ masks, const int2* __restrict__ tiles, int ntiles,
                                                         const uint2* __restrict__ runs, unsigned long long* __restrict__ vals, int h) {
    __shared__ u64 part[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {           // uniform over the workgroup: every thread meets every barrier
        const int2 tl = tiles[t];
        const RpMask mk = masks[tl.x];
        const int k = tl.y + (int)threadIdx.x;
        u64 acc[6] = {0, 0, 0, 0, 0, 0};
        if (k < mk.n) {
            const uint2 r = runs[mk.run0 + k];
            amp::rp_run_sums(r.x, r.y, (u64)h, acc);
        }
        for (int k = 0; k < 6; ++k) {
            const u64 s = wave_sum(acc[k]);
            if (lane == 0) part[wave][k] = s;
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            const u64 s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
            if (s) atomicAdd(&vals[13 * (size_t)tl.x + threadIdx.x], s);
        }
        __syncthreads();
    }
}

// same tiles.  Every run of a mask lies inside the mask's tight box, so no clipping is needed
__global__ __launch_bounds__(256) void rp_decode_kernel(const RpMask* __restrict__ masks, const int2* __restrict__ tiles, int ntiles,
                                                        const uint2* __restrict__ runs, unsigned long long* __restrict__ planes, int h) {
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int2 tl = tiles[t];
        const RpMask mk = masks[tl.x];
        const int k = tl.y + (int)threadIdx.x;
        if (k >= mk.n) continue;
        const uint2 r = runs[mk.run0 + k];
        amp::paint_run<false>(r.x, r.y, h, planes + mk.plane, mk.r0, mk.c0, mk.H, mk.W, mk.pitch, amp::OrAtomic());
    }
}

// CLASSIFY = false: writes the border plane behind the mask plane.  true: reads it and adds the three class counts to vals[mask][6 .. 8]
template <bool CLASSIFY>
__global__ __launch_bounds__(256) void rp_words_kernel(const RpMask* __restrict__ masks, int n, const unsigned long long* __restrict__ uoff,
                                                       unsigned long long total, unsigned long long* __restrict__ planes,
                                                       unsigned long long* __restrict__ vals) {
    const unsigned long long rounds = (total + (unsigned long long)gridDim.x * 256 - 1) / ((unsigned long long)gridDim.x * 256);
    for (unsigned long long it = 0; it < rounds; ++it) {             // every lane of a wave makes every round: the wave votes below
        const unsigned long long u = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        int m = -1;
        u64 cls[3] = {0, 0, 0};
        if (u < total) {
            m = amp::owner_of(uoff, n, u);           // masks without a plane have an empty range and are never found
            const RpMask mk = masks[m];
            const unsigned long long local = u - uoff[m], units = (unsigned long long)mk.W * mk.pitch;
            const int q = (int)(local / (unsigned)mk.pitch), wv = (int)(local % (unsigned)mk.pitch);
            if (!CLASSIFY) {
                planes[mk.plane + units + local] = amp::rp_border_at(planes + mk.plane, mk.W, mk.pitch, q, wv);
            } else if (planes[mk.plane + units + local]) {
                amp::rp_classify_at(planes + mk.plane + units, mk.W, mk.pitch, q, wv, cls);
            }
        }
        if (CLASSIFY) {
            const int cnt[3] = {amp::popc(cls[0]), amp::popc(cls[1]), amp::popc(cls[2])};
            const int m0 = __shfl(m, 0, 64);
            if (__all(m == m0)) {                                    // one mask in the wave (or none): one add per class
                for (int k = 0; k < 3; ++k) {
                    const u64 s = wave_sum((u64)cnt[k]);
                    if ((threadIdx.x & 63) == 0 && s && m0 >= 0) atomicAdd(&vals[13 * (size_t)m0 + 6 + k], s);
                }
            } else if (m >= 0) {
                for (int k = 0; k < 3; ++k)
                    if (cnt[k]) atomicAdd(&vals[13 * (size_t)m + 6 + k], (u64)cnt[k]);
            }
        }
    }
}

// one wave per mask; hull: the scratch of RpMask::hull
__global__ __launch_bounds__(64) void rp_hull_kernel(const RpMask* __restrict__ masks, int n, const unsigned long long* __restrict__ planes,
                                                     int* __restrict__ hull, unsigned long long* __restrict__ vals) {
    __shared__ int klen[2];
    const int lane = threadIdx.x;
    for (int m = blockIdx.x; m < n; m += gridDim.x) {
        const RpMask mk = masks[m];
        if (mk.W == 0) continue;                                     // uniform over the wave
        const int np = 2 * mk.W + 1;
        int* lo = hull + mk.hull;
        int *hi = lo + np, *sl = hi + np, *su = sl + np;
        for (int i = lane; i < np; i += 64) amp::rp_point(i, mk.W, planes + mk.plane, mk.pitch, &lo[i], &hi[i]);
        __syncthreads();
        if (lane == 0) klen[0] = amp::rp_chain(lo, np, +1, sl);
        if (lane == 1) klen[1] = amp::rp_chain(hi, np, -1, su);
        __syncthreads();
        const int kl = klen[0], ku = klen[1];
        long long s = 0;
        for (int k = lane; k + 1 < ku; k += 64) s += amp::rp_edge_sum(su[k], hi[su[k]], su[k + 1], hi[su[k + 1]], true);
        for (int k = lane; k + 1 < kl; k += 64) s -= amp::rp_edge_sum(sl[k], lo[sl[k]], sl[k + 1], lo[sl[k + 1]], false);
        const u64 tot = wave_sum((u64)s);                   // two's complement: the wrapped partial sums add up to the true total
        if (lane == 0) vals[13 * (size_t)m + 9] = tot + (u64)mk.W;
        __syncthreads();                                             // klen is rewritten for the next mask
    }
}

static int region_props_device(amp_ctx* ctx, const amp::RunPlan& plan, int h, unsigned long long* vals) {
    // mask records, the runs of ones, (mask, 256 runs) tiles, plane and hull scratch offsets
    const int n = (int)plan.m.size();
    std::vector<uint2> runs;
    std::vector<RpMask> masks((size_t)n);
    std::vector<int2> tiles;
    std::vector<unsigned long long> uoff((size_t)n + 1, 0);
    unsigned long long units = 0, hints = 0;
    // a lane decodes its run word by word: a run of more than ~4096 plane words (many whole columns of a large mask) is cut into pieces of
    // that size, so the full image is a few hundred lanes' work and not one lane's
    const unsigned int piece = (unsigned)h * (unsigned)std::max(1, 4096 / ((h + 63) >> 6));
    for (int p = 0; p < n; ++p) {
        const amp::RunMask& mk = plan.m[(size_t)p];
        RpMask& e = masks[(size_t)p];
        e.H = mk.r1 - mk.r0; e.W = mk.c1 - mk.c0; e.r0 = mk.r0; e.c0 = mk.c0;
        e.pitch = (e.H + 63) >> 6;
        e.plane = 2 * units; e.run0 = runs.size(); e.hull = hints;
        uoff[(size_t)p] = units;
        for (int k = 0; k < mk.n; ++k) {
            unsigned int s = plan.S[mk.ro + k];
            const unsigned int t = plan.E[mk.ro + k];
            for (; t - s > piece; s += piece) runs.push_back(make_uint2(s, s + piece));
            runs.push_back(make_uint2(s, t));
        }
        e.n = (int)(runs.size() - e.run0);                           // 0 for an empty mask: no pixel, no tile and no plane, its 13 integers stay 0
        units += (unsigned long long)e.W * e.pitch;
        hints += e.n ? 4ull * (2ull * e.W + 1) : 0ull;
        for (int k = 0; k < e.n; k += 256) tiles.push_back(make_int2(p, k));
        AMP_REQUIRE(tiles.size() < (1u << 30) && runs.size() < (1ull << 31), "amp_mask_region_props: the masks of one call have more than 2^31 runs");
    }
    uoff[(size_t)n] = units;
    const int nt = (int)tiles.size();

    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_masks, d_tiles, d_runs, d_uoff, d_planes, d_hull, d_vals;
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_masks, masks));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_tiles, tiles));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_runs, runs));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_uoff, uoff));
    AMP_TRY_STATUS(amp::dev_alloc(d_planes, (size_t)units * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_hull, (size_t)hints * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_vals, (size_t)n * 13 * 8));
    unsigned long long* dv = d_vals.as<unsigned long long>();
    unsigned long long* planes = d_planes.as<unsigned long long>();
    AMP_HIP_CHECK(hipMemsetAsync(dv, 0, (size_t)n * 13 * 8, st));
    if (units) AMP_HIP_CHECK(hipMemsetAsync(planes, 0, (size_t)units * 16, st));
    if (nt) {
        const dim3 grid((unsigned)std::min(nt, 1 << 20));
        hipLaunchKernelGGL(rp_moments_kernel, grid, dim3(256), 0, st, d_masks.as<RpMask>(), d_tiles.as<int2>(), nt, d_runs.as<uint2>(), dv, h);
        AMP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(rp_decode_kernel, grid, dim3(256), 0, st, d_masks.as<RpMask>(), d_tiles.as<int2>(), nt, d_runs.as<uint2>(), planes, h);
        AMP_HIP_CHECK(hipGetLastError());
        const dim3 wgrid((unsigned)std::min<unsigned long long>((units + 255) / 256, 1ull << 20));
        hipLaunchKernelGGL(rp_words_kernel<false>, wgrid, dim3(256), 0, st, d_masks.as<RpMask>(), n, d_uoff.as<unsigned long long>(), units, planes, dv);
        AMP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(rp_words_kernel<true>, wgrid, dim3(256), 0, st, d_masks.as<RpMask>(), n, d_uoff.as<unsigned long long>(), units, planes, dv);
        AMP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(rp_hull_kernel, dim3((unsigned)std::min(n, 1 << 20)), dim3(64), 0, st, d_masks.as<RpMask>(), n, planes, d_hull.as<int>(), dv);
        AMP_HIP_CHECK(hipGetLastError());
    }
    AMP_HIP_CHECK(hipMemcpyAsync(vals, dv, (size_t)n * 13 * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_region_props(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                                     long long* bbox, unsigned long long* vals) {
    amp::RunPlan plan;
    AMP_TRY_STATUS(amp::region_props_check(pool, off, len, n, h, w, bbox, vals, plan));
    if (n == 0) return AMP_OK;
    AMP_TRY_STATUS(ctx ? region_props_device(ctx, plan, h, vals) : amp::region_props_host(plan, h, vals));
    for (int p = 0; p < n; ++p) {
        const amp::RunMask& mk = plan.m[(size_t)p];
        long long* b = bbox + 4 * (size_t)p;
        b[0] = mk.r0; b[1] = mk.c0; b[2] = mk.r1; b[3] = mk.c1;
    }
    return AMP_OK;
}
