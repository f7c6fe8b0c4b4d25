// amp_polygons_to_rle on the device: the polygon instances of one image (VIA ground truth: ampis/data_utils.py get_ddicts 'via2', detectron2
// PolygonMasks) as COCO run lists, boxes and areas in one call, without a dense mask or a plane per instance.  rleFrPoly restated (mask_analysis.h
// polygon_edge / polygon_crossing, the host routine's expressions in the host routine's order): a polygon is a multiset of toggle positions
// col * h + row, one per step of its 5x boundary walk that changes column; its mask is the prefix parity of the toggles, so positions of even
// multiplicity vanish and toggles at h * w change nothing; an instance is the OR of its polygons.  The launches, whatever the call holds
// (V vertices = edges, T walk steps, C crossings, n instances):
//   1. pg_edge_kernel      one lane per edge: its end points on the 5x grid, its polygon, its number of steps;
//   2. exclusive scan      of the steps (rocprim): where the steps of every edge start among the T items;
//   3. pg_cross_kernel     COUNT: a fixed grid, every workgroup a contiguous slice of the items, one lane per (edge, step): is it a crossing;
//   4. exclusive scan      of the workgroup sums.  The host reads C and sizes the arrays;
//   5. pg_cross_kernel     EMIT: the same walk with a workgroup scan (compaction.h): the key (polygon, position) of every crossing;
//   6. radix sort          of the keys (rocprim): equal keys are indistinguishable, so any order among them gives the same array;
//   7. pg_polystart_kernel one lane per polygon: where its crossings start;
//   8. pg_toggle_kernel    one lane per sorted crossing: the first of a group of equal keys survives when the group is odd and lies inside the
//                          image; it opens (+1) when an even number of the polygon's crossings precede it, else it closes (-1).  Key
//                          (instance, position, closes), every other lane a padding key behind the last instance;
//   9. radix sort          of those keys: an instance's toggles by position;
//  10. pg_delta_kernel     +1 / -1 / 0 per sorted key, and where every instance starts;
//  11. inclusive scan      of the deltas: the number of polygons that cover the pixels behind each toggle;
//  12. pg_bound_kernel     one lane per group of equal (instance, position): a boundary where the cover leaves or reaches 0 over the group;
//  13. exclusive scan      of the boundary flags;
//  14. count_offsets_kernel where every instance's counts start (its boundaries and the closing count).  The host reads the total, reports the
//                          need and refuses a capacity that is too small;
//  15. pg_place_kernel     the boundary positions, in order;
//  16. run_counts_kernel   one lane per count: boundary minus the boundary before; the runs of ones give box and area by atomic min / max / add.
// No buffer has a size fixed at compile time: one long edge or one polygon with tens of thousands of crossings is spread over lanes like any
// other, and memory is linear in vertices + crossings + counts.  Double arithmetic as on the host (-ffp-contract=off, IEEE division); the
// atomics are integer min / max / add whose order cannot show; every other word is written once by the lane that owns it.  So the bytes repeat
// and equal the host's (polygon_runs_host.hip).  Every loop in a kernel states why it ends; none waits for another lane.
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "common.h"
#include "compaction.h"
#include "mask_analysis.h"

namespace {

using amp::u64;

constexpr unsigned int PG_GRID = 2048;            // the workgroups of the walk over the items, whatever T is
constexpr int PG_POS_BITS = 31;                   // a position is at most h * w <= 2^30

struct PgEdge { int xs, ys, xe, ye, poly; };      // an edge's end points on the 5x grid as the polygon lists them, and its polygon

// the first of the n ascending keys that is >= x (n when there is none)
__device__ __forceinline__ unsigned int pg_lower_bound(const u64* __restrict__ a, unsigned int n, u64 x) {
    unsigned int lo = 0, hi = n;
    while (lo < hi) {                                                                    // ends: hi - lo halves
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// voff: the first vertex of every polygon, [P + 1] ascending, no polygon empty; elen[V] = 0 closes the array the scan reads
__global__ __launch_bounds__(256) void pg_edge_kernel(const double* __restrict__ xy, const u64* __restrict__ voff, int P, unsigned int V,
                                                      PgEdge* __restrict__ edges, u64* __restrict__ elen) {
    for (unsigned int e = blockIdx.x * 256 + threadIdx.x; e <= V; e += gridDim.x * 256) { // ends: e grows by the grid (V <= 2^30)
        if (e == V) { elen[e] = 0; continue; }
        const int p = amp::owner_of(voff, P, (u64)e);
        const u64 first = voff[p], k = voff[p + 1] - first, j = e - first, jn = j + 1 == k ? 0 : j + 1;
        PgEdge ed;
        ed.xs = amp::polygon_grid(xy[2 * (first + j)]);
        ed.ys = amp::polygon_grid(xy[2 * (first + j) + 1]);
        ed.xe = amp::polygon_grid(xy[2 * (first + jn)]);
        ed.ye = amp::polygon_grid(xy[2 * (first + jn) + 1]);
        ed.poly = p;
        edges[e] = ed;
        elen[e] = (u64)amp::polygon_edge(ed.xs, ed.ys, ed.xe, ed.ye).len;
    }
}

// Workgroup b walks items [b * slice, (b + 1) * slice) of the T = eoff[V] steps, slice a multiple of 256 that depends on T only.  COUNT: bsum[b]
// = its crossings (bsum[gridDim.x] = 0 closes the array the scan reads).  EMIT (boff = the exclusive scan of bsum): the keys, in item order.
template <bool EMIT>
__global__ __launch_bounds__(256) void pg_cross_kernel(const PgEdge* __restrict__ edges, const u64* __restrict__ eoff, unsigned int V, int h, int w,
                                                       u64* __restrict__ bsum, const u64* __restrict__ boff, u64* __restrict__ keys) {
    __shared__ unsigned int wtot[4];
    const u64 T = eoff[V], chunks = (T + 255) / 256, slice = ((chunks + gridDim.x - 1) / gridDim.x) * 256;
    const u64 first = (u64)blockIdx.x * slice, last = min(first + slice, T);
    u64 at = EMIT ? boff[blockIdx.x] : 0ull;
    for (u64 t0 = first; t0 < last; t0 += 256) {                                         // ends: t0 grows to last; uniform over the workgroup
        const u64 t = t0 + threadIdx.x;
        unsigned int pos = 0, poly = 0;
        bool hit = false;
        if (t < last) {
            const int e = amp::owner_of(eoff, (int)V, t);                                // eoff[e] <= t < eoff[e + 1]: an edge with steps
            const PgEdge ed = edges[e];
            hit = amp::polygon_crossing(amp::polygon_edge(ed.xs, ed.ys, ed.xe, ed.ye), (int)(t - eoff[e]) + 1, h, w, &pos);
            poly = (unsigned)ed.poly;
        }
        unsigned int total;
        const unsigned int before = block_before_256((unsigned)hit, wtot, &total);
        if (EMIT && hit) keys[at + before] = ((u64)poly << PG_POS_BITS) | pos;
        at += total;
    }
    if (!EMIT && threadIdx.x == 0) {
        bsum[blockIdx.x] = at;
        if (blockIdx.x == 0) bsum[gridDim.x] = 0;
    }
}

__global__ __launch_bounds__(256) void pg_polystart_kernel(const u64* __restrict__ skeys, unsigned int C, int P, unsigned int* __restrict__ pstart) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p <= P; p += gridDim.x * 256)           // ends: p grows by the grid
        pstart[p] = pg_lower_bound(skeys, C, (u64)p << PG_POS_BITS);
}

__global__ __launch_bounds__(256) void pg_toggle_kernel(const u64* __restrict__ skeys, unsigned int C, const unsigned int* __restrict__ pstart,
                                                        const int* __restrict__ pinst, int n, unsigned int area, u64* __restrict__ keys2) {
    const u64 pad = (u64)n << 32;
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < C; i += gridDim.x * 256) { // ends: i grows by the grid (C < 2^31)
        const u64 k = skeys[i];
        u64 out = pad;
        if (i == 0 || skeys[i - 1] != k) {
            const unsigned int mult = pg_lower_bound(skeys, C, k + 1) - i, pos = (unsigned int)(k & ((1ull << PG_POS_BITS) - 1));
            const unsigned int poly = (unsigned int)(k >> PG_POS_BITS);
            if ((mult & 1u) && pos < area) out = ((u64)pinst[poly] << 32) | ((u64)pos << 1) | (u64)((i - pstart[poly]) & 1u);
        }
        keys2[i] = out;
    }
}

__global__ __launch_bounds__(256) void pg_delta_kernel(const u64* __restrict__ skeys2, unsigned int C, int n, int* __restrict__ delta,
                                                       unsigned int* __restrict__ ioff) {
    const u64 pad = (u64)n << 32;
    const unsigned int items = max(C, (unsigned)n + 1u);
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < items; i += gridDim.x * 256) {   // ends: i grows by the grid
        if (i < C) delta[i] = skeys2[i] >= pad ? 0 : ((skeys2[i] & 1ull) ? -1 : 1);
        if (i <= (unsigned)n) ioff[i] = pg_lower_bound(skeys2, C, (u64)i << 32);
    }
}

// cover[i] = the sum of the deltas up to and including i; an instance's own cover is that minus the cover in front of its first toggle
__global__ __launch_bounds__(256) void pg_bound_kernel(const u64* __restrict__ skeys2, unsigned int C, int n, const int* __restrict__ cover,
                                                       const unsigned int* __restrict__ ioff, unsigned int* __restrict__ flags) {
    const u64 pad = (u64)n << 32;
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i <= C; i += gridDim.x * 256) { // ends: i grows by the grid
        unsigned int flag = 0;
        const u64 k = i < C ? skeys2[i] : pad;
        if (k < pad && (i == 0 || (skeys2[i - 1] >> 1) != (k >> 1))) {
            const unsigned int s0 = ioff[(unsigned int)(k >> 32)], tail = pg_lower_bound(skeys2, C, (k | 1ull) + 1ull) - 1u;
            const int base = s0 ? cover[s0 - 1] : 0, before = i == s0 ? 0 : cover[i - 1] - base, after = cover[tail] - base;
            flag = (before == 0) != (after == 0) ? 1u : 0u;
        }
        flags[i] = flag;                                                                 // flags[C] = 0 closes the array the scan reads
    }
}

__global__ __launch_bounds__(256) void pg_place_kernel(const u64* __restrict__ skeys2, unsigned int C, const unsigned int* __restrict__ flags,
                                                       const unsigned int* __restrict__ bidx, unsigned int* __restrict__ bnd) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < C; i += gridDim.x * 256)   // ends: i grows by the grid
        if (flags[i]) bnd[bidx[i]] = (unsigned int)((skeys2[i] >> 1) & 0x7fffffffull);
}

// one allocation cut into aligned pieces
struct PgArena {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

int bit_length(unsigned long long v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }      // ends: v loses a bit each time

int polygons_device(amp_ctx* ctx, const double* xy, const unsigned long long* poly_off, const int* inst_first, int n, int h, int w,
                    uint32_t* counts, unsigned long long counts_cap, unsigned long long* counts_off, int* counts_len, int* boxes,
                    unsigned int* areas, unsigned long long* need) {
    const unsigned int area = (unsigned int)((unsigned long long)h * (unsigned long long)w);
    const int p0 = inst_first[0], P = inst_first[n] - p0;
    const unsigned long long d0 = poly_off[p0];
    std::vector<u64> voff((size_t)P + 1);
    std::vector<int> pinst((size_t)P);
    for (int p = 0; p <= P; ++p) voff[(size_t)p] = (poly_off[p0 + p] - d0) / 2;
    for (int i = 0; i < n; ++i)
        for (int p = inst_first[i]; p < inst_first[i + 1]; ++p) pinst[(size_t)(p - p0)] = i;
    const unsigned int V = (unsigned int)voff[(size_t)P];
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // ---- the edges and the crossings' number
    size_t tmp_a = 0, q = 0;
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, q, (u64*)nullptr, (u64*)nullptr, 0ull, (size_t)V + 1, rocprim::plus<u64>(), st));
    tmp_a = std::max(tmp_a, q);
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, q, (u64*)nullptr, (u64*)nullptr, 0ull, (size_t)PG_GRID + 1, rocprim::plus<u64>(), st));
    tmp_a = std::max(tmp_a, q);
    PgArena aa;
    const size_t o_xy = aa.add((size_t)V * 16), o_voff = aa.add(((size_t)P + 1) * 8), o_pinst = aa.add((size_t)P * 4), o_edges = aa.add((size_t)V * sizeof(PgEdge)),
                 o_elen = aa.add(((size_t)V + 1) * 8), o_eoff = aa.add(((size_t)V + 1) * 8), o_bsum = aa.add(((size_t)PG_GRID + 1) * 8),
                 o_boff = aa.add(((size_t)PG_GRID + 1) * 8), o_tmpa = aa.add(tmp_a);
    amp::DevBuf d_a;
    AMP_TRY_STATUS(amp::dev_alloc(d_a, aa.total));
    char* A = d_a.as<char>();
    double* g_xy = (double*)(A + o_xy);
    u64 *g_voff = (u64*)(A + o_voff), *g_elen = (u64*)(A + o_elen), *g_eoff = (u64*)(A + o_eoff), *g_bsum = (u64*)(A + o_bsum), *g_boff = (u64*)(A + o_boff);
    int* g_pinst = (int*)(A + o_pinst);
    PgEdge* g_edges = (PgEdge*)(A + o_edges);
    AMP_HIP_CHECK(hipMemcpyAsync(g_xy, xy + d0, (size_t)V * 16, hipMemcpyHostToDevice, st));
    AMP_HIP_CHECK(hipMemcpyAsync(g_voff, voff.data(), ((size_t)P + 1) * 8, hipMemcpyHostToDevice, st));
    AMP_HIP_CHECK(hipMemcpyAsync(g_pinst, pinst.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pg_edge_kernel, grid_256((u64)V + 1), dim3(256), 0, st, g_xy, g_voff, P, V, g_edges, g_elen);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_a;
    AMP_HIP_CHECK(rocprim::exclusive_scan(A + o_tmpa, q, g_elen, g_eoff, 0ull, (size_t)V + 1, rocprim::plus<u64>(), st));
    hipLaunchKernelGGL(pg_cross_kernel<false>, dim3(PG_GRID), dim3(256), 0, st, g_edges, g_eoff, V, h, w, g_bsum, (const u64*)nullptr, (u64*)nullptr);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_a;
    AMP_HIP_CHECK(rocprim::exclusive_scan(A + o_tmpa, q, g_bsum, g_boff, 0ull, (size_t)PG_GRID + 1, rocprim::plus<u64>(), st));
    unsigned long long crossings = 0;
    AMP_HIP_CHECK(hipMemcpyAsync(&crossings, g_boff + PG_GRID, 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    AMP_REQUIRE(crossings < (1ull << 31), "amp_polygons_to_rle: the polygons cross %llu column borders (at most 2^31 - 1)", crossings);
    if (crossings == 0) {                                            // every mask is empty: one run of h * w zeros each
        AMP_TRY_STATUS(amp::polygons_capacity((unsigned long long)n, counts_cap, need));
        for (int i = 0; i < n; ++i) {
            counts[i] = area; counts_off[i] = (unsigned long long)i; counts_len[i] = 1; areas[i] = 0;
            boxes[4 * i] = boxes[4 * i + 1] = boxes[4 * i + 2] = boxes[4 * i + 3] = 0;
        }
        return AMP_OK;
    }
    const unsigned int C = (unsigned int)crossings;

    // ---- the toggles of every instance and the boundaries among them
    const unsigned int bits1 = (unsigned)(PG_POS_BITS + bit_length((unsigned long long)P)), bits2 = (unsigned)(32 + bit_length((unsigned long long)n));
    size_t tmp_b = 0;
    AMP_HIP_CHECK(rocprim::radix_sort_keys(nullptr, q, (u64*)nullptr, (u64*)nullptr, (size_t)C, 0u, bits1, st));
    tmp_b = std::max(tmp_b, q);
    AMP_HIP_CHECK(rocprim::radix_sort_keys(nullptr, q, (u64*)nullptr, (u64*)nullptr, (size_t)C, 0u, bits2, st));
    tmp_b = std::max(tmp_b, q);
    AMP_HIP_CHECK(rocprim::inclusive_scan(nullptr, q, (int*)nullptr, (int*)nullptr, (size_t)C, rocprim::plus<int>(), st));
    tmp_b = std::max(tmp_b, q);
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, q, (unsigned int*)nullptr, (unsigned int*)nullptr, 0u, (size_t)C + 1, rocprim::plus<unsigned int>(), st));
    tmp_b = std::max(tmp_b, q);
    PgArena ab;
    const size_t o_k1 = ab.add((size_t)C * 8), o_k2 = ab.add((size_t)C * 8), o_pstart = ab.add(((size_t)P + 1) * 4), o_delta = ab.add((size_t)C * 4),
                 o_cover = ab.add((size_t)C * 4), o_flags = ab.add(((size_t)C + 1) * 4), o_bidx = ab.add(((size_t)C + 1) * 4),
                 o_ioff = ab.add(((size_t)n + 1) * 4), o_coff = ab.add(((size_t)n + 1) * 8), o_mins = ab.add((size_t)n * 8), o_maxs = ab.add((size_t)n * 8),
                 o_areas = ab.add((size_t)n * 4), o_tmpb = ab.add(tmp_b);
    amp::DevBuf d_b;
    AMP_TRY_STATUS(amp::dev_alloc(d_b, ab.total));
    char* B = d_b.as<char>();
    u64 *g_k1 = (u64*)(B + o_k1), *g_k2 = (u64*)(B + o_k2), *g_coff = (u64*)(B + o_coff);
    unsigned int *g_pstart = (unsigned int*)(B + o_pstart), *g_flags = (unsigned int*)(B + o_flags), *g_bidx = (unsigned int*)(B + o_bidx),
                 *g_ioff = (unsigned int*)(B + o_ioff), *g_areas = (unsigned int*)(B + o_areas);
    int *g_delta = (int*)(B + o_delta), *g_cover = (int*)(B + o_cover), *g_mins = (int*)(B + o_mins), *g_maxs = (int*)(B + o_maxs);
    hipLaunchKernelGGL(pg_cross_kernel<true>, dim3(PG_GRID), dim3(256), 0, st, g_edges, g_eoff, V, h, w, (u64*)nullptr, g_boff, g_k1);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::radix_sort_keys(B + o_tmpb, q, g_k1, g_k2, (size_t)C, 0u, bits1, st));              // g_k2: the crossings by (polygon, position)
    hipLaunchKernelGGL(pg_polystart_kernel, grid_256((u64)P + 1), dim3(256), 0, st, g_k2, C, P, g_pstart);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pg_toggle_kernel, grid_256(C), dim3(256), 0, st, g_k2, C, g_pstart, g_pinst, n, area, g_k1);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::radix_sort_keys(B + o_tmpb, q, g_k1, g_k2, (size_t)C, 0u, bits2, st));              // g_k2: the toggles by (instance, position)
    hipLaunchKernelGGL(pg_delta_kernel, grid_256(std::max<u64>(C, (u64)n + 1)), dim3(256), 0, st, g_k2, C, n, g_delta, g_ioff);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::inclusive_scan(B + o_tmpb, q, g_delta, g_cover, (size_t)C, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(pg_bound_kernel, grid_256((u64)C + 1), dim3(256), 0, st, g_k2, C, n, g_cover, g_ioff, g_flags);
    AMP_HIP_CHECK(hipGetLastError());
    q = tmp_b;
    AMP_HIP_CHECK(rocprim::exclusive_scan(B + o_tmpb, q, g_flags, g_bidx, 0u, (size_t)C + 1, rocprim::plus<unsigned int>(), st));
    hipLaunchKernelGGL(count_offsets_kernel, grid_256((u64)n + 1), dim3(256), 0, st, g_bidx, g_ioff, n, g_coff, g_mins, g_maxs, g_areas);
    AMP_HIP_CHECK(hipGetLastError());
    std::vector<u64> coff((size_t)n + 1);
    AMP_HIP_CHECK(hipMemcpyAsync(coff.data(), g_coff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long total = coff[(size_t)n];
    if (total < (unsigned long long)n || total > (unsigned long long)n + C) {            // cannot happen: a crossing is at most one boundary
        amp::set_error("amp_polygons_to_rle: %llu counts from %u crossings of %d instances on the device", total, C, n);
        return AMP_ERR_HIP;
    }
    AMP_TRY_STATUS(amp::polygons_capacity(total, counts_cap, need));

    // ---- the counts, the boxes and the areas
    PgArena ac;
    const size_t o_bnd = ac.add((size_t)(total - n) * 4), o_counts = ac.add((size_t)total * 4);
    amp::DevBuf d_c;
    AMP_TRY_STATUS(amp::dev_alloc(d_c, ac.total));
    unsigned int *g_bnd = (unsigned int*)(d_c.as<char>() + o_bnd), *g_counts = (unsigned int*)(d_c.as<char>() + o_counts);
    hipLaunchKernelGGL(pg_place_kernel, grid_256(C), dim3(256), 0, st, g_k2, C, g_flags, g_bidx, g_bnd);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(run_counts_kernel, grid_256(total), dim3(256), 0, st, g_bnd, g_coff, n, (u64)total, h, area, g_counts, g_mins, g_maxs, g_areas);
    AMP_HIP_CHECK(hipGetLastError());
    std::vector<int> mins(2 * (size_t)n), maxs(2 * (size_t)n);
    std::vector<unsigned int> ar((size_t)n);
    AMP_HIP_CHECK(hipMemcpyAsync(mins.data(), g_mins, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(maxs.data(), g_maxs, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(ar.data(), g_areas, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    AMP_HIP_CHECK(hipMemcpyAsync(counts, g_counts, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < (size_t)n; ++i) {
        const bool any = ar[i] != 0;
        boxes[4 * i] = any ? mins[2 * i] : 0; boxes[4 * i + 1] = any ? mins[2 * i + 1] : 0;
        boxes[4 * i + 2] = any ? maxs[2 * i] : 0; boxes[4 * i + 3] = any ? maxs[2 * i + 1] : 0;
        areas[i] = ar[i];
        counts_off[i] = coff[i];
        counts_len[i] = (int)(coff[i + 1] - coff[i]);
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_polygons_to_rle(amp_ctx* ctx, const double* xy, const unsigned long long* poly_off, const int* inst_first, int n, int h, int w,
                                   uint32_t* counts, unsigned long long counts_cap, unsigned long long* counts_off, int* counts_len, int* boxes,
                                   unsigned int* areas, unsigned long long* need) {
    AMP_TRY_STATUS(amp::polygons_check(xy, poly_off, inst_first, n, h, w, counts, counts_off, counts_len, boxes, areas, need));
    if (n == 0) return amp::polygons_capacity(0, counts_cap, need);
    return ctx ? polygons_device(ctx, xy, poly_off, inst_first, n, h, w, counts, counts_cap, counts_off, counts_len, boxes, areas, need)
               : amp::polygons_host(xy, poly_off, inst_first, n, h, w, counts, counts_cap, counts_off, counts_len, boxes, areas, need);
}
