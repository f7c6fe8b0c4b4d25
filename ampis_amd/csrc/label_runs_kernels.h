// The run stages of a label image on the device, shared by label_runs.hip (amp_label_runs: the instances of an annotation image) and
// flatten.hip (amp_flatten_instances: the visible lists are the per-id runs of the owner map), moved out of label_runs.hip unchanged the way
// union_find.h was.  The image is cut into VERTICAL runs -- foreground runs of a BINARY image, constant-id runs of a LABEL image, never
// across a column end --, which in column-major order are the pieces of every instance's COCO run list; positions are those of the
// column-major image, col * h + row.
//   lr_planes_kernel   one lane per (64 rows, column), columns fastest so a wave reads rows of the row-major image: two column-major bit
//                      planes (64 rows a word), START = the pixel opens a run, END = it closes one;
//   lr_count_kernel    one lane per plane word in column-major order: the set bits of both planes, a workgroup sum each;
//   scan_sums_kernel   one workgroup: the exclusive scan of the sums (compaction.h, as the workgroup sums and scans of the kernels here);
//   lr_write_kernel    as lr_count_kernel with a workgroup scan: run k's start S[k], end E[k], id V[k] (LABEL), parent[k] = k, and the first
//                      run of every column;
//   lr_keys_kernel     the sort key of every run -- its root's smallest position, or the id with the sign bit flipped -- and the run's index
//                      as the value, for a stable radix sort;
//   lr_heads_kernel    one lane per sorted run: does it open an instance, how many boundaries it writes (none where it is joined with its
//                      neighbour across a column end; the closing h * w after an instance's last run), a workgroup sum each;
//   lr_emit_kernel     as lr_heads_kernel with a workgroup scan: boundary positions, id and offset of every instance, box and area by atomic
//                      min / max / add.
// The host drives them in three steps over one LrStages, which both entry points call in this order: lr_cut (planes, count, scan, the
// number of runs read back, write), lr_group (keys, the stable radix sort, heads, scan, the instances and counts read back) and lr_emit.
// Between them an entry point does what is its own: amp_label_runs unites the runs of a BINARY image, each judges the numbers read back
// by its own bound and reports its own capacity.
// Integer arithmetic only; nothing is placed through a counter, so the bytes repeat.  Every loop states why it ends; none waits for
// another lane.  For hipcc only; every file that includes this header gets kernels of its own.
#pragma once
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "compaction.h"
#include "mask_analysis.h"

namespace {

using amp::u64;

__global__ __launch_bounds__(256) void lr_planes_kernel(const void* __restrict__ img, int h, int w, int kind, int zero_bg, int pitch,
                                                        unsigned long long units, unsigned long long* __restrict__ planes) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < units; t += (unsigned long long)gridDim.x * 256) {   // ends: t grows by the grid
        const int c = (int)(t % (unsigned)w), wv = (int)(t / (unsigned)w), ra = wv << 6, n = min(64, h - ra);
        int prev = ra > 0 ? amp::label_pixel(img, kind, (size_t)(ra - 1) * w + c) : 0;
        bool has_prev = ra > 0;
        int cur = amp::label_pixel(img, kind, (size_t)ra * w + c);
        u64 start = 0, end = 0;
        for (int b = 0; b < n; ++b) {                                                    // ends: at most 64 rows
            const bool has_next = ra + b + 1 < h;
            const int next = has_next ? amp::label_pixel(img, kind, (size_t)(ra + b + 1) * w + c) : 0;
            if (amp::label_is_instance(cur, kind, zero_bg)) {
                if (!has_prev || prev != cur) start |= 1ull << b;
                if (!has_next || next != cur) end |= 1ull << b;
            }
            prev = cur; has_prev = true; cur = next;
        }
        planes[(size_t)c * pitch + wv] = start;
        planes[units + (size_t)c * pitch + wv] = end;
    }
}

// workgroup b owns plane words [256 b, 256 b + 256) in column-major order; sums[k * nblk + b] = the set bits of plane k in them
__global__ __launch_bounds__(256) void lr_count_kernel(const unsigned long long* __restrict__ planes, unsigned long long units, unsigned int nblk,
                                                       unsigned long long* __restrict__ sums) {
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const unsigned long long u = (unsigned long long)blk * 256 + threadIdx.x;
        block_sums_256<2>(2, nblk, blk, sums, [&](int k) { return u < units ? amp::popc(planes[k * units + u]) : 0; });
    }
}

__global__ __launch_bounds__(256) void lr_write_kernel(const unsigned long long* __restrict__ planes, unsigned long long units, int h, int w,
                                                       int pitch, unsigned int nblk, const unsigned long long* __restrict__ sums,
                                                       const unsigned long long* __restrict__ base, const void* __restrict__ img, int kind,
                                                       unsigned int* __restrict__ S, unsigned int* __restrict__ E, int* __restrict__ V,
                                                       unsigned int* __restrict__ parent, unsigned int* __restrict__ colstart) {
    __shared__ unsigned int wtot[4];
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const unsigned long long u = (unsigned long long)blk * 256 + threadIdx.x;
        const bool in = u < units;
        const int c = in ? (int)(u / (unsigned)pitch) : 0, wv = in ? (int)(u % (unsigned)pitch) : 0;
        const unsigned int pos = (unsigned)c * (unsigned)h + ((unsigned)wv << 6);
        const u64 start = in ? planes[u] : 0ull, end = in ? planes[units + u] : 0ull;
        unsigned int at = (unsigned int)(sums[blk] - base[0]) + block_before_256((unsigned)amp::popc(start), wtot);
        if (in && wv == 0) colstart[c] = at;
        for (u64 x = start; x; x &= x - 1) {                                             // ends: one set bit fewer each time
            const int b = amp::ctz(x);
            S[at] = pos + (unsigned)b;
            parent[at] = at;
            if (kind != 0) V[at] = amp::label_pixel(img, kind, (size_t)((wv << 6) + b) * w + c);
            ++at;
        }
        if (in && u == units - 1) colstart[w] = at;
        at = (unsigned int)(sums[(size_t)nblk + blk] - base[1]) + block_before_256((unsigned)amp::popc(end), wtot);
        for (u64 x = end; x; x &= x - 1) E[at++] = pos + (unsigned)amp::ctz(x) + 1u;     // ends: one set bit fewer each time
    }
}

__global__ __launch_bounds__(256) void lr_keys_kernel(const unsigned int* __restrict__ root_of, const unsigned int* __restrict__ first,
                                                      const int* __restrict__ V, int kind, unsigned int R, unsigned int* __restrict__ keys,
                                                      unsigned int* __restrict__ idx) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < R; i += gridDim.x * 256) { // ends: i grows by the grid
        keys[i] = kind == 0 ? first[root_of[i]] : (unsigned int)V[i] ^ 0x80000000u;
        idx[i] = i;
    }
}

// sorted run j: does it open an instance, and the boundaries it writes
struct LrItem {
    unsigned int s, e;
    bool head, keep_s, keep_e, close;
    __device__ unsigned int bounds() const { return (unsigned)keep_s + (unsigned)keep_e + (unsigned)close; }
};
__device__ __forceinline__ LrItem lr_item(const unsigned int* __restrict__ SK, const unsigned int* __restrict__ SI, const unsigned int* __restrict__ S,
                                          const unsigned int* __restrict__ E, unsigned int R, unsigned int j, unsigned int area) {
    LrItem it{0, 0, false, false, false, false};
    if (j >= R) return it;
    const unsigned int i = SI[j], key = SK[j];
    it.s = S[i]; it.e = E[i];
    it.head = j == 0 || SK[j - 1] != key;
    const bool last = j + 1 == R || SK[j + 1] != key;
    it.keep_s = it.head || E[SI[j - 1]] != it.s;                     // joined with the run before: it ended at the last row of the column before
    it.keep_e = last || S[SI[j + 1]] != it.e;
    it.close = last && it.e != area;
    return it;
}

__global__ __launch_bounds__(256) void lr_heads_kernel(const unsigned int* __restrict__ SK, const unsigned int* __restrict__ SI,
                                                       const unsigned int* __restrict__ S, const unsigned int* __restrict__ E, unsigned int R,
                                                       unsigned int area, unsigned int nblk, unsigned long long* __restrict__ sums) {
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const LrItem it = lr_item(SK, SI, S, E, R, blk * 256 + threadIdx.x, area);
        block_sums_256<2>(2, nblk, blk, sums, [&](int k) { return k ? it.bounds() : (unsigned)it.head; });
    }
}

// mins / maxs: {r0, c0} / {r1, c1} per instance, preset to a large value / 0
__global__ __launch_bounds__(256) void lr_emit_kernel(const unsigned int* __restrict__ SK, const unsigned int* __restrict__ SI,
                                                      const unsigned int* __restrict__ S, const unsigned int* __restrict__ E, unsigned int R,
                                                      unsigned int area, int h, int kind, unsigned int nblk,
                                                      const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ base,
                                                      unsigned int* __restrict__ rank, int* __restrict__ ids, unsigned long long* __restrict__ off,
                                                      unsigned int* __restrict__ bnd, int* __restrict__ mins, int* __restrict__ maxs,
                                                      unsigned int* __restrict__ areas) {
    __shared__ unsigned int wtot[4];
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const unsigned int j = blk * 256 + threadIdx.x;
        const LrItem it = lr_item(SK, SI, S, E, R, j, area);
        const unsigned int inst = (unsigned int)(sums[blk] - base[0]) + block_before_256((unsigned)it.head, wtot) + (unsigned)it.head - 1u;
        unsigned long long at = sums[(size_t)nblk + blk] - base[1] + block_before_256(it.bounds(), wtot);
        if (j >= R) continue;                                                            // after the barriers
        rank[j] = inst;
        if (it.head) {
            ids[inst] = kind == 0 ? (int)inst + 1 : (int)(SK[j] ^ 0x80000000u);
            off[inst] = at;
        }
        if (it.keep_s) bnd[at++] = it.s;
        if (it.keep_e) bnd[at++] = it.e;
        if (it.close) bnd[at++] = area;
        const int c = (int)(it.s / (unsigned)h), ra = (int)(it.s - (unsigned)c * (unsigned)h), rb = (int)(it.e - (unsigned)c * (unsigned)h);
        atomicMin(&mins[2 * (size_t)inst], ra);
        atomicMin(&mins[2 * (size_t)inst + 1], c);
        atomicMax(&maxs[2 * (size_t)inst], rb);
        atomicMax(&maxs[2 * (size_t)inst + 1], c + 1);
        atomicAdd(&areas[inst], it.e - it.s);
    }
}

// what the three steps below hand from one to the next
struct LrStages {
    int h, w, kind, pitch;
    unsigned long long units;
    unsigned int area, nblk, R, nblk2;            // R runs; 0: the image holds none, and lr_cut has written nothing
    unsigned long long N, listed;                 // after lr_group: the instances, the counts of their lists
    amp::DevBuf planes, sums, base, S, E, V, parent, col, keys, idx, skeys, sidx, tmp, sums2, base2, rank, ids, off, bnd, mins, maxs, areas;
};

// The h x w image d_img (on the device) cut into runs: S, E, V (LABEL), parent, col.  The host reads the number of runs back in between.
int lr_cut(const char* api, hipStream_t st, const void* d_img, int h, int w, int kind, int zero_bg, LrStages& g) {
    g.h = h; g.w = w; g.kind = kind; g.pitch = (h + 63) >> 6;
    g.units = (unsigned long long)w * g.pitch;
    const unsigned long long pixels = (unsigned long long)h * w;
    g.area = (unsigned int)pixels; g.nblk = (unsigned int)((g.units + 255) / 256);
    g.R = 0;
    AMP_TRY_STATUS(amp::dev_alloc(g.planes, (size_t)g.units * 16));
    AMP_TRY_STATUS(amp::dev_alloc(g.sums, (size_t)g.nblk * 16));
    AMP_TRY_STATUS(amp::dev_alloc(g.base, 3 * 8));
    unsigned long long *planes = g.planes.as<unsigned long long>(), *sums = g.sums.as<unsigned long long>(), *base = g.base.as<unsigned long long>();
    hipLaunchKernelGGL(lr_planes_kernel, grid_256(g.units), dim3(256), 0, st, d_img, h, w, kind, zero_bg, g.pitch, g.units, planes);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lr_count_kernel, grid_256(g.units), dim3(256), 0, st, planes, g.units, g.nblk, sums);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, sums, g.nblk, 2, base);
    AMP_HIP_CHECK(hipGetLastError());
    unsigned long long hb[3];
    AMP_HIP_CHECK(hipMemcpyAsync(hb, base, sizeof(hb), hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long runs = hb[1] - hb[0];
    if (hb[2] - hb[1] != runs || runs > pixels) {                    // cannot happen: every run has one first and one last pixel
        amp::set_error("%s: %llu run starts and %llu run ends on the device", api, runs, hb[2] - hb[1]);
        return AMP_ERR_HIP;
    }
    if (runs == 0) return AMP_OK;
    const unsigned int R = (unsigned int)runs;
    g.R = R; g.nblk2 = (R + 255) / 256;
    AMP_TRY_STATUS(amp::dev_alloc(g.S, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.E, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.V, kind == AMP_LABEL_BINARY ? 0 : (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.parent, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.col, ((size_t)w + 1) * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.keys, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.idx, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.skeys, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.sidx, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.sums2, (size_t)g.nblk2 * 16));
    AMP_TRY_STATUS(amp::dev_alloc(g.base2, 3 * 8));
    hipLaunchKernelGGL(lr_write_kernel, grid_256(g.units), dim3(256), 0, st, planes, g.units, h, w, g.pitch, g.nblk, sums, base, d_img, kind,
                       g.S.as<unsigned int>(), g.E.as<unsigned int>(), g.V.as<int>(), g.parent.as<unsigned int>(), g.col.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

// The runs grouped into instances: sorted by key (root_of, first: the roots of a BINARY image and their smallest positions; a LABEL image
// sorts by V), skeys / sidx, and the workgroup sums of the heads scanned.  The host reads N and listed back; the caller judges them.
int lr_group(hipStream_t st, const unsigned int* root_of, const unsigned int* first, LrStages& g) {
    const unsigned int R = g.R;
    unsigned int *keys = g.keys.as<unsigned int>(), *idx = g.idx.as<unsigned int>(), *skeys = g.skeys.as<unsigned int>(), *sidx = g.sidx.as<unsigned int>();
    hipLaunchKernelGGL(lr_keys_kernel, grid_256(R), dim3(256), 0, st, root_of, first, g.V.as<int>(), g.kind, R, keys, idx);
    AMP_HIP_CHECK(hipGetLastError());
    size_t tmp_bytes = 0;
    AMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, skeys, idx, sidx, (size_t)R, 0u, 32u, st));
    AMP_TRY_STATUS(amp::dev_alloc(g.tmp, tmp_bytes));
    AMP_HIP_CHECK(rocprim::radix_sort_pairs(g.tmp.p, tmp_bytes, keys, skeys, idx, sidx, (size_t)R, 0u, 32u, st));
    unsigned long long *sums2 = g.sums2.as<unsigned long long>(), *base2 = g.base2.as<unsigned long long>();
    hipLaunchKernelGGL(lr_heads_kernel, grid_256(R), dim3(256), 0, st, skeys, sidx, g.S.as<unsigned int>(), g.E.as<unsigned int>(), R, g.area, g.nblk2,
                       sums2);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, sums2, g.nblk2, 2, base2);
    AMP_HIP_CHECK(hipGetLastError());
    unsigned long long hb[3];
    AMP_HIP_CHECK(hipMemcpyAsync(hb, base2, sizeof(hb), hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    g.N = hb[1] - hb[0]; g.listed = hb[2] - hb[1];
    return AMP_OK;
}

// rank of every sorted run, ids / off / bnd / mins / maxs / areas of the N instances
int lr_emit(hipStream_t st, LrStages& g) {
    const size_t N = (size_t)g.N;
    AMP_TRY_STATUS(amp::dev_alloc(g.rank, (size_t)g.R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.ids, N * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.off, N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(g.bnd, (size_t)g.listed * 4));
    AMP_TRY_STATUS(amp::dev_alloc(g.mins, N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(g.maxs, N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(g.areas, N * 4));
    AMP_HIP_CHECK(hipMemsetAsync(g.mins.p, 0x7f, N * 8, st));                            // 0x7f7f7f7f: above every row and column
    AMP_HIP_CHECK(hipMemsetAsync(g.maxs.p, 0, N * 8, st));
    AMP_HIP_CHECK(hipMemsetAsync(g.areas.p, 0, N * 4, st));
    hipLaunchKernelGGL(lr_emit_kernel, grid_256(g.R), dim3(256), 0, st, g.skeys.as<unsigned int>(), g.sidx.as<unsigned int>(), g.S.as<unsigned int>(),
                       g.E.as<unsigned int>(), g.R, g.area, g.h, g.kind, g.nblk2, g.sums2.as<unsigned long long>(), g.base2.as<unsigned long long>(),
                       g.rank.as<unsigned int>(), g.ids.as<int>(), g.off.as<unsigned long long>(), g.bnd.as<unsigned int>(), g.mins.as<int>(),
                       g.maxs.as<int>(), g.areas.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    return AMP_OK;
}

}  // namespace
