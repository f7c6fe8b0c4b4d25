// amp_label_runs on the device: the instances of an annotation image (ampis/data_utils.py:412-428, get_ddicts 'binary' / 'label') as COCO run
// lists, boxes and areas without a dense mask per instance.  The image is cut into VERTICAL runs -- foreground runs of a BINARY image,
// constant-id runs of a LABEL image, never across a column end --, which in column-major order are the pieces of every instance's COCO run list;
// positions are those of the column-major image, col * h + row.  The launches, whatever the image holds:
//   1. lr_planes_kernel   one lane per (64 rows, column), columns fastest so a wave reads rows of the row-major image: two column-major bit
//                         planes (64 rows a word), START = the pixel opens a run, END = it closes one;
//   2. lr_count_kernel    one lane per plane word in column-major order: the set bits of both planes, a workgroup sum each;
//   3. lr_scan_kernel     one workgroup: the exclusive scan of the sums.  The host reads the number of runs R and sizes the run arrays;
//   4. lr_write_kernel    as 2 with a workgroup scan: run k's start S[k], end E[k], id V[k] (LABEL), parent[k] = k, and the first run of
//                         every column;
//   5. lr_union_kernel    BINARY: one lane per run, against the runs of the column before whose rows meet its own (one row wider on each side
//                         for 8 neighbours): lock-free union-find, the larger root hooked under the smaller by compare-and-swap (union_find.h);
//   6. lr_flatten_kernel  BINARY: every run's root, and per root the smallest row-major position of its runs (atomic min);
//   7. lr_keys_kernel     the sort key of every run -- that position, or the id with the sign bit flipped -- and the run's index as the value;
//   8. rocprim::radix_sort_pairs: stable, so the runs of an instance stay in column-major order and the instances come in key order (the
//                         library's own launches depend on R only);
//   9. lr_heads_kernel    one lane per sorted run: does it open an instance, how many boundaries it writes (none where it is joined with its
//                         neighbour across a column end; the closing h * w after an instance's last run), a workgroup sum each;
//  10. lr_scan_kernel     again.  The host reads the instances N and the counts, reports both needs and refuses a capacity that is too small;
//  11. lr_emit_kernel     as 9 with a workgroup scan: boundary positions, id and offset of every instance, box and area by atomic min / max / add;
//  12. lr_diff_kernel     one lane per count: boundary minus the boundary before it (0 in front of an instance's first);
//  13. lr_paint_kernel    when the label image is asked for: one lane per sorted run writes its rows.
// Integer arithmetic only.  The atomics are integer min / max / add and compare-and-swap on the parents: the partition into sets, and with it
// every root's smallest position, does not depend on the order of the unions; nothing is placed through a counter.  So the bytes repeat and
// equal the host's (label_runs_host.hip).  Every loop in a kernel states why it ends; none waits for another lane.  The stages that
// amp_flatten_instances shares (1-4, 7, 9-11) are in label_runs_kernels.h.
#include <string.h>

#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "label_runs_kernels.h"
#include "mask_analysis.h"
#include "union_find.h"

namespace {

__global__ __launch_bounds__(256) void lr_union_kernel(const unsigned int* __restrict__ S, const unsigned int* __restrict__ E,
                                                       const unsigned int* __restrict__ colstart, unsigned int R, int h, int d,
                                                       unsigned int* parent) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < R; i += gridDim.x * 256) { // ends: i grows by the grid (R <= 2^30, the grid < 2^25 lanes)
        const int c = (int)(S[i] / (unsigned)h);
        if (c == 0) continue;
        const int shift = h;                                                             // a run of column c - 1 moved one column right
        const int s = (int)S[i], e = (int)E[i];
        int lo = (int)colstart[c - 1], hi = (int)colstart[c];
        const int jend = hi;
        while (lo < hi) {                                                                // ends: hi - lo halves; the first run that ends below s - d
            const int mid = (lo + hi) >> 1;
            if ((int)E[mid] + shift + d <= s) lo = mid + 1; else hi = mid;
        }
        for (int j = lo; j < jend && (int)S[j] + shift < e + d; ++j) amp::uf_unite(parent, i, (unsigned)j); // ends: j grows to jend
    }
}

__global__ __launch_bounds__(256) void lr_flatten_kernel(const unsigned int* __restrict__ S, unsigned int* parent, unsigned int R, int h, int w,
                                                         unsigned int* __restrict__ root_of, unsigned int* __restrict__ first) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < R; i += gridDim.x * 256) { // ends: i grows by the grid
        const unsigned int root = amp::uf_find<false>(parent, i);                        // no parent is written in this launch
        const unsigned int c = S[i] / (unsigned)h, r = S[i] - c * (unsigned)h;
        root_of[i] = root;
        atomicMin(&first[root], r * (unsigned)w + c);
    }
}

__global__ __launch_bounds__(256) void lr_diff_kernel(const unsigned int* __restrict__ bnd, const unsigned long long* __restrict__ off, int N,
                                                      unsigned long long total, unsigned int* __restrict__ counts) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * 256) {   // ends: t grows by the grid
        const int lo = amp::owner_of(off, N, t);                                         // off[0] = 0 <= t: the instance that owns count t
        counts[t] = bnd[t] - (off[lo] == t ? 0u : bnd[t - 1]);
    }
}

__global__ __launch_bounds__(256) void lr_paint_kernel(const unsigned int* __restrict__ SI, const unsigned int* __restrict__ S,
                                                       const unsigned int* __restrict__ E, const unsigned int* __restrict__ rank, unsigned int R,
                                                       int h, int w, int* __restrict__ labels) {
    for (unsigned int j = blockIdx.x * 256 + threadIdx.x; j < R; j += gridDim.x * 256) { // ends: j grows by the grid
        const unsigned int i = SI[j], c = S[i] / (unsigned)h, ra = S[i] - c * (unsigned)h, rb = E[i] - c * (unsigned)h;
        const int v = (int)rank[j] + 1;
        for (unsigned int r = ra; r < rb; ++r) labels[(size_t)r * w + c] = v;            // ends: r grows to rb <= h
    }
}

int label_runs_device(amp_ctx* ctx, const void* image, int h, int w, int kind, int connectivity, int zero_bg, int* ids, int* boxes,
                      unsigned int* areas, uint32_t* counts, unsigned long long* counts_off, int* counts_len, int inst_cap,
                      unsigned long long counts_cap, int* labels, unsigned long long* need) {
    const int pitch = (h + 63) >> 6;
    const unsigned long long units = (unsigned long long)w * pitch, pixels = (unsigned long long)h * w;
    const unsigned int area = (unsigned int)pixels, nblk = (unsigned int)((units + 255) / 256);
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    amp::DevBuf d_img, d_planes, d_sums, d_base;
    const size_t img_bytes = (size_t)pixels * (kind == AMP_LABEL_BINARY ? 1 : 4);
    AMP_TRY_STATUS(amp::dev_alloc(d_img, img_bytes));
    AMP_HIP_CHECK(hipMemcpyAsync(d_img.p, image, img_bytes, hipMemcpyHostToDevice, st));
    AMP_TRY_STATUS(amp::dev_alloc(d_planes, (size_t)units * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_sums, (size_t)nblk * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_base, 3 * 8));
    unsigned long long *planes = d_planes.as<unsigned long long>(), *sums = d_sums.as<unsigned long long>(), *base = d_base.as<unsigned long long>();
    hipLaunchKernelGGL(lr_planes_kernel, lr_grid(units), dim3(256), 0, st, d_img.p, h, w, kind, zero_bg, pitch, units, planes);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lr_count_kernel, lr_grid(units), dim3(256), 0, st, planes, units, nblk, sums);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lr_scan_kernel, dim3(1), dim3(1024), 0, st, sums, nblk, base);
    AMP_HIP_CHECK(hipGetLastError());
    unsigned long long hb[3];
    AMP_HIP_CHECK(hipMemcpyAsync(hb, base, sizeof(hb), hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long runs = hb[1] - hb[0];
    if (hb[2] - hb[1] != runs || runs > pixels) {                    // cannot happen: every run has one first and one last pixel
        amp::set_error("amp_label_runs: %llu run starts and %llu run ends on the device", runs, hb[2] - hb[1]);
        return AMP_ERR_HIP;
    }
    if (runs == 0) {
        AMP_TRY_STATUS(amp::label_runs_capacity(0, 0, inst_cap, counts_cap, need));
        if (labels) std::fill(labels, labels + (size_t)pixels, 0);
        return AMP_OK;
    }
    const unsigned int R = (unsigned int)runs, nblk2 = (R + 255) / 256;

    amp::DevBuf d_S, d_E, d_V, d_parent, d_col, d_root, d_first, d_keys, d_idx, d_skeys, d_sidx, d_tmp, d_sums2, d_base2;
    AMP_TRY_STATUS(amp::dev_alloc(d_S, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_E, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_V, kind == AMP_LABEL_BINARY ? 0 : (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_parent, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_col, ((size_t)w + 1) * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_keys, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_idx, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_skeys, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_sidx, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_sums2, (size_t)nblk2 * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_base2, 3 * 8));
    unsigned int *S = d_S.as<unsigned int>(), *E = d_E.as<unsigned int>(), *parent = d_parent.as<unsigned int>();
    hipLaunchKernelGGL(lr_write_kernel, lr_grid(units), dim3(256), 0, st, planes, units, h, w, pitch, nblk, sums, base, d_img.p, kind, S, E,
                       d_V.as<int>(), parent, d_col.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    if (kind == AMP_LABEL_BINARY) {
        AMP_TRY_STATUS(amp::dev_alloc(d_root, (size_t)R * 4));
        AMP_TRY_STATUS(amp::dev_alloc(d_first, (size_t)R * 4));
        AMP_HIP_CHECK(hipMemsetAsync(d_first.p, 0xff, (size_t)R * 4, st));
        hipLaunchKernelGGL(lr_union_kernel, lr_grid(R), dim3(256), 0, st, S, E, d_col.as<unsigned int>(), R, h, connectivity == 2 ? 1 : 0, parent);
        AMP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(lr_flatten_kernel, lr_grid(R), dim3(256), 0, st, S, parent, R, h, w, d_root.as<unsigned int>(), d_first.as<unsigned int>());
        AMP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(lr_keys_kernel, lr_grid(R), dim3(256), 0, st, d_root.as<unsigned int>(), d_first.as<unsigned int>(), d_V.as<int>(), kind, R,
                       d_keys.as<unsigned int>(), d_idx.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    size_t tmp_bytes = 0;
    AMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_keys.as<unsigned int>(), d_skeys.as<unsigned int>(), d_idx.as<unsigned int>(),
                                            d_sidx.as<unsigned int>(), (size_t)R, 0u, 32u, st));
    AMP_TRY_STATUS(amp::dev_alloc(d_tmp, tmp_bytes));
    AMP_HIP_CHECK(rocprim::radix_sort_pairs(d_tmp.p, tmp_bytes, d_keys.as<unsigned int>(), d_skeys.as<unsigned int>(), d_idx.as<unsigned int>(),
                                            d_sidx.as<unsigned int>(), (size_t)R, 0u, 32u, st));
    const unsigned int *SK = d_skeys.as<unsigned int>(), *SI = d_sidx.as<unsigned int>();
    unsigned long long *sums2 = d_sums2.as<unsigned long long>(), *base2 = d_base2.as<unsigned long long>();
    hipLaunchKernelGGL(lr_heads_kernel, lr_grid(R), dim3(256), 0, st, SK, SI, S, E, R, area, nblk2, sums2);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lr_scan_kernel, dim3(1), dim3(1024), 0, st, sums2, nblk2, base2);
    AMP_HIP_CHECK(hipGetLastError());
    AMP_HIP_CHECK(hipMemcpyAsync(hb, base2, sizeof(hb), hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long N = hb[1] - hb[0], total = hb[2] - hb[1];
    if (N == 0 || N > R || total < 2 * N || total > 3ull * R) {      // cannot happen: a run opens at most one instance and writes at most three boundaries
        amp::set_error("amp_label_runs: %llu instances and %llu counts from %u runs on the device", N, total, R);
        return AMP_ERR_HIP;
    }
    AMP_TRY_STATUS(amp::label_runs_capacity(N, total, inst_cap, counts_cap, need));

    amp::DevBuf d_rank, d_ids, d_off, d_bnd, d_counts, d_mins, d_maxs, d_areas, d_labels;
    AMP_TRY_STATUS(amp::dev_alloc(d_rank, (size_t)R * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_ids, (size_t)N * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_off, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_bnd, (size_t)total * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_counts, (size_t)total * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_mins, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_maxs, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_areas, (size_t)N * 4));
    AMP_HIP_CHECK(hipMemsetAsync(d_mins.p, 0x7f, (size_t)N * 8, st));                    // 0x7f7f7f7f: above every row and column
    AMP_HIP_CHECK(hipMemsetAsync(d_maxs.p, 0, (size_t)N * 8, st));
    AMP_HIP_CHECK(hipMemsetAsync(d_areas.p, 0, (size_t)N * 4, st));
    hipLaunchKernelGGL(lr_emit_kernel, lr_grid(R), dim3(256), 0, st, SK, SI, S, E, R, area, h, kind, nblk2, sums2, base2, d_rank.as<unsigned int>(),
                       d_ids.as<int>(), d_off.as<unsigned long long>(), d_bnd.as<unsigned int>(), d_mins.as<int>(), d_maxs.as<int>(),
                       d_areas.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lr_diff_kernel, lr_grid(total), dim3(256), 0, st, d_bnd.as<unsigned int>(), d_off.as<unsigned long long>(), (int)N, total,
                       d_counts.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    if (labels) {
        AMP_TRY_STATUS(amp::dev_alloc(d_labels, (size_t)pixels * 4));
        AMP_HIP_CHECK(hipMemsetAsync(d_labels.p, 0, (size_t)pixels * 4, st));
        hipLaunchKernelGGL(lr_paint_kernel, lr_grid(R), dim3(256), 0, st, SI, S, E, d_rank.as<unsigned int>(), R, h, w, d_labels.as<int>());
        AMP_HIP_CHECK(hipGetLastError());
    }
    std::vector<int> mins(2 * (size_t)N), maxs(2 * (size_t)N);
    AMP_HIP_CHECK(hipMemcpyAsync(mins.data(), d_mins.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(maxs.data(), d_maxs.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    AMP_HIP_CHECK(hipMemcpyAsync(ids, d_ids.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(areas, d_areas.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(counts_off, d_off.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    if (labels) AMP_HIP_CHECK(hipMemcpyAsync(labels, d_labels.p, (size_t)pixels * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t n = 0; n < (size_t)N; ++n) {
        boxes[4 * n] = mins[2 * n]; boxes[4 * n + 1] = mins[2 * n + 1]; boxes[4 * n + 2] = maxs[2 * n]; boxes[4 * n + 3] = maxs[2 * n + 1];
        counts_len[n] = (int)((n + 1 < (size_t)N ? counts_off[n + 1] : total) - counts_off[n]);
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_label_runs(amp_ctx* ctx, const void* image, int h, int w, int kind, int connectivity, int zero_is_background, int* ids,
                              int* boxes, unsigned int* areas, uint32_t* counts, unsigned long long* counts_off, int* counts_len, int inst_cap,
                              unsigned long long counts_cap, int* labels, unsigned long long* need) {
    AMP_TRY_STATUS(amp::label_runs_check(image, h, w, kind, connectivity, ids, boxes, areas, counts, counts_off, counts_len, inst_cap, need));
    return ctx ? label_runs_device(ctx, image, h, w, kind, connectivity, zero_is_background, ids, boxes, areas, counts, counts_off, counts_len,
                                   inst_cap, counts_cap, labels, need)
               : amp::label_runs_host(image, h, w, kind, connectivity, zero_is_background, ids, boxes, areas, counts, counts_off, counts_len,
                                      inst_cap, counts_cap, labels, need);
}
