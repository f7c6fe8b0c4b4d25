// amp_label_runs on the device: the instances of an annotation image (ampis/data_utils.py:412-428, get_ddicts 'binary' / 'label') as COCO run
// lists, boxes and areas without a dense mask per instance.  The image is cut into VERTICAL runs -- foreground runs of a BINARY image,
// constant-id runs of a LABEL image, never across a column end --, which in column-major order are the pieces of every instance's COCO run list;
// positions are those of the column-major image, col * h + row.  The launches, whatever the image holds:
//   1. lr_planes_kernel   one lane per (64 rows, column), columns fastest so a wave reads rows of the row-major image: two column-major bit
//                         planes (64 rows a word), START = the pixel opens a run, END = it closes one;
//   2. lr_count_kernel    one lane per plane word in column-major order: the set bits of both planes, a workgroup sum each;
//   3. scan_sums_kernel   one workgroup: the exclusive scan of the sums.  The host reads the number of runs R and sizes the run arrays;
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
//  10. scan_sums_kernel   again.  The host reads the instances N and the counts, reports both needs and refuses a capacity that is too small;
//  11. lr_emit_kernel     as 9 with a workgroup scan: boundary positions, id and offset of every instance, box and area by atomic min / max / add;
//  12. diff_counts_kernel one lane per count: boundary minus the boundary before it (0 in front of an instance's first);
//  13. lr_paint_kernel    when the label image is asked for: one lane per sorted run writes its rows.
// Integer arithmetic only.  The atomics are integer min / max / add and compare-and-swap on the parents: the partition into sets, and with it
// every root's smallest position, does not depend on the order of the unions; nothing is placed through a counter.  So the bytes repeat and
// equal the host's (label_runs_host.hip).  Every loop in a kernel states why it ends; none waits for another lane.  The stages that
// amp_flatten_instances shares (1-4, 7-11) and the host functions that drive them (lr_cut: 1-4, lr_group: 7-10, lr_emit: 11) are in
// label_runs_kernels.h; the scan and the differences (3, 10, 12) are compaction.h's.
#include <string.h>

#include <vector>

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
    const unsigned long long pixels = (unsigned long long)h * w;
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    amp::DevBuf d_img, d_root, d_first, d_counts, d_labels;
    LrStages g;
    const size_t img_bytes = (size_t)pixels * (kind == AMP_LABEL_BINARY ? 1 : 4);
    AMP_TRY_STATUS(amp::dev_alloc(d_img, img_bytes));
    AMP_HIP_CHECK(hipMemcpyAsync(d_img.p, image, img_bytes, hipMemcpyHostToDevice, st));
    AMP_TRY_STATUS(lr_cut("amp_label_runs", st, d_img.p, h, w, kind, zero_bg, g));
    if (g.R == 0) {
        AMP_TRY_STATUS(amp::label_runs_capacity(0, 0, inst_cap, counts_cap, need));
        if (labels) std::fill(labels, labels + (size_t)pixels, 0);
        return AMP_OK;
    }
    const unsigned int R = g.R;
    unsigned int *S = g.S.as<unsigned int>(), *E = g.E.as<unsigned int>(), *parent = g.parent.as<unsigned int>();
    if (kind == AMP_LABEL_BINARY) {
        AMP_TRY_STATUS(amp::dev_alloc(d_root, (size_t)R * 4));
        AMP_TRY_STATUS(amp::dev_alloc(d_first, (size_t)R * 4));
        AMP_HIP_CHECK(hipMemsetAsync(d_first.p, 0xff, (size_t)R * 4, st));
        hipLaunchKernelGGL(lr_union_kernel, grid_256(R), dim3(256), 0, st, S, E, g.col.as<unsigned int>(), R, h, connectivity == 2 ? 1 : 0, parent);
        AMP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(lr_flatten_kernel, grid_256(R), dim3(256), 0, st, S, parent, R, h, w, d_root.as<unsigned int>(), d_first.as<unsigned int>());
        AMP_HIP_CHECK(hipGetLastError());
    }
    AMP_TRY_STATUS(lr_group(st, d_root.as<unsigned int>(), d_first.as<unsigned int>(), g));
    const unsigned long long N = g.N, total = g.listed;
    if (N == 0 || N > R || total < 2 * N || total > 3ull * R) {      // cannot happen: a run opens at most one instance and writes at most three boundaries
        amp::set_error("amp_label_runs: %llu instances and %llu counts from %u runs on the device", N, total, R);
        return AMP_ERR_HIP;
    }
    AMP_TRY_STATUS(amp::label_runs_capacity(N, total, inst_cap, counts_cap, need));

    AMP_TRY_STATUS(amp::dev_alloc(d_counts, (size_t)total * 4));
    AMP_TRY_STATUS(lr_emit(st, g));
    hipLaunchKernelGGL(diff_counts_kernel, grid_256(total), dim3(256), 0, st, g.bnd.as<unsigned int>(), g.off.as<unsigned long long>(), (int)N, total,
                       d_counts.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    if (labels) {
        AMP_TRY_STATUS(amp::dev_alloc(d_labels, (size_t)pixels * 4));
        AMP_HIP_CHECK(hipMemsetAsync(d_labels.p, 0, (size_t)pixels * 4, st));
        hipLaunchKernelGGL(lr_paint_kernel, grid_256(R), dim3(256), 0, st, g.sidx.as<unsigned int>(), S, E, g.rank.as<unsigned int>(), R, h, w,
                           d_labels.as<int>());
        AMP_HIP_CHECK(hipGetLastError());
    }
    std::vector<int> mins(2 * (size_t)N), maxs(2 * (size_t)N);
    AMP_HIP_CHECK(hipMemcpyAsync(mins.data(), g.mins.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(maxs.data(), g.maxs.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));                         // everything computed: the outputs are written from here on
    AMP_HIP_CHECK(hipMemcpyAsync(ids, g.ids.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(areas, g.areas.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(counts_off, g.off.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
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
