// The run stages of a label image on the device, shared by label_runs.hip (amp_label_runs: the instances of an annotation image) and
// flatten.hip (amp_flatten_instances: the visible lists are the per-id runs of the owner map), moved out of label_runs.hip unchanged the way
// union_find.h was.  The image is cut into VERTICAL runs -- foreground runs of a BINARY image, constant-id runs of a LABEL image, never
// across a column end --, which in column-major order are the pieces of every instance's COCO run list; positions are those of the
// column-major image, col * h + row.
//   lr_planes_kernel   one lane per (64 rows, column), columns fastest so a wave reads rows of the row-major image: two column-major bit
//                      planes (64 rows a word), START = the pixel opens a run, END = it closes one;
//   lr_count_kernel    one lane per plane word in column-major order: the set bits of both planes, a workgroup sum each;
//   lr_scan_kernel     one workgroup: the exclusive scan of the sums;
//   lr_write_kernel    as lr_count_kernel with a workgroup scan: run k's start S[k], end E[k], id V[k] (LABEL), parent[k] = k, and the first
//                      run of every column;
//   lr_keys_kernel     the sort key of every run -- its root's smallest position, or the id with the sign bit flipped -- and the run's index
//                      as the value, for a stable radix sort;
//   lr_heads_kernel    one lane per sorted run: does it open an instance, how many boundaries it writes (none where it is joined with its
//                      neighbour across a column end; the closing h * w after an instance's last run), a workgroup sum each;
//   lr_emit_kernel     as lr_heads_kernel with a workgroup scan: boundary positions, id and offset of every instance, box and area by atomic
//                      min / max / add.
// Integer arithmetic only; nothing is placed through a counter, so the bytes repeat.  Every loop states why it ends; none waits for
// another lane.  For hipcc only; every file that includes this header gets kernels of its own.
#pragma once
#include <algorithm>

#include "common.h"
#include "mask_analysis.h"

namespace {

using amp::u64;
using amp::wave_sum;

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
    __shared__ unsigned long long part[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const unsigned long long u = (unsigned long long)blk * 256 + threadIdx.x;
        for (int k = 0; k < 2; ++k) {
            const unsigned long long s = wave_sum((unsigned long long)(u < units ? amp::popc(planes[k * units + u]) : 0));
            if (lane == 0) part[wave][k] = s;
        }
        __syncthreads();
        if (threadIdx.x < 2) sums[(size_t)threadIdx.x * nblk + blk] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        __syncthreads();
    }
}

// one workgroup of 1024: sums[0 .. 2 nblk) becomes its exclusive scan; base[k] = where quantity k starts in it, base[2] = the total
__global__ __launch_bounds__(1024) void lr_scan_kernel(unsigned long long* __restrict__ sums, unsigned int nblk, unsigned long long* __restrict__ base) {
    __shared__ unsigned long long tot[1024];
    const unsigned long long m = 2ull * nblk, chunk = (m + 1023) / 1024, first = chunk * threadIdx.x, last = min(first + chunk, m);
    unsigned long long s = 0;
    for (unsigned long long i = first; i < last; ++i) s += sums[i];                      // ends: i grows to last
    unsigned long long run = amp::block_scan_1024(tot, s) - s;
    for (unsigned long long i = first; i < last; ++i) {                                  // ends: i grows to last
        const unsigned long long v = sums[i];
        sums[i] = run;
        if (i == 0 || i == nblk) base[i / nblk] = run;
        run += v;
    }
    if (threadIdx.x == 0) base[2] = tot[1023];
}

// what lies in front of this lane in its workgroup (exclusive scan of c over 256 threads); every thread calls it
__device__ __forceinline__ unsigned int lr_block_before(unsigned int c, unsigned int* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int inc = c;
    for (int o = 1; o < 64; o <<= 1) {                                                   // ends: six steps
        const unsigned int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    __syncthreads();                                                                     // wtot of the call before has been read
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned int before = inc - c;
    for (int v = 0; v < wave; ++v) before += wtot[v];                                    // ends: at most three waves
    return before;
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
        unsigned int at = (unsigned int)(sums[blk] - base[0]) + lr_block_before((unsigned)amp::popc(start), wtot);
        if (in && wv == 0) colstart[c] = at;
        for (u64 x = start; x; x &= x - 1) {                                             // ends: one set bit fewer each time
            const int b = amp::ctz(x);
            S[at] = pos + (unsigned)b;
            parent[at] = at;
            if (kind != 0) V[at] = amp::label_pixel(img, kind, (size_t)((wv << 6) + b) * w + c);
            ++at;
        }
        if (in && u == units - 1) colstart[w] = at;
        at = (unsigned int)(sums[(size_t)nblk + blk] - base[1]) + lr_block_before((unsigned)amp::popc(end), wtot);
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
    __shared__ unsigned long long part[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {                  // ends: blk grows by the grid; uniform over the workgroup
        const LrItem it = lr_item(SK, SI, S, E, R, blk * 256 + threadIdx.x, area);
        const unsigned long long a = wave_sum((unsigned long long)it.head), b = wave_sum((unsigned long long)it.bounds());
        if (lane == 0) { part[wave][0] = a; part[wave][1] = b; }
        __syncthreads();
        if (threadIdx.x < 2) sums[(size_t)threadIdx.x * nblk + blk] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        __syncthreads();
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
        const unsigned int inst = (unsigned int)(sums[blk] - base[0]) + lr_block_before((unsigned)it.head, wtot) + (unsigned)it.head - 1u;
        unsigned long long at = sums[(size_t)nblk + blk] - base[1] + lr_block_before(it.bounds(), wtot);
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

dim3 lr_grid(unsigned long long items) { return dim3((unsigned)std::min<unsigned long long>(std::max<unsigned long long>((items + 255) / 256, 1ull), 1ull << 16)); }

}  // namespace
