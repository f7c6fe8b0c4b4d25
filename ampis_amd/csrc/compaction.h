// The compaction toolkit of the run-list ops (label_runs_kernels.h, mask_parts.hip, seg_class_map.hip, polygon_runs.hip, edge_distance.hip):
// count per lane, sum per workgroup, scan the sums in one workgroup, scan inside the workgroup again and write every item where the two scans
// say.  What those ops share of it exists here once:
//   grid_256           the grid of a grid-stride kernel of 256 threads a workgroup;
//   block_sums_256     the workgroup's sum of K values a lane, to sums[k * nblk + blk];
//   scan_sums_in_place one workgroup of 1024: an array becomes its exclusive scan, the caller notes what it needs on the way;
//   scan_sums_kernel   that scan as a kernel for K quantities of nblk sums each: where each starts, and the total;
//   block_before_256   what lies in front of a lane in its workgroup;
//   diff_counts_kernel boundaries to counts;
//   count_offsets_kernel / run_counts_kernel  the last two stages of the ops that find a pool's boundaries among sorted events
//                      (polygon_runs.hip, morphology.hip): where every mask's counts start, and the counts with box and area.
// Fixed trees and no atomics: the order is fixed and the bytes repeat.  Every loop states why it ends; none waits for another lane.  For hipcc
// only; every file that includes this header gets kernels of its own.
#pragma once
#include <algorithm>

#include "common.h"
#include "run_list.h"

namespace {

// at least one workgroup, at most 2^16: the kernels stride by the grid
inline dim3 grid_256(unsigned long long items) {
    return dim3((unsigned)std::min<unsigned long long>(std::max<unsigned long long>((items + 255) / 256, 1ull), 1ull << 16));
}

// sums[k * nblk + blk] = the sum of this lane's value(k) over the workgroup of 256, k < n <= K; every thread calls it, and it ends with a
// barrier
template <int K, class Value>
__device__ __forceinline__ void block_sums_256(int n, unsigned int nblk, unsigned int blk, unsigned long long* __restrict__ sums, Value value) {
    __shared__ unsigned long long part[4][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < n; ++k) {                                                        // ends: n <= K steps
        const unsigned long long s = amp::wave_sum((unsigned long long)value(k));
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < n) sums[(size_t)threadIdx.x * nblk + blk] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    __syncthreads();
}

// One workgroup of 1024, every thread calls it: sums[0 .. m) becomes its exclusive scan, thread t taking the chunk [t * chunk, (t + 1) * chunk)
// clamped to m.  visit(i, run) sees every element's index and scanned value, in the thread that owns it; tot is the LDS array of
// block_scan_1024, tot[1023] the total once this returns.
template <class Visit>
__device__ __forceinline__ void scan_sums_in_place(unsigned long long* __restrict__ sums, unsigned long long m, unsigned long long* tot, Visit visit) {
    const unsigned long long chunk = (m + 1023) / 1024, first = min(chunk * threadIdx.x, m), last = min(first + chunk, m);
    unsigned long long s = 0;
    for (unsigned long long i = first; i < last; ++i) s += sums[i];                      // ends: i grows to last
    unsigned long long run = amp::block_scan_1024(tot, s) - s;                           // what lies in front of this thread's chunk
    for (unsigned long long i = first; i < last; ++i) {                                  // ends: i grows to last
        const unsigned long long v = sums[i];
        sums[i] = run;
        visit(i, run);
        run += v;
    }
}

// one workgroup of 1024: sums[0 .. K nblk), K quantities of nblk workgroup sums each, becomes its exclusive scan; base[k] = where quantity k
// starts in it, base[K] = the total
__global__ __launch_bounds__(1024) void scan_sums_kernel(unsigned long long* __restrict__ sums, unsigned int nblk, int K,
                                                         unsigned long long* __restrict__ base) {
    __shared__ unsigned long long tot[1024];
    scan_sums_in_place(sums, (unsigned long long)K * nblk, tot, [&](unsigned long long i, unsigned long long run) {
        for (int k = 0; k < K; ++k)                                                      // ends: K steps
            if (i == (unsigned long long)k * nblk) base[k] = run;
    });
    if (threadIdx.x == 0) base[K] = tot[1023];
}

// what lies in front of this lane in its workgroup (exclusive scan of c over 256 threads) and, when asked for, the workgroup's sum; every
// thread calls it
__device__ __forceinline__ unsigned int block_before_256(unsigned int c, unsigned int* wtot, unsigned int* total = nullptr) {
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
    if (total) *total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    return before;
}

// one lane per count: boundary minus the boundary before it, 0 in front of the first of a list; off [n] ascending = where every list starts
__global__ __launch_bounds__(256) void diff_counts_kernel(const unsigned int* __restrict__ bnd, const unsigned long long* __restrict__ off, int n,
                                                          unsigned long long total, unsigned int* __restrict__ counts) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * 256) {   // ends: t grows by the grid
        const int lo = amp::owner_of(off, n, t);                                         // off[0] = 0 <= t, every list has a count: the list that owns count t
        counts[t] = bnd[t] - (off[lo] == t ? 0u : bnd[t - 1]);
    }
}

// coff[i] = where mask i's counts start: the boundaries of the masks before it and one closing count each (bidx: the exclusive scan of the
// boundary flags over the sorted events, ioff[i]: mask i's first event); the box and the area of every mask preset for the atomics of
// run_counts_kernel
__global__ __launch_bounds__(256) void count_offsets_kernel(const unsigned int* __restrict__ bidx, const unsigned int* __restrict__ ioff, int n,
                                                            unsigned long long* __restrict__ coff, int* __restrict__ mins, int* __restrict__ maxs,
                                                            unsigned int* __restrict__ areas) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i <= n; i += gridDim.x * 256) {         // ends: i grows by the grid
        coff[i] = (unsigned long long)bidx[ioff[i]] + (unsigned long long)i;
        if (i < n) { mins[2 * i] = 0x7fffffff; mins[2 * i + 1] = 0x7fffffff; maxs[2 * i] = 0; maxs[2 * i + 1] = 0; areas[i] = 0; }
    }
}

// one lane per count: boundary minus the boundary before, the closing count up to area = h * w; the runs of ones give box {row, column} and
// area by atomic min / max / add.  bnd: the boundaries of all masks back to back, mask i's behind the coff[i] - i of the masks before it
__global__ __launch_bounds__(256) void run_counts_kernel(const unsigned int* __restrict__ bnd, const unsigned long long* __restrict__ coff, int n,
                                                         unsigned long long total, int h, unsigned int area, unsigned int* __restrict__ counts,
                                                         int* __restrict__ mins, int* __restrict__ maxs, unsigned int* __restrict__ areas) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * 256) {   // ends: t grows by the grid
        const int i = amp::owner_of(coff, n, t);                                         // coff[0] = 0 <= t < coff[n] = total, every mask has a count
        const unsigned long long j = t - coff[i], nb = coff[i + 1] - coff[i] - 1, b0 = coff[i] - (unsigned long long)i;
        const unsigned int s = j > 0 ? bnd[b0 + j - 1] : 0u, e = j < nb ? bnd[b0 + j] : area;
        counts[t] = e - s;
        if (!(j & 1ull) || e == s) continue;                                             // pixels [s, e) are a run of ones
        const int cf = (int)(s / (unsigned)h), cl = (int)((e - 1) / (unsigned)h);
        const int ra = cf == cl ? (int)(s - (unsigned)cf * (unsigned)h) : 0, rb = cf == cl ? (int)(e - (unsigned)cf * (unsigned)h) : h;
        atomicMin(&mins[2 * (size_t)i], ra);
        atomicMin(&mins[2 * (size_t)i + 1], cf);
        atomicMax(&maxs[2 * (size_t)i], rb);
        atomicMax(&maxs[2 * (size_t)i + 1], cl + 1);
        atomicAdd(&areas[i], e - s);
    }
}

}  // namespace
