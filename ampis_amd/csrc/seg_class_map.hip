// Segmentation class map on the device (ampis/analyze.py:589-699, seg_perf_iset: decode every mask to the image, three [pairs x h x w] bool
// arrays, OR over the pairs, code every pixel, encode 4 or 7 class masks).  Here the masks stay run lists until they are three COLUMN-major bit
// planes of the image -- TP = OR (g & q), FN = OR (g & ~q), FP = OR (~g & q), 64 rows a word, ceil(h / 64) words a column -- and the class
// masks leave as run lists again.  The host plan (run_list.h, built by the argument checks in mask_analysis_host.hip) keeps per named mask the
// positions [S, E) of its runs of ones and the tight box; an item is one (pair, column, word) of the union of a pair's two boxes:
//   1. sc_paint_kernel   one lane per item, grid-stride.  The lane finds its pair by binary search over the item offsets, builds the 64 rows of
//                        g and of q from the runs that meet them (binary search over the run ends for the first, then the runs in order: at
//                        most 32 a word) and ORs g & q, g & ~q, ~g & q into the planes with 64-bit atomic OR;
//   2. sc_count_kernel   one lane per plane word: the class words of the mode (seg_class_map.h), their transitions against the pixel before
//                        the word -- row 63 of the word above or the last row of the previous column: the run lists are column-major over
//                        the whole image and the padding rows of a column's last word do not exist --, a workgroup sum per class; the eight
//                        code counts by popcount, a wave sum and one 64-bit atomic add per wave and code;
//   3. sc_scan_kernel    one workgroup: the exclusive scan of the classes x workgroups sums in class-major order, the offsets of the K run
//                        lists and the closing boundary h * w of each;
//   4. sc_write_kernel   as 2, with a workgroup scan: every transition writes its pixel position where the scan says;
//   5. sc_diff_kernel    one lane per count: boundary minus the boundary before it (0 in front of a class's first).
// The workgroup sums of 2, the scan loop of 3 and the workgroup scan of 4 are compaction.h's.
// Five launches and one memset per call whatever the number of pairs.  Integer arithmetic only; the atomics are 64-bit ORs and adds, whose
// results do not depend on the order, and every other word is written once by the lane that owns it: the bytes repeat and equal the host's
// (mask_analysis_host.hip paints the planes by one walk over the two run lists of a pair and reads the same words).  Scratch: the plan, three planes of
// h * w bits, two buffers of the counts capacity.
#include <vector>

#include "common.h"
#include "compaction.h"
#include "mask_analysis.h"
#include "seg_class_map.h"

namespace {

using amp::RunMask;
using amp::u64;
using amp::wave_sum;

struct ScPair {
    int g, q;                     // masks of the two plans
    int c0, wv0, nwords, pad;     // first column and first word row of the union box, words per column of the box
};

__global__ __launch_bounds__(256) void sc_paint_kernel(const ScPair* __restrict__ pairs, int n, const unsigned long long* __restrict__ ioff,
                                                       unsigned long long total, const RunMask* __restrict__ gm, const RunMask* __restrict__ pm,
                                                       const unsigned int* __restrict__ gS, const unsigned int* __restrict__ gE,
                                                       const unsigned int* __restrict__ pS, const unsigned int* __restrict__ pE,
                                                       unsigned long long* __restrict__ planes, unsigned long long units, int h, int pitch) {
    for (unsigned long long it = (unsigned long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (unsigned long long)gridDim.x * 256) {
        const int lo = amp::owner_of(ioff, n, it);                   // the pair that owns item it
        const ScPair pr = pairs[lo];
        const unsigned int local = (unsigned int)(it - ioff[lo]);
        const int col = pr.c0 + (int)(local / (unsigned)pr.nwords), wv = pr.wv0 + (int)(local % (unsigned)pr.nwords);
        const unsigned int a = (unsigned)col * (unsigned)h + ((unsigned)wv << 6), b = min(a + 64u, ((unsigned)col + 1u) * (unsigned)h);
        const RunMask G = gm[pr.g], Q = pm[pr.q];
        const u64 g = amp::mask_word(gS + G.ro, gE + G.ro, G.n, a, b), q = amp::mask_word(pS + Q.ro, pE + Q.ro, Q.n, a, b);
        unsigned long long* at = planes + (size_t)col * pitch + wv;
        if (g & q) atomicOr(at, g & q);
        if (g & ~q) atomicOr(at + units, g & ~q);
        if (~g & q) atomicOr(at + 2 * units, ~g & q);
    }
}

// the transition words of plane word u for the K classes; false beyond the planes
__device__ __forceinline__ bool sc_word_transitions(const unsigned long long* __restrict__ planes, unsigned long long units, unsigned long long u,
                                                    int h, int pitch, int mode, int K, u64* t, u64* tp, u64* fn, u64* fp, u64* valid) {
    for (int k = 0; k < 7; ++k) t[k] = 0;
    if (u >= units) return false;
    const int wv = (int)(u % (unsigned)pitch);
    *valid = amp::sc_valid(h, wv);
    *tp = planes[u]; *fn = planes[units + u]; *fp = planes[2 * units + u];
    const int pb = amp::sc_prev_bit(h, wv);
    const u64 qt = u ? (planes[u - 1] >> pb) & 1ull : 0ull, qf = u ? (planes[units + u - 1] >> pb) & 1ull : 0ull,
                 qp = u ? (planes[2 * units + u - 1] >> pb) & 1ull : 0ull;
    for (int k = 0; k < K; ++k)
        t[k] = amp::sc_transitions(amp::sc_class_word(*tp, *fn, *fp, mode, k) & *valid, amp::sc_class_word(qt, qf, qp, mode, k), *valid);
    return true;
}

// workgroup b owns plane words [256 b, 256 b + 256); sums[k * nblk + b] = the transitions of class k in them; px[8] += the code counts
__global__ __launch_bounds__(256) void sc_count_kernel(const unsigned long long* __restrict__ planes, unsigned long long units, int h, int pitch,
                                                       int mode, int K, unsigned int nblk, unsigned long long* __restrict__ sums,
                                                       unsigned long long* __restrict__ px) {
    const int lane = threadIdx.x & 63;
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {          // uniform over the workgroup: every thread meets every barrier
        const unsigned long long u = (unsigned long long)blk * 256 + threadIdx.x;
        u64 t[7], tp = 0, fn = 0, fp = 0, valid = 0;
        sc_word_transitions(planes, units, u, h, pitch, mode, K, t, &tp, &fn, &fp, &valid);      // beyond the planes: valid = 0, nothing counts
        for (int c = 0; c < 8; ++c) {
            const unsigned long long s = wave_sum((unsigned long long)amp::popc(amp::sc_code_word(tp, fn, fp, c) & valid));
            if (lane == 0 && s) atomicAdd(&px[c], s);
        }
        block_sums_256<7>(K, nblk, blk, sums, [&](int k) { return amp::popc(t[k]); });
    }
}

// one workgroup of 1024: sums[0 .. m) becomes its exclusive scan; coff[k] = where class k's counts start (its boundaries + one closing entry
// each), coff[K] = all counts; the closing boundary h * w of every class is written
__global__ __launch_bounds__(1024) void sc_scan_kernel(unsigned long long* __restrict__ sums, unsigned long long m, unsigned int nblk, int K,
                                                       unsigned int area, unsigned long long* __restrict__ coff, unsigned int* __restrict__ bnd) {
    __shared__ unsigned long long tot[1024];
    __shared__ unsigned long long start[7];
    scan_sums_in_place(sums, m, tot, [&](unsigned long long i, unsigned long long run) {
        if (i % nblk == 0) start[i / nblk] = run;                    // the first workgroup of a class: where the class's boundaries start
    });
    __syncthreads();
    if ((int)threadIdx.x <= K) {
        const int k = threadIdx.x;
        const unsigned long long at = (k < K ? start[k] : tot[1023]) + (unsigned long long)k;
        coff[k] = at;
        if (k > 0) bnd[at - 1] = area;                               // the closing entry of class k - 1
    }
}

// boundary positions: class k's boundary number j lies at bnd[coff[k] + j]
__global__ __launch_bounds__(256) void sc_write_kernel(const unsigned long long* __restrict__ planes, unsigned long long units, int h, int pitch,
                                                       int mode, int K, unsigned int nblk, const unsigned long long* __restrict__ sums,
                                                       unsigned int* __restrict__ bnd) {
    __shared__ unsigned int wtot[4];
    for (unsigned int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {          // uniform over the workgroup: every thread meets every barrier
        const unsigned long long u = (unsigned long long)blk * 256 + threadIdx.x;
        u64 t[7], tp = 0, fn = 0, fp = 0, valid = 0;
        sc_word_transitions(planes, units, u, h, pitch, mode, K, t, &tp, &fn, &fp, &valid);
        const unsigned int base = (unsigned int)(u / (unsigned)pitch) * (unsigned)h + ((unsigned int)(u % (unsigned)pitch) << 6);
        for (int k = 0; k < K; ++k) {                                // the barrier that opens a scan protects the wtot of the class before
            unsigned long long at = sums[(size_t)k * nblk + blk] + (unsigned long long)k + block_before_256((unsigned)amp::popc(t[k]), wtot);
            for (u64 x = t[k]; x; x &= x - 1) bnd[at++] = base + (unsigned)amp::ctz(x);
        }
    }
}

__global__ __launch_bounds__(256) void sc_diff_kernel(const unsigned int* __restrict__ bnd, const unsigned long long* __restrict__ coff, int K,
                                                      unsigned int* __restrict__ counts) {
    const unsigned long long total = coff[K];
    for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < total; j += (unsigned long long)gridDim.x * 256) {
        bool first = false;
        for (int k = 0; k < K; ++k) first |= coff[k] == j;
        counts[j] = bnd[j] - (first ? 0u : bnd[j - 1]);
    }
}

static int seg_class_map_device(amp_ctx* ctx, const amp::RunPlan& g, const amp::RunPlan& p, const int* pair_g, const int* pair_p, int n, int h, int w,
                                int mode, unsigned long long need, uint32_t* counts, unsigned long long* counts_off, unsigned long long* pixels) {
    const int pitch = (h + 63) >> 6, K = amp::sc_classes(mode);
    const unsigned long long units = (unsigned long long)w * pitch;
    std::vector<ScPair> pairs;
    std::vector<unsigned long long> ioff(1, 0ull);
    for (int i = 0; i < n; ++i) {
        const RunMask& G = g.m[(size_t)pair_g[i]];
        const RunMask& Q = p.m[(size_t)pair_p[i]];
        if (G.n == 0 && Q.n == 0) continue;                          // two masks without a pixel paint nothing
        const RunMask& A = G.n ? G : Q;
        const RunMask& B = Q.n ? Q : G;
        const int r0 = std::min(A.r0, B.r0), r1 = std::max(A.r1, B.r1), c0 = std::min(A.c0, B.c0), c1 = std::max(A.c1, B.c1);
        const int wv0 = r0 >> 6, nwords = ((r1 - 1) >> 6) - wv0 + 1;
        pairs.push_back(ScPair{pair_g[i], pair_p[i], c0, wv0, nwords, 0});
        ioff.push_back(ioff.back() + (unsigned long long)(c1 - c0) * (unsigned long long)nwords);
    }
    const int npairs = (int)pairs.size();
    const unsigned long long items = ioff.back();
    const unsigned int nblk = (unsigned int)((units + 255) / 256);
    const unsigned long long m = (unsigned long long)K * nblk;

    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_pairs, d_ioff, d_gm, d_pm, d_gS, d_gE, d_pS, d_pE, d_planes, d_sums, d_bnd, d_counts;
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_pairs, pairs));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_ioff, ioff));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_gm, g.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_pm, p.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_gS, g.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_gE, g.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_pS, p.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_pE, p.E));
    const size_t plane_words = (size_t)(3 * units + 8 + 8);          // the planes, the eight code counts, the K + 1 offsets
    AMP_TRY_STATUS(amp::dev_alloc(d_planes, plane_words * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_sums, (size_t)m * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_bnd, (size_t)need * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_counts, (size_t)need * 4));
    unsigned long long* planes = d_planes.as<unsigned long long>();
    unsigned long long *px = planes + 3 * units, *coff = px + 8;
    AMP_HIP_CHECK(hipMemsetAsync(planes, 0, plane_words * 8, st));
    if (items) {
        const dim3 grid((unsigned)std::min<unsigned long long>((items + 255) / 256, 1ull << 16));
        hipLaunchKernelGGL(sc_paint_kernel, grid, dim3(256), 0, st, d_pairs.as<ScPair>(), npairs, d_ioff.as<unsigned long long>(), items,
                           d_gm.as<RunMask>(), d_pm.as<RunMask>(), d_gS.as<unsigned int>(), d_gE.as<unsigned int>(), d_pS.as<unsigned int>(),
                           d_pE.as<unsigned int>(), planes, units, h, pitch);
        AMP_HIP_CHECK(hipGetLastError());
    }
    const dim3 wgrid(std::min(nblk, 1u << 16));
    hipLaunchKernelGGL(sc_count_kernel, wgrid, dim3(256), 0, st, planes, units, h, pitch, mode, K, nblk, d_sums.as<unsigned long long>(), px);
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sc_scan_kernel, dim3(1), dim3(1024), 0, st, d_sums.as<unsigned long long>(), m, nblk, K,
                       (unsigned int)((unsigned long long)h * w), coff, d_bnd.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sc_write_kernel, wgrid, dim3(256), 0, st, planes, units, h, pitch, mode, K, nblk, d_sums.as<unsigned long long>(),
                       d_bnd.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    const dim3 dgrid((unsigned)std::min<unsigned long long>((need + 255) / 256, 1ull << 12));
    hipLaunchKernelGGL(sc_diff_kernel, dgrid, dim3(256), 0, st, d_bnd.as<unsigned int>(), coff, K, d_counts.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    unsigned long long tail[16];                                     // px[8], coff[K + 1]
    AMP_HIP_CHECK(hipMemcpyAsync(tail, px, sizeof(tail), hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long total = tail[8 + K];
    if (total > need) {                                              // cannot happen: every class boundary is a boundary of a named run list
        amp::set_error("amp_seg_class_map: %llu counts on the device, the plan allows %llu", total, need);
        return AMP_ERR_HIP;
    }
    AMP_HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    std::copy(tail, tail + 8, pixels);
    std::copy(tail + 8, tail + 8 + K + 1, counts_off);
    return AMP_OK;
}

}  // namespace

extern "C" int amp_seg_class_map(amp_ctx* ctx, const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                                 const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, int n, int h, int w,
                                 int mode, uint32_t* counts, unsigned long long counts_cap, unsigned long long* counts_off,
                                 unsigned long long* pixels) {
    amp::RunPlan g, p;
    unsigned long long need = 0;
    AMP_TRY_STATUS(amp::seg_class_map_check(gpool, goff, glen, ng, ppool, poff, plen, np, pair_g, pair_p, n, h, w, mode, counts, counts_cap,
                                            counts_off, pixels, g, p, &need));
    return ctx ? seg_class_map_device(ctx, g, p, pair_g, pair_p, n, h, w, mode, need, counts, counts_off, pixels)
               : amp::seg_class_map_host(g, p, pair_g, pair_p, n, h, w, mode, counts, counts_off, pixels);
}
