// mask_edge_distance on the device (ampis/analyze.py:416-499, the one place where AMPIS itself reaches for a GPU): for every matched
// (ground truth, prediction) pair, the squared distance of each false-positive pixel to the nearest ground-truth pixel of the pair's crop and of
// each false-negative pixel to the nearest predicted pixel.  The reference broadcasts [queries x targets x 2] doubles per pair; here
//   1. ed_decode_kernel   decodes both run lists of every pair into bit planes of the crop.  The planes are COLUMN-major like the runs (64 rows a
//                         word): a run is a few word-wide ORs, where a row-major plane would cost one atomic per pixel.  The search below is
//                         symmetric in rows and columns, so it walks columns; only the OUTPUT order is row-major, and steps 2-4 produce it;
//   2. ed_rows_kernel<0>  counts the query pixels of every crop row (one lane per row, 64 rows of a word per wave);
//   3. ed_scan_kernel     turns the counts into output offsets (one workgroup, a fixed tree: no atomics, so the order is the contract's and
//                         the bytes repeat) and picks the per-pair offsets out of them;
//   4. ed_rows_kernel<1>  writes every query's (row, column) into its output slot;
//   5. ed_search_kernel   one lane per query: replaces the coordinates by the squared distance.  It walks the columns outwards from the
//                         query's own, finds the nearest set bit of each with word scans and stops when the column offset squared reaches the
//                         best so far -- exact, a few columns for the boundary band of matched masks, O(crop width) for a far pixel.
// Five launches and one memset per call whatever the number of pairs; scratch is two bit planes and two 8-byte words per crop row.  Integer
// arithmetic only: h, w <= 32768 keeps every squared distance below 2^31.  Work is cut into host-built tile lists -- (pair, mask, 256 runs of
// ones) for the decoder, (pair, 64 rows) for the row kernels -- so a full-image crop spreads over the chip like three hundred small ones.  The
// runs come from the plan the argument checks build (run_list.h, mask_analysis_host.hip); the painter and the scan are run_list.h's, the
// chunked scan of an array in one workgroup is compaction.h's.
#include <vector>

#include "common.h"
#include "compaction.h"
#include "mask_analysis.h"

namespace {

struct EdPair {
    int H, W;                     // the crop
    int r1, c1;                   // its origin in the image
    int pitch;                    // 64-bit words per plane column = ceil(H / 64)
    int tile0;                    // first row tile of the pair (== the next pair's when the crop is empty)
    int gn, pn;                   // runs of ones of the two masks
    unsigned int gro, pro;        // where they start in the plan's S / E
    unsigned long long plane;     // word offset of the ground-truth plane; the prediction's follows it (W * pitch words each)
};

// tile = {2 * pair + mask, first run of ones}: thread t takes run first + t
__global__ __launch_bounds__(256) void ed_decode_kernel(const EdPair* __restrict__ pairs, const int2* __restrict__ tiles, int ntiles,
                                                        const unsigned int* __restrict__ S, const unsigned int* __restrict__ E,
                                                        unsigned long long* __restrict__ planes, int h) {
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int2 tl = tiles[t];
        const EdPair pr = pairs[tl.x >> 1];
        const int side = tl.x & 1;
        const int k = tl.y + (int)threadIdx.x;
        if (k >= (side ? pr.pn : pr.gn)) continue;
        const unsigned int at = (side ? pr.pro : pr.gro) + (unsigned)k;
        unsigned long long* plane = planes + pr.plane + (side ? (unsigned long long)pr.W * pr.pitch : 0ull);
        amp::paint_run<true>(S[at], E[at], h, plane, pr.r1, pr.c1, pr.H, pr.W, pr.pitch, amp::OrAtomic());
    }
}

// tile = {pair, first row (a multiple of 64)}: one wave per tile, lane = row.  rows[0] / rows[1]: [ntiles * 64] counts (WRITE = 0, written) or
// output offsets (WRITE = 1, read) of the false-positive / false-negative queries; out_fp / out_fn: (row << 16 | column) of every query.
template <bool WRITE>
__global__ __launch_bounds__(256) void ed_rows_kernel(const EdPair* __restrict__ pairs, const int2* __restrict__ tiles, int ntiles,
                                                      const unsigned long long* __restrict__ planes, unsigned long long* __restrict__ rows_fp,
                                                      unsigned long long* __restrict__ rows_fn, unsigned int* __restrict__ out_fp,
                                                      unsigned int* __restrict__ out_fn) {
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * 4) {
        const int2 tl = tiles[t];
        const EdPair pr = pairs[tl.x];
        const unsigned long long* G = planes + pr.plane + (tl.y >> 6);
        const unsigned long long* P = G + (size_t)pr.W * pr.pitch;
        const size_t slot = (size_t)t * 64 + lane;
        const unsigned int rbits = (unsigned)(tl.y + lane) << 16;
        unsigned long long nfp = WRITE ? rows_fp[slot] : 0ull, nfn = WRITE ? rows_fn[slot] : 0ull;
        for (int c = 0; c < pr.W; ++c) {
            const unsigned long long g = G[(size_t)c * pr.pitch], p = P[(size_t)c * pr.pitch];   // bits past the crop's last row are never set
            const bool fp = ((p & ~g) >> lane) & 1ull, fn = ((g & ~p) >> lane) & 1ull;
            if (WRITE) {
                if (fp) out_fp[nfp] = rbits | (unsigned)c;
                if (fn) out_fn[nfn] = rbits | (unsigned)c;
            }
            nfp += fp;
            nfn += fn;
        }
        if (!WRITE) { rows_fp[slot] = nfp; rows_fn[slot] = nfn; }
    }
}

// exclusive scan of the row counts in place (one workgroup: each thread sums a contiguous chunk, the chunk sums are scanned in LDS), then
// off[p] = the offset of pair p's first row, off[n] = the total
__global__ __launch_bounds__(1024) void ed_scan_kernel(unsigned long long* rows_fp, unsigned long long* rows_fn, long long nrows,
                                                       const EdPair* __restrict__ pairs, int n, int ntiles, unsigned long long* __restrict__ off_fp,
                                                       unsigned long long* __restrict__ off_fn) {
    __shared__ unsigned long long s[1024];
    const int tid = threadIdx.x;
    const auto nothing = [](unsigned long long, unsigned long long) {};
    scan_sums_in_place(rows_fp, (unsigned long long)nrows, s, nothing);
    const unsigned long long ta = s[1023];
    __syncthreads();                                                 // s is read before the second scan writes it
    scan_sums_in_place(rows_fn, (unsigned long long)nrows, s, nothing);
    const unsigned long long tb = s[1023];
    __syncthreads();
    for (int p = tid; p <= n; p += 1024) {
        const int t0 = p < n ? pairs[p].tile0 : ntiles;
        off_fp[p] = t0 < ntiles ? rows_fp[(size_t)t0 * 64] : ta;
        off_fn[p] = t0 < ntiles ? rows_fn[(size_t)t0 * 64] : tb;
    }
}

// nearest set bit of one plane column to row r, as a squared distance with the column's own d2c added; `best` bounds the walk
__device__ __forceinline__ unsigned int ed_column(const unsigned long long* __restrict__ col, int pitch, int r, unsigned int d2c, unsigned int best) {
    const int w0 = r >> 6, b = r & 63;
    const unsigned long long x = col[w0];
    const unsigned long long below = b == 63 ? ~0ull : ((2ull << b) - 1ull);                    // bits 0 .. b: rows up to and including r
    unsigned long long y = x & below;
    if (y) {
        const unsigned int dr = (unsigned)(b - (63 - __clzll((long long)y)));
        best = min(best, dr * dr + d2c);
    } else {
        unsigned int lb = (unsigned)b + 1u;                                                     // distance to the top row of the word above
        for (int wv = w0 - 1; wv >= 0 && lb * lb + d2c < best; --wv, lb += 64u) {
            y = col[wv];
            if (y) { const unsigned int dr = lb + (unsigned)__clzll((long long)y); best = min(best, dr * dr + d2c); break; }
        }
    }
    y = x & ~below;
    if (y) {
        const unsigned int dr = (unsigned)(__ffsll((long long)y) - 1 - b);
        best = min(best, dr * dr + d2c);
    } else {
        unsigned int lb = 64u - (unsigned)b;                                                    // distance to the first row of the word below
        for (int wv = w0 + 1; wv < pitch && lb * lb + d2c < best; ++wv, lb += 64u) {
            y = col[wv];
            if (y) { const unsigned int dr = lb + (unsigned)(__ffsll((long long)y) - 1); best = min(best, dr * dr + d2c); break; }
        }
    }
    return best;
}

// out: the false-positive queries [0, tot_fp), then the false-negative ones [tot_fp, tot): coordinates in, squared distances out
// (0xffffffff where the target mask has no pixel in the crop)
__global__ __launch_bounds__(256) void ed_search_kernel(const EdPair* __restrict__ pairs, int n, const unsigned long long* __restrict__ planes,
                                                        const unsigned long long* __restrict__ off_fp, const unsigned long long* __restrict__ off_fn,
                                                        unsigned long long tot_fp, unsigned long long tot, unsigned int* __restrict__ out) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < tot; q += (unsigned long long)gridDim.x * 256) {
        const bool side = q >= tot_fp;
        const unsigned long long i = side ? q - tot_fp : q;
        const unsigned long long* off = side ? off_fn : off_fp;
        const EdPair pr = pairs[amp::owner_of(off, n, i)];
        const unsigned long long* T = planes + pr.plane + (side ? (unsigned long long)pr.W * pr.pitch : 0ull);    // false negatives look for the prediction
        const unsigned int rc = out[q];
        const int r = (int)(rc >> 16), c = (int)(rc & 0xffffu);
        unsigned int best = 0xffffffffu;
        for (int dc = 0; (unsigned)(dc * dc) < best && (c - dc >= 0 || c + dc < pr.W); ++dc) {
            const unsigned int d2c = (unsigned)(dc * dc);
            if (c - dc >= 0) best = ed_column(T + (size_t)(c - dc) * pr.pitch, pr.pitch, r, d2c, best);
            if (dc > 0 && c + dc < pr.W) best = ed_column(T + (size_t)(c + dc) * pr.pitch, pr.pitch, r, d2c, best);
        }
        out[q] = best;
    }
}

static int edge_distance_device(amp_ctx* ctx, const amp::RunPlan& runs, int ng, const int* pair_g, const int* pair_p, const int* crop, int n, int h,
                                uint32_t* fp_d2, unsigned long long fp_cap, unsigned long long* fp_off, uint32_t* fn_d2, unsigned long long fn_cap,
                                unsigned long long* fn_off) {
    // pair records, decode and row tiles
    std::vector<EdPair> pairs((size_t)n);
    std::vector<int2> dtiles, rtiles;
    unsigned long long words = 0;
    for (int p = 0; p < n; ++p) {
        const amp::RunMask &G = runs.m[(size_t)pair_g[p]], &Q = runs.m[(size_t)ng + pair_p[p]];
        const int* cr = crop + 4 * (size_t)p;
        EdPair& e = pairs[(size_t)p];
        e.H = cr[1] - cr[0]; e.W = cr[3] - cr[2]; e.r1 = cr[0]; e.c1 = cr[2];
        e.pitch = (e.H + 63) >> 6;
        e.tile0 = (int)rtiles.size();
        e.gn = G.n; e.pn = Q.n; e.gro = G.ro; e.pro = Q.ro;
        e.plane = words;
        if (e.H == 0 || e.W == 0) { e.H = e.W = e.pitch = 0; continue; }         // an empty crop has no pixel, no tile and no plane
        words += 2ull * (unsigned long long)e.W * e.pitch;
        for (int k = 0; k < e.gn; k += 256) dtiles.push_back(make_int2(2 * p, k));
        for (int k = 0; k < e.pn; k += 256) dtiles.push_back(make_int2(2 * p + 1, k));
        for (int r = 0; r < e.H; r += 64) rtiles.push_back(make_int2(p, r));
        AMP_REQUIRE(rtiles.size() < (1u << 25) && dtiles.size() < (1u << 30), "amp_mask_edge_distance: the crops of one call have more than 2^31 rows");
    }
    const int ndt = (int)dtiles.size(), nrt = (int)rtiles.size();
    const long long nrows = (long long)nrt * 64;

    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_pairs, d_dt, d_rt, d_S, d_E, d_planes, d_rows, d_off, d_out;
    std::vector<unsigned long long> off((size_t)2 * (n + 1), 0);
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_pairs, pairs));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_dt, dtiles));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_rt, rtiles));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_S, runs.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_E, runs.E));
    AMP_TRY_STATUS(amp::dev_alloc(d_planes, words * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_rows, (size_t)nrows * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_off, off.size() * 8));
    unsigned long long* rows_fp = d_rows.as<unsigned long long>();
    unsigned long long* rows_fn = rows_fp + nrows;
    unsigned long long* off_fp = d_off.as<unsigned long long>();
    unsigned long long* off_fn = off_fp + (n + 1);
    if (words) AMP_HIP_CHECK(hipMemsetAsync(d_planes.p, 0, words * 8, st));
    if (ndt) {
        hipLaunchKernelGGL(ed_decode_kernel, dim3((unsigned)std::min(ndt, 1 << 20)), dim3(256), 0, st, d_pairs.as<EdPair>(), d_dt.as<int2>(), ndt,
                           d_S.as<unsigned int>(), d_E.as<unsigned int>(), d_planes.as<unsigned long long>(), h);
        AMP_HIP_CHECK(hipGetLastError());
    }
    const unsigned rblocks = (unsigned)std::min(amp::cdiv(std::max(nrt, 1), 4), 1 << 20);
    if (nrt) {
        hipLaunchKernelGGL(ed_rows_kernel<false>, dim3(rblocks), dim3(256), 0, st, d_pairs.as<EdPair>(), d_rt.as<int2>(), nrt,
                           d_planes.as<unsigned long long>(), rows_fp, rows_fn, (unsigned int*)nullptr, (unsigned int*)nullptr);
        AMP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ed_scan_kernel, dim3(1), dim3(1024), 0, st, rows_fp, rows_fn, nrows, d_pairs.as<EdPair>(), n, nrt, off_fp, off_fn);
    AMP_HIP_CHECK(hipGetLastError());
    AMP_HIP_CHECK(hipMemcpyAsync(off.data(), d_off.p, off.size() * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long tot_fp = off[(size_t)n], tot_fn = off[(size_t)2 * n + 1], tot = tot_fp + tot_fn;
    if (tot_fp > fp_cap || tot_fn > fn_cap) {                        // nothing has been written to the caller's arrays
        amp::set_error("amp_mask_edge_distance: %llu false-positive and %llu false-negative pixels, capacities %llu and %llu", tot_fp, tot_fn, fp_cap, fn_cap);
        return AMP_ERR_NOMEM;
    }
    if (tot) {
        AMP_TRY_STATUS(amp::dev_alloc(d_out, (size_t)tot * 4));
        unsigned int* out = d_out.as<unsigned int>();
        hipLaunchKernelGGL(ed_rows_kernel<true>, dim3(rblocks), dim3(256), 0, st, d_pairs.as<EdPair>(), d_rt.as<int2>(), nrt,
                           d_planes.as<unsigned long long>(), rows_fp, rows_fn, out, out + tot_fp);
        AMP_HIP_CHECK(hipGetLastError());
        const unsigned sblocks = (unsigned)std::min<unsigned long long>((tot + 255) / 256, 1ull << 20);
        hipLaunchKernelGGL(ed_search_kernel, dim3(sblocks), dim3(256), 0, st, d_pairs.as<EdPair>(), n, d_planes.as<unsigned long long>(), off_fp, off_fn,
                           tot_fp, tot, out);
        AMP_HIP_CHECK(hipGetLastError());
        if (tot_fp) AMP_HIP_CHECK(hipMemcpyAsync(fp_d2, out, (size_t)tot_fp * 4, hipMemcpyDeviceToHost, st));
        if (tot_fn) AMP_HIP_CHECK(hipMemcpyAsync(fn_d2, out + tot_fp, (size_t)tot_fn * 4, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipStreamSynchronize(st));
    }
    std::copy(off.begin(), off.begin() + (n + 1), fp_off);
    std::copy(off.begin() + (n + 1), off.end(), fn_off);
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_edge_distance(amp_ctx* ctx, const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng,
                                      const uint32_t* ppool, const unsigned long long* poff, const int* plen, int np, const int* pair_g,
                                      const int* pair_p, const int* box, int n, int h, int w, uint32_t* fp_d2, unsigned long long fp_cap,
                                      unsigned long long* fp_off, uint32_t* fn_d2, unsigned long long fn_cap, unsigned long long* fn_off) {
    std::vector<int> crop;
    amp::RunPlan runs;
    AMP_TRY_STATUS(amp::edge_distance_check(gpool, goff, glen, ng, ppool, poff, plen, np, pair_g, pair_p, box, n, h, w, fp_d2, fp_cap, fp_off, fn_d2,
                                            fn_cap, fn_off, crop, runs));
    if (n == 0) { fp_off[0] = fn_off[0] = 0; return AMP_OK; }
    return ctx ? edge_distance_device(ctx, runs, ng, pair_g, pair_p, crop.data(), n, h, fp_d2, fp_cap, fp_off, fn_d2, fn_cap, fn_off)
               : amp::edge_distance_host(runs, ng, pair_g, pair_p, crop.data(), n, h, fp_d2, fp_cap, fp_off, fn_d2, fn_cap, fn_off);
}
