// amp_flatten_instances on the device: which instance a pixel belongs to when the run-list masks of an image overlap -- the label image of
// owner + 1, per instance the run list of the pixels it owns, and the statistics -- what users compute today with a loop of decoded
// full-image masks (labels[mask_i] = i + 1 in reverse priority, then encode(labels == i + 1) per instance).  The masks stay run lists.  The
// host hands over the plan of run_list.h and the priority order (flatten.h: order[p] = the instance at place p by (rank, index)), so a
// pixel is claimed once, by the first instance in order that covers it.  The launches, whatever n is:
//   1. fl_owner_kernel   one workgroup of one wave per tile of 64 rows x 64 columns, as in render.hip: the lanes box-test 64 instances of the
//                        order at a time and a ballot leaves the hits, walked in order; for a hit lane c builds the 64-row word of its column
//                        (amp::mask_word), claims the bits nothing claimed before in LDS and keeps two words "covered" / "covered twice";
//                        the claimed bits of a hit become the instance's owned pixels and box by one integer atomic add / min / max per
//                        tile and instance; the tile then writes its rows of the int32 label image coalesced (zeros where nothing is);
//   a statistics / label-image call (counts NULL) ends here.  The visible lists are the per-id column-major runs of the label image,
//   exactly what amp_label_runs computes for AMP_LABEL_IDS, so the stages of label_runs_kernels.h run on the device's label image:
//   2. lr_planes_kernel, 3. lr_count_kernel, 4. scan_sums_kernel (the host reads the number of runs), 5. lr_write_kernel (lr_cut),
//   6. lr_keys_kernel, 7. rocprim::radix_sort_pairs (stable; its own launches depend on the number of runs only), 8. lr_heads_kernel,
//   9. scan_sums_kernel (lr_group; the host reads the owners and the counts, reports the need and refuses a capacity that is too small),
//  10. lr_emit_kernel (lr_emit);
//  11. fl_diff_kernel    one lane per count of the result, all n instances back to back: boundary minus the boundary before it, or the single
//                        run h * w of an instance that owns nothing.
// LDS: the owner of pixel (r, c) of the tile at c * 65 + r -- a lane walks its own column, the odd dword stride keeps the lanes on distinct
// banks when the rows are read back.  Integer arithmetic only; the atomics are integer add / min / max, whose results do not depend on
// their order, and nothing is placed through a counter.  So the bytes repeat and equal the host's (flatten_host.hip).  Every loop in a
// kernel states why it ends; none waits for another lane.
#include <string.h>

#include <vector>

#include "common.h"
#include "flatten.h"
#include "label_runs_kernels.h"
#include "mask_analysis.h"

namespace {

using amp::RunMask;
using amp::wave_sum;

constexpr int FL_STRIDE = 65;                     // dwords of one tile column in LDS: 64 rows + 1

// OR over the 64 lanes, valid in lane 0
__device__ __forceinline__ u64 fl_wave_or(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_down(v, o, 64);                         // ends: six steps
    return v;
}

// owned [n]: pixels owned; mins / maxs [n][2]: {r0, c0} / {r1, c1} of the owned pixels, preset to a large value / 0; covered [2]: the pixels
// covered once / twice or more
__global__ __launch_bounds__(64) void fl_owner_kernel(int* __restrict__ labels, int h, int w, int tiles_x, const RunMask* __restrict__ rm,
                                                      const unsigned int* __restrict__ S, const unsigned int* __restrict__ E,
                                                      const int* __restrict__ order, int n, unsigned long long* __restrict__ owned,
                                                      int* __restrict__ mins, int* __restrict__ maxs, unsigned long long* __restrict__ covered) {
    __shared__ int own[64 * FL_STRIDE];
    const int lane = threadIdx.x;
    const int row0 = (int)(blockIdx.x / (unsigned)tiles_x) << 6, col0 = (int)(blockIdx.x % (unsigned)tiles_x) << 6;
    const int rows = min(64, h - row0), cols = min(64, w - col0), col = col0 + lane;
    for (int q = lane; q < 64 * FL_STRIDE; q += 64) own[q] = 0;                          // ends: q grows to the array's size
    __syncthreads();
    int* mine = own + lane * FL_STRIDE;
    u64 once = 0, twice = 0;                      // of this lane's column: covered at all (= claimed), covered by two or more
    for (int base = 0; base < n; base += 64) {                                           // ends: base grows to n; uniform over the wave
        const int p = base + lane;
        int i = 0;
        bool hit = false;
        if (p < n) {
            i = order[p];
            const RunMask k = rm[i];
            hit = k.n > 0 && k.r0 < row0 + rows && k.r1 > row0 && k.c0 < col0 + cols && k.c1 > col0;
        }
        for (u64 any = __ballot(hit); any; any &= any - 1) {                             // ends: one set bit fewer each time; uniform over the wave
            const int ii = __shfl(i, amp::ctz(any), 64);
            const RunMask k = rm[ii];
            u64 m = 0;
            if (lane < cols && col >= k.c0 && col < k.c1) {
                const unsigned int cb = (unsigned)col * (unsigned)h, a = cb + (unsigned)row0;
                m = amp::mask_word(S + k.ro, E + k.ro, k.n, a, min(a + 64u, cb + (unsigned)h));
            }
            const u64 fresh = m & ~once;
            twice |= once & m;
            once |= m;
            for (u64 x = fresh; x; x &= x - 1) mine[amp::ctz(x)] = ii + 1;               // ends: one set bit fewer each time
            const u64 fcols = __ballot(fresh != 0);
            if (!fcols) continue;                                                        // uniform: the tile's part of the mask lies under others
            const u64 frows = fl_wave_or(fresh), cnt = wave_sum((u64)amp::popc(fresh));
            if (lane == 0) {
                atomicAdd(&owned[ii], cnt);
                atomicMin(&mins[2 * (size_t)ii], row0 + amp::ctz(frows));
                atomicMax(&maxs[2 * (size_t)ii], row0 + 64 - amp::clz(frows));
                atomicMin(&mins[2 * (size_t)ii + 1], col0 + amp::ctz(fcols));
                atomicMax(&maxs[2 * (size_t)ii + 1], col0 + 64 - amp::clz(fcols));
            }
        }
    }
    __syncthreads();                                                                     // the columns are complete before the rows are read
    if (lane < cols)
        for (int r = 0; r < rows; ++r) labels[(size_t)(row0 + r) * w + col] = own[lane * FL_STRIDE + r];      // ends: r grows to rows
    const u64 c1 = wave_sum((u64)amp::popc(once & ~twice)), c2 = wave_sum((u64)amp::popc(twice));
    if (lane == 0 && (c1 | c2)) { atomicAdd(&covered[0], c1); atomicAdd(&covered[1], c2); }
}

// count t of the result belongs to instance i = the owner of t among foff [n] (every instance has a count); src[i] = where the instance's
// boundaries start in bnd, ~0 for an instance that owns nothing: the single run `area`
__global__ __launch_bounds__(256) void fl_diff_kernel(const unsigned int* __restrict__ bnd, const unsigned long long* __restrict__ foff,
                                                      const unsigned long long* __restrict__ src, int n, unsigned long long total,
                                                      unsigned int area, unsigned int* __restrict__ counts) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * 256) {   // ends: t grows by the grid
        const int i = amp::owner_of(foff, n, t);                                         // foff[0] = 0 <= t
        if (src[i] == ~0ull) { counts[t] = area; continue; }
        const unsigned long long s = src[i] + (t - foff[i]);
        counts[t] = bnd[s] - (t == foff[i] ? 0u : bnd[s - 1]);
    }
}

int flatten_device(amp_ctx* ctx, const amp::RunPlan& runs, const std::vector<int>& order, int h, int w, int* labels, uint32_t* counts,
                   unsigned long long counts_cap, unsigned long long* counts_off, int* counts_len, unsigned long long* stats, int* boxes,
                   unsigned long long* pixels, unsigned long long* need) {
    const int n = (int)runs.m.size();
    const unsigned long long image = (unsigned long long)h * w;
    const unsigned int area = (unsigned int)image;
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    amp::DevBuf d_rm, d_S, d_E, d_order, d_labels, d_owned, d_mins, d_maxs, d_cov;
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_rm, runs.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_S, runs.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_E, runs.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_order, order));
    AMP_TRY_STATUS(amp::dev_alloc(d_labels, (size_t)image * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_owned, (size_t)n * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_mins, (size_t)n * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_maxs, (size_t)n * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_cov, 16));
    AMP_HIP_CHECK(hipMemsetAsync(d_owned.p, 0, (size_t)n * 8, st));
    AMP_HIP_CHECK(hipMemsetAsync(d_mins.p, 0x7f, (size_t)n * 8, st));                    // 0x7f7f7f7f: above every row and column
    AMP_HIP_CHECK(hipMemsetAsync(d_maxs.p, 0, (size_t)n * 8, st));
    AMP_HIP_CHECK(hipMemsetAsync(d_cov.p, 0, 16, st));
    const int tiles_x = (w + 63) >> 6, tiles_y = (h + 63) >> 6;                          // at most 2^24 tiles: h * w <= 2^30
    hipLaunchKernelGGL(fl_owner_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(64), 0, st, d_labels.as<int>(), h, w, tiles_x,
                       d_rm.as<RunMask>(), d_S.as<unsigned int>(), d_E.as<unsigned int>(), d_order.as<int>(), n, d_owned.as<unsigned long long>(),
                       d_mins.as<int>(), d_maxs.as<int>(), d_cov.as<unsigned long long>());
    AMP_HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> owned((size_t)n), cov(2);
    std::vector<int> mins(2 * (size_t)n), maxs(2 * (size_t)n);
    AMP_HIP_CHECK(hipMemcpyAsync(cov.data(), d_cov.p, 16, hipMemcpyDeviceToHost, st));
    if (n) {
        AMP_HIP_CHECK(hipMemcpyAsync(owned.data(), d_owned.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipMemcpyAsync(mins.data(), d_mins.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipMemcpyAsync(maxs.data(), d_maxs.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    // everything but the lists: written once nothing can be refused any more
    auto finish = [&]() -> int {
        if (labels) AMP_HIP_CHECK(hipMemcpyAsync(labels, d_labels.p, (size_t)image * 4, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipStreamSynchronize(st));
        for (size_t i = 0; i < (size_t)n; ++i) {
            stats[2 * i] = runs.m[i].area;
            stats[2 * i + 1] = owned[i];
            const bool any = owned[i] != 0;
            boxes[4 * i] = any ? mins[2 * i] : 0; boxes[4 * i + 1] = any ? mins[2 * i + 1] : 0;
            boxes[4 * i + 2] = any ? maxs[2 * i] : 0; boxes[4 * i + 3] = any ? maxs[2 * i + 1] : 0;
        }
        pixels[0] = image - cov[0] - cov[1]; pixels[1] = cov[0]; pixels[2] = cov[1];
        return AMP_OK;
    };
    if (!counts) return finish();

    // the runs of the label image, by the stages of amp_label_runs
    LrStages g;
    AMP_TRY_STATUS(lr_cut("amp_flatten_instances", st, d_labels.p, h, w, (int)AMP_LABEL_IDS, 1, g));
    std::vector<unsigned long long> foff((size_t)n), src((size_t)n, ~0ull);
    unsigned long long total = (unsigned long long)n;               // nothing is owned: the single run h * w for every instance
    amp::DevBuf d_foff, d_src, d_counts;
    if (g.R) {
        const unsigned int R = g.R;
        AMP_TRY_STATUS(lr_group(st, nullptr, nullptr, g));
        const unsigned long long N = g.N, listed = g.listed;
        if (N == 0 || N > (unsigned long long)n || listed < 2 * N || listed > 3ull * R) {            // cannot happen: an owner is one of the n instances
            amp::set_error("amp_flatten_instances: %llu owners and %llu counts from %u runs of %d instances on the device", N, listed, R, n);
            return AMP_ERR_HIP;
        }
        total = listed + ((unsigned long long)n - N);
        AMP_TRY_STATUS(amp::flatten_capacity(total, counts_cap, need));
        AMP_TRY_STATUS(lr_emit(st, g));
        std::vector<int> ids((size_t)N);
        std::vector<unsigned long long> off((size_t)N);
        AMP_HIP_CHECK(hipMemcpyAsync(ids.data(), g.ids.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipMemcpyAsync(off.data(), g.off.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
        AMP_HIP_CHECK(hipStreamSynchronize(st));
        for (size_t k = 0; k < (size_t)N; ++k) {                     // the owners come in ascending id order
            if (ids[k] < 1 || ids[k] > n || off[k] >= listed || (k && ids[k] <= ids[k - 1])) {       // cannot happen
                amp::set_error("amp_flatten_instances: owner %d at place %zu of %llu on the device", ids[k], k, N);
                return AMP_ERR_HIP;
            }
            src[(size_t)ids[k] - 1] = off[k];
        }
        unsigned long long at = 0;
        for (size_t i = 0, k = 0; i < (size_t)n; ++i) {
            foff[i] = at;
            if (src[i] == ~0ull) { at += 1; continue; }
            at += (k + 1 < (size_t)N ? off[k + 1] : listed) - off[k];
            ++k;
        }
        if (at != total) {                                           // cannot happen
            amp::set_error("amp_flatten_instances: %llu counts laid out, %llu expected", at, total);
            return AMP_ERR_HIP;
        }
    } else {
        AMP_TRY_STATUS(amp::flatten_capacity(total, counts_cap, need));
        for (size_t i = 0; i < (size_t)n; ++i) foff[i] = i;
    }
    if (n) {
        AMP_TRY_STATUS(amp::dev_upload(ctx, d_foff, foff));
        AMP_TRY_STATUS(amp::dev_upload(ctx, d_src, src));
        AMP_TRY_STATUS(amp::dev_alloc(d_counts, (size_t)total * 4));
        hipLaunchKernelGGL(fl_diff_kernel, grid_256(total), dim3(256), 0, st, g.bnd.as<unsigned int>(), d_foff.as<unsigned long long>(),
                           d_src.as<unsigned long long>(), n, total, area, d_counts.as<unsigned int>());
        AMP_HIP_CHECK(hipGetLastError());
        AMP_HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    }
    AMP_TRY_STATUS(finish());
    for (size_t i = 0; i < (size_t)n; ++i) {
        counts_off[i] = foff[i];
        counts_len[i] = (int)((i + 1 < (size_t)n ? foff[i + 1] : total) - foff[i]);
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_flatten_instances(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                                     const uint32_t* rank, int* labels, uint32_t* counts, unsigned long long counts_cap,
                                     unsigned long long* counts_off, int* counts_len, unsigned long long* stats, int* boxes,
                                     unsigned long long* pixels, unsigned long long* need) {
    amp::RunPlan plan;
    std::vector<int> order;
    AMP_TRY_STATUS(amp::flatten_check(pool, off, len, n, h, w, rank, counts, counts_cap, counts_off, counts_len, stats, boxes, pixels, need, plan,
                                      order));
    return ctx ? flatten_device(ctx, plan, order, h, w, labels, counts, counts_cap, counts_off, counts_len, stats, boxes, pixels, need)
               : amp::flatten_host(plan, order, h, w, labels, counts, counts_cap, counts_off, counts_len, stats, boxes, pixels, need);
}
