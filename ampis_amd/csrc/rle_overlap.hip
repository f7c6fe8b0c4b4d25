// All-pairs mask intersection inside groups on the device (ampis/applications/powder.py:80-83: for every satellite of an image
// RLE.merge([satellite, particle], intersect=True) + RLE.area against every particle).  A group is one image: its masks of pool A against its masks
// of pool B, the exact pixel count of a_i AND b_j for every pair, many images in one call.  The masks stay run lists.  The host plan (run_list.h,
// built by the argument checks in mask_analysis_host.hip) keeps per mask the positions [S, E) of its runs of ones, an exclusive prefix P of their
// lengths, the tight box and the area; the work is cut into tiles {mask i of A, 64 consecutive masks j of B of the same group}:
//   ov_pairs_kernel   one wavefront per tile, grid-stride.  Each lane tests the boxes of its pair; a ballot gives the pairs whose boxes meet,
//                     and the whole wave evaluates those one after the other: the lanes stride over the runs [s, e) of the list with FEWER runs
//                     and each takes cover(e) - cover(s) in the other list, where cover(x) = the set pixels below position x = a binary search
//                     in the run ends + the prefix + the part of the run x lies in.  A 64-lane butterfly sum, and the lane that owns the pair
//                     keeps it.  Every lane then stores its pair's count: one coalesced store per tile.
// One launch per call whatever the number of groups.  Integer arithmetic only, no atomic and no memset: every output word is written exactly
// once, by the lane that owns it, so the bytes repeat and equal the host's (mask_analysis_host.hip walks both run lists of a pair instead).  On the
// reference's micrographs the box test leaves under 1 % of the pairs (202 - 285 of 29 000 - 38 000 an image).  Scratch: the plan and the output.
#include <vector>

#include "common.h"
#include "mask_analysis.h"

namespace {

using amp::RunMask;

struct OvTile {
    int a;                        // mask of pool A
    int b0, cnt;                  // masks b0 .. b0 + cnt - 1 of pool B, cnt <= 64
    int pad;
    unsigned long long out;       // where inter[a][b0] lies
};

// the set pixels of a mask below position x.  E: the run ends, ascending; S[n] = 0xffffffff closes the list, P[n] is the area
__device__ __forceinline__ unsigned int ov_cover(const unsigned int* __restrict__ S, const unsigned int* __restrict__ E,
                                                 const unsigned int* __restrict__ P, int n, unsigned int x) {
    const int lo = amp::first_run_ending_after(E, n, x);
    const unsigned int s = S[lo];
    return P[lo] + (s < x ? x - s : 0u);
}

__global__ __launch_bounds__(256) void ov_pairs_kernel(const RunMask* __restrict__ am, const RunMask* __restrict__ bm, const OvTile* __restrict__ tiles,
                                                       int ntiles, const unsigned int* __restrict__ aS, const unsigned int* __restrict__ aE,
                                                       const unsigned int* __restrict__ aP, const unsigned int* __restrict__ bS,
                                                       const unsigned int* __restrict__ bE, const unsigned int* __restrict__ bP,
                                                       unsigned int* __restrict__ inter) {
    const int lane = threadIdx.x & 63;
    const int nwaves = (int)gridDim.x * 4;
    for (int t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); t < ntiles; t += nwaves) {      // uniform over the wave
        const OvTile tl = tiles[t];
        const RunMask A = am[tl.a];
        int bn = 0;
        unsigned int bro = 0;
        bool live = false;
        if (lane < tl.cnt) {
            const RunMask B = bm[tl.b0 + lane];
            bn = B.n; bro = B.ro;
            live = A.n > 0 && B.n > 0 && A.r0 < B.r1 && B.r0 < A.r1 && A.c0 < B.c1 && B.c0 < A.c1;
        }
        unsigned long long todo = __ballot(live);
        unsigned int mine = 0;
        while (todo) {                                               // the same mask in every lane: the wave stays together
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int n = __shfl(bn, l, 64);
            const unsigned int ro = __shfl(bro, l, 64);
            unsigned int sum = 0;
            if (A.n <= n) {
                for (int k = lane; k < A.n; k += 64)
                    sum += ov_cover(bS + ro, bE + ro, bP + ro, n, aE[A.ro + k]) - ov_cover(bS + ro, bE + ro, bP + ro, n, aS[A.ro + k]);
            } else {
                for (int k = lane; k < n; k += 64)
                    sum += ov_cover(aS + A.ro, aE + A.ro, aP + A.ro, A.n, bE[ro + k]) - ov_cover(aS + A.ro, aE + A.ro, aP + A.ro, A.n, bS[ro + k]);
            }
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            if (lane == l) mine = sum;
        }
        if (lane < tl.cnt) inter[tl.out + lane] = mine;
    }
}

static int overlap_groups_device(amp_ctx* ctx, const amp::RunPlan& a, const amp::RunPlan& b, const int* a_first, const int* b_first, int ngroups,
                                 uint32_t* inter) {
    std::vector<OvTile> tiles;
    unsigned long long out = 0;
    for (int g = 0; g < ngroups; ++g) {
        const int nb = b_first[g + 1] - b_first[g];
        for (int i = a_first[g]; i < a_first[g + 1]; ++i, out += (unsigned long long)nb)
            for (int j = 0; j < nb; j += 64) tiles.push_back(OvTile{i, b_first[g] + j, std::min(64, nb - j), 0, out + (unsigned long long)j});
        AMP_REQUIRE(tiles.size() < (1u << 27), "amp_rle_overlap_groups: more than 2^27 tiles of 64 pairs in one call (split the groups over calls)");
    }
    if (out == 0) return AMP_OK;
    const int nt = (int)tiles.size();

    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    amp::DevBuf d_am, d_bm, d_tiles, d_aS, d_aE, d_aP, d_bS, d_bE, d_bP, d_inter;
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_am, a.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_bm, b.m));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_tiles, tiles));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_aS, a.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_aE, a.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_aP, a.P));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_bS, b.S));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_bE, b.E));
    AMP_TRY_STATUS(amp::dev_upload(ctx, d_bP, b.P));
    AMP_TRY_STATUS(amp::dev_alloc(d_inter, (size_t)out * 4));
    const dim3 grid((unsigned)std::min((nt + 3) / 4, 2048));         // 256 CUs x 8 workgroups, the tiles beyond that by stride
    hipLaunchKernelGGL(ov_pairs_kernel, grid, dim3(256), 0, st, d_am.as<RunMask>(), d_bm.as<RunMask>(), d_tiles.as<OvTile>(), nt,
                       d_aS.as<unsigned int>(), d_aE.as<unsigned int>(), d_aP.as<unsigned int>(), d_bS.as<unsigned int>(), d_bE.as<unsigned int>(),
                       d_bP.as<unsigned int>(), d_inter.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    AMP_HIP_CHECK(hipMemcpyAsync(inter, d_inter.p, (size_t)out * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    return AMP_OK;
}

}  // namespace

extern "C" int amp_rle_overlap_groups(amp_ctx* ctx, const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                                      const unsigned long long* boff, const int* blen, const int* a_first, const int* b_first, const int* gh,
                                      const int* gw, int ngroups, uint32_t* inter, size_t inter_cap, unsigned long long* area_a,
                                      unsigned long long* area_b) {
    amp::RunPlan a, b;
    AMP_TRY_STATUS(amp::overlap_groups_check(apool, aoff, alen, bpool, boff, blen, a_first, b_first, gh, gw, ngroups, inter, inter_cap, area_a, area_b,
                                             a, b));
    if (ngroups == 0) return AMP_OK;
    AMP_TRY_STATUS(ctx ? overlap_groups_device(ctx, a, b, a_first, b_first, ngroups, inter)
                       : amp::overlap_groups_host(a, b, a_first, b_first, ngroups, inter));
    for (size_t p = 0; p < a.m.size(); ++p) area_a[p] = a.m[p].area;
    for (size_t p = 0; p < b.m.size(); ++p) area_b[p] = b.m[p].area;
    return AMP_OK;
}
