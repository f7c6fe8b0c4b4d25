// amp_mask_contours on the device: the boundary rings of every mask of a pool in one call, as corner lists on pixel corners -- what users get from
// cv2.findContours / detectron2's GenericMask.mask_to_polygons on one decoded full-image array per mask, here as exact crack rings.  The masks
// stay run lists: the host cuts the plan into the colour-1 items of mask_parts.h, two NODES an item (contours.h: its top edge heading east, its
// bottom edge heading west).  The successor function of contours.h is a permutation of the live nodes of a mask; its cycles are the rings.
// The launches, with K = ceil(log2(the most nodes of any one mask)) fixed on the host (a ring lies within one mask):
//   1. ct_succ_kernel     one lane per node: its successor by binary searches in its own and the neighbouring column (no walk), the two
//                         corners of its turn if it is no straight step; the turns counted;
//   2. ct_min_kernel x K  pointer jumping, one buffer read and the other written each round: after round r a node knows the smallest node
//                         among the 2^r that follow it, after K rounds its ring's LEADER;
//   3. ct_link_kernel     the ring cut open in front of its leader: every node starts a list {next, nodes, turns} for the second jumping;
//                         per leader the smallest corner by (x, y) with the node that owns it (64-bit atomic min), twice the area and the
//                         vertical length (64-bit atomic adds); the leaders counted.  The host reads the two counts, reports the need and
//                         refuses capacities that are too small;
//   4. ct_rank_kernel x K pointer jumping again: the nodes and the turns from a node to the end of its list, so its place behind the leader;
//   5. ct_keys_kernel     one 64-bit key per node: (mask, smallest corner) for a leader, all ones for every other node;
//   6. rocprim::radix_sort_pairs over the nodes (its own launches depend on the number of nodes only): the rings in their final order first;
//   7. ct_rings_kernel    one lane per ring: corners, area2, length, its mask, the place of the smallest corner in the walk from the leader;
//   8. rocprim::exclusive_scan of the corner counts: where every ring starts;
//   9. ct_write_kernel    one lane per node: its two corners at their place, the ring turned so that the smallest corner comes first.
// Integer arithmetic only.  The atomics are integer min and add, nothing is placed through a counter, so the bytes repeat and equal the host's
// (contours_host.hip).  Every loop in a kernel states why it ends; none waits for another lane.  No dense mask, no bit plane.
#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "contours.h"
#include "mask_parts_dev.h"

namespace {

using amp::u64;
using amp::wave_sum;

struct CtArgs : amp::MpItemsView {
    int h, k;
    unsigned int N;                              // nodes: two an item
};

#define CT_END 0xffffffffu

// stp[v] = {x, y0, y1, turn}; jump[v] = {smallest node so far, the node 2^r steps on}; totals[0] += the turns
__global__ __launch_bounds__(256) void ct_succ_kernel(CtArgs g, unsigned int* __restrict__ succ, int4* __restrict__ stp, uint2* __restrict__ jump,
                                                      unsigned long long* __restrict__ ringmin, unsigned long long* __restrict__ area,
                                                      unsigned long long* __restrict__ vlen, unsigned long long* __restrict__ totals) {
    const unsigned int v = blockIdx.x * 256 + threadIdx.x;                               // the grid covers the nodes once: N < 2^30
    unsigned int turn = 0;
    if (v < g.N) {
        unsigned int nx = v;
        int4 s = make_int4(0, 0, 0, 0);
        if (g.T[v >> 1] != amp::MP_END) {
            const amp::CtStep st = amp::ct_successor(g.S, g.E, g.col, g.masks[amp::owner_of(g.first, g.n, (u64)(v >> 1))], g.h, g.k, v);
            nx = st.next;
            s = make_int4(st.x, st.y0, st.y1, st.turn);
            turn = (unsigned)st.turn;
        }
        succ[v] = nx; stp[v] = s; jump[v] = make_uint2(v, nx);
        ringmin[v] = ~0ull; area[v] = 0ull; vlen[v] = 0ull;
    }
    const u64 t = wave_sum((u64)turn);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(&totals[0], t);
}

__global__ __launch_bounds__(256) void ct_min_kernel(unsigned int N, const uint2* __restrict__ in, uint2* __restrict__ out) {
    const unsigned int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const uint2 a = in[v], b = in[a.y];                                                  // a.y < N: a successor is a node of the same mask
    out[v] = make_uint2(min(a.x, b.x), b.y);
}

// list[v] = {the next node or CT_END in front of the leader, nodes from v to the end, turns from v to the end, -}; totals[1] += the leaders
__global__ __launch_bounds__(256) void ct_link_kernel(CtArgs g, const unsigned int* __restrict__ succ, const int4* __restrict__ stp,
                                                      const uint2* __restrict__ jump, uint4* __restrict__ list,
                                                      unsigned long long* __restrict__ ringmin, unsigned long long* __restrict__ area,
                                                      unsigned long long* __restrict__ vlen, unsigned long long* __restrict__ totals) {
    const unsigned int v = blockIdx.x * 256 + threadIdx.x;
    unsigned int leads = 0;
    if (v < g.N) {
        const unsigned int l = jump[v].x, nx = succ[v];
        const int4 s = stp[v];
        list[v] = make_uint4(nx == l ? CT_END : nx, 1u, (unsigned)s.w, 0u);
        if (s.w) {
            const amp::CtStep st{nx, 1, s.x, s.y, s.z};
            const u64 k0 = ((u64)amp::ct_key(s.x, s.y) << 32) | (u64)(2u * v), k1 = ((u64)amp::ct_key(s.x, s.z) << 32) | (u64)(2u * v + 1u);
            atomicMin(&ringmin[l], k0 < k1 ? k0 : k1);
            atomicAdd(&area[l], (unsigned long long)amp::ct_area2(st));                  // two's complement: the sum is the signed sum
            atomicAdd(&vlen[l], (unsigned long long)amp::ct_vlen(st));
        }
        leads = l == v && g.T[v >> 1] != amp::MP_END;
    }
    const u64 t = wave_sum((u64)leads);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(&totals[1], t);
}

__global__ __launch_bounds__(256) void ct_rank_kernel(unsigned int N, const uint4* __restrict__ in, uint4* __restrict__ out) {
    const unsigned int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    uint4 a = in[v];
    if (a.x != CT_END) {
        const uint4 b = in[a.x];
        a.x = b.x; a.y += b.y; a.z += b.z;
    }
    out[v] = a;
}

__global__ __launch_bounds__(256) void ct_keys_kernel(CtArgs g, const uint2* __restrict__ jump, const unsigned long long* __restrict__ ringmin,
                                                      unsigned long long* __restrict__ keys, unsigned int* __restrict__ vals) {
    const unsigned int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.N) return;
    const bool leads = jump[v].x == v && g.T[v >> 1] != amp::MP_END;
    keys[v] = leads ? ((u64)amp::owner_of(g.first, g.n, (u64)(v >> 1)) << 32) | (ringmin[v] >> 32) : ~0ull;
    vals[v] = v;
}

struct CtRings {
    unsigned long long* corners;                 // [rings] for the scan
    int* len;
    long long *area2, *length;
    int* mask;
    unsigned int* rot;                           // the place of the smallest corner in the walk from the leader
};

__global__ __launch_bounds__(256) void ct_rings_kernel(unsigned int N, unsigned int rings, const unsigned int* __restrict__ svals, const unsigned long long* __restrict__ skeys,
                                                       const uint4* __restrict__ list, const unsigned long long* __restrict__ ringmin,
                                                       const unsigned long long* __restrict__ area, const unsigned long long* __restrict__ vlen,
                                                       unsigned int* __restrict__ ringpos, CtRings r) {
    const unsigned int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= rings) return;
    const unsigned int l = svals[p];
    if (l >= N) return;                                                                  // cannot happen: the first `rings` values are leaders
    const uint4 a = list[l];                                                             // the leader's list is the whole ring
    const unsigned int code = (unsigned int)(ringmin[l] & 0xffffffffull);
    r.corners[p] = 2ull * a.z; r.len[p] = (int)(2u * a.z);
    r.area2[p] = (long long)area[l]; r.length[p] = (long long)(vlen[l] + a.y);
    r.mask[p] = (int)(skeys[p] >> 32);
    r.rot[p] = (code >> 1) < N ? 2u * (a.z - list[code >> 1].z) + (code & 1u) : 0u;      // a ring has a turn, so its smallest corner a node
    ringpos[l] = p;
}

__global__ __launch_bounds__(256) void ct_write_kernel(unsigned int N, unsigned int rings, unsigned long long vertices, const uint2* __restrict__ jump,
                                                       const uint4* __restrict__ list, const int4* __restrict__ stp,
                                                       const unsigned int* __restrict__ ringpos, const unsigned long long* __restrict__ roff,
                                                       const int* __restrict__ rlen, const unsigned int* __restrict__ rot, int* __restrict__ xy) {
    const unsigned int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const int4 s = stp[v];
    if (!s.w) return;
    const unsigned int p = ringpos[jump[v].x];
    if (p >= rings) return;                                                              // cannot happen: a turn belongs to a ring
    const unsigned int L = (unsigned int)rlen[p], idx = L - 2u * list[v].z;              // the corners in front of this node's in the walk
    if (L == 0 || idx >= L) return;                                                      // cannot happen: this turn is one of the ring's
    for (unsigned int j = 0; j < 2; ++j) {                                               // ends: two corners
        const unsigned long long at = roff[p] + (idx + j + L - rot[p]) % L;
        if (at >= vertices) continue;                                                    // cannot happen: the rings tile the vertices
        xy[2 * at] = s.x; xy[2 * at + 1] = j ? s.z : s.y;
    }
}

dim3 ct_grid(unsigned long long items) { return dim3((unsigned)std::max<unsigned long long>((items + 255) / 256, 1ull)); }

int contours_device(amp_ctx* ctx, const amp::MpItems& it, int h, int connectivity, unsigned long long* ring_first, unsigned long long* ring_off,
                    int* ring_len, long long* ring_area2, long long* ring_length, unsigned long long ring_cap, int* xy, unsigned long long xy_cap,
                    unsigned long long* need) {
    const int n = (int)it.m.size();
    const unsigned int R = (unsigned int)it.S.size(), N = 2 * R;
    u64 most = 0;                                                                        // the most nodes of any one mask
    for (int p = 0; p < n; ++p) most = std::max<u64>(most, 2 * (it.first[p + 1] - it.first[p] - 1));
    int K = 0;
    while ((1ull << K) < most) ++K;                                                      // ends: most < 2^30
    AMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    amp::MpItemsDev d_items;
    amp::DevBuf d_succ, d_stp, d_j0, d_j1, d_l0, d_l1, d_min, d_area, d_vlen, d_tot;
    AMP_TRY_STATUS(d_items.upload(ctx, it));
    AMP_TRY_STATUS(amp::dev_alloc(d_succ, (size_t)N * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_stp, (size_t)N * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_j0, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_j1, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_l0, (size_t)N * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_l1, (size_t)N * 16));
    AMP_TRY_STATUS(amp::dev_alloc(d_min, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_area, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_vlen, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_tot, 16));
    AMP_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, 16, st));
    const CtArgs g{d_items.view(), h, connectivity, N};
    unsigned long long *ringmin = d_min.as<unsigned long long>(), *area = d_area.as<unsigned long long>(), *vlen = d_vlen.as<unsigned long long>(),
                       *tot = d_tot.as<unsigned long long>();
    uint2 *ja = d_j0.as<uint2>(), *jb = d_j1.as<uint2>();
    uint4 *la = d_l0.as<uint4>(), *lb = d_l1.as<uint4>();
    hipLaunchKernelGGL(ct_succ_kernel, ct_grid(N), dim3(256), 0, st, g, d_succ.as<unsigned int>(), d_stp.as<int4>(), ja, ringmin, area, vlen, tot);
    AMP_HIP_CHECK(hipGetLastError());
    for (int r = 0; r < K; ++r) {                                                        // ends: K <= 30 rounds
        hipLaunchKernelGGL(ct_min_kernel, ct_grid(N), dim3(256), 0, st, N, ja, jb);
        AMP_HIP_CHECK(hipGetLastError());
        std::swap(ja, jb);
    }
    hipLaunchKernelGGL(ct_link_kernel, ct_grid(N), dim3(256), 0, st, g, d_succ.as<unsigned int>(), d_stp.as<int4>(), ja, la, ringmin, area, vlen, tot);
    AMP_HIP_CHECK(hipGetLastError());
    unsigned long long htot[2] = {0, 0};
    AMP_HIP_CHECK(hipMemcpyAsync(htot, tot, 16, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long vertices = 2 * htot[0], rings = htot[1];
    if (htot[0] > N || 2 * rings > N || (rings == 0) != (vertices == 0)) {               // cannot happen: a node turns at most once, a ring has two nodes or more
        amp::set_error("amp_mask_contours: %llu turns in %llu rings from %u nodes on the device", htot[0], rings, N);
        return AMP_ERR_HIP;
    }
    AMP_TRY_STATUS(amp::contours_capacity(vertices, rings, xy_cap, ring_cap, need));
    if (rings == 0) {
        std::fill(ring_first, ring_first + n + 1, 0ull);
        return AMP_OK;
    }
    for (int r = 0; r < K; ++r) {                                                        // ends: K rounds
        hipLaunchKernelGGL(ct_rank_kernel, ct_grid(N), dim3(256), 0, st, N, la, lb);
        AMP_HIP_CHECK(hipGetLastError());
        std::swap(la, lb);
    }

    amp::DevBuf d_keys, d_vals, d_skeys, d_svals, d_tmp, d_pos, d_corners, d_roff, d_len, d_a2, d_length, d_mask, d_rot, d_tmp2, d_xy;
    AMP_TRY_STATUS(amp::dev_alloc(d_keys, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_vals, (size_t)N * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_skeys, (size_t)N * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_svals, (size_t)N * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_pos, (size_t)N * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_corners, (size_t)rings * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_roff, (size_t)rings * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_len, (size_t)rings * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_a2, (size_t)rings * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_length, (size_t)rings * 8));
    AMP_TRY_STATUS(amp::dev_alloc(d_mask, (size_t)rings * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_rot, (size_t)rings * 4));
    AMP_TRY_STATUS(amp::dev_alloc(d_xy, (size_t)vertices * 8));
    AMP_HIP_CHECK(hipMemsetAsync(d_pos.p, 0xff, (size_t)N * 4, st));
    hipLaunchKernelGGL(ct_keys_kernel, ct_grid(N), dim3(256), 0, st, g, ja, ringmin, d_keys.as<unsigned long long>(), d_vals.as<unsigned int>());
    AMP_HIP_CHECK(hipGetLastError());
    unsigned int bits = 32;                                                              // the key bits that tell the masks and "no leader" apart
    while ((unsigned long long)n >> (bits - 32)) ++bits;                                 // ends: n < 2^31; all ones in these bits is no mask
    size_t tmp_bytes = 0;
    AMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_keys.as<unsigned long long>(), d_skeys.as<unsigned long long>(),
                                            d_vals.as<unsigned int>(), d_svals.as<unsigned int>(), (size_t)N, 0u, bits, st));
    AMP_TRY_STATUS(amp::dev_alloc(d_tmp, tmp_bytes));
    AMP_HIP_CHECK(rocprim::radix_sort_pairs(d_tmp.p, tmp_bytes, d_keys.as<unsigned long long>(), d_skeys.as<unsigned long long>(),
                                            d_vals.as<unsigned int>(), d_svals.as<unsigned int>(), (size_t)N, 0u, bits, st));
    const CtRings rr{d_corners.as<unsigned long long>(), d_len.as<int>(), d_a2.as<long long>(), d_length.as<long long>(), d_mask.as<int>(),
                     d_rot.as<unsigned int>()};
    hipLaunchKernelGGL(ct_rings_kernel, ct_grid(rings), dim3(256), 0, st, N, (unsigned int)rings, d_svals.as<unsigned int>(),
                       d_skeys.as<unsigned long long>(), la, ringmin, area, vlen, d_pos.as<unsigned int>(), rr);
    AMP_HIP_CHECK(hipGetLastError());
    size_t tmp2_bytes = 0;
    AMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, tmp2_bytes, rr.corners, d_roff.as<unsigned long long>(), 0ull, (size_t)rings,
                                          rocprim::plus<unsigned long long>(), st));
    AMP_TRY_STATUS(amp::dev_alloc(d_tmp2, tmp2_bytes));
    AMP_HIP_CHECK(rocprim::exclusive_scan(d_tmp2.p, tmp2_bytes, rr.corners, d_roff.as<unsigned long long>(), 0ull, (size_t)rings,
                                          rocprim::plus<unsigned long long>(), st));
    hipLaunchKernelGGL(ct_write_kernel, ct_grid(N), dim3(256), 0, st, N, (unsigned int)rings, vertices, ja, la, d_stp.as<int4>(),
                       d_pos.as<unsigned int>(), d_roff.as<unsigned long long>(), rr.len, rr.rot, d_xy.as<int>());
    AMP_HIP_CHECK(hipGetLastError());

    std::vector<int> hmask((size_t)rings), hlen((size_t)rings);
    std::vector<unsigned long long> hoff((size_t)rings);
    AMP_HIP_CHECK(hipMemcpyAsync(hmask.data(), d_mask.p, (size_t)rings * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(hlen.data(), d_len.p, (size_t)rings * 4, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(hoff.data(), d_roff.p, (size_t)rings * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t r = 0; r < (size_t)rings; ++r) {                                         // cannot fail: the rings come in mask order and tile the vertices
        const bool ok = hmask[r] >= 0 && hmask[r] < n && (r == 0 || hmask[r] >= hmask[r - 1]) && hlen[r] >= 4
                        && hoff[r] == (r ? hoff[r - 1] + (unsigned long long)hlen[r - 1] : 0ull) && hoff[r] + (unsigned long long)hlen[r] <= vertices;
        if (!ok || (r + 1 == (size_t)rings && hoff[r] + (unsigned long long)hlen[r] != vertices)) {
            amp::set_error("amp_mask_contours: ring %zu of %llu: mask %d, %d corners at %llu of %llu on the device", r, rings, hmask[r], hlen[r],
                           hoff[r], vertices);
            return AMP_ERR_HIP;
        }
    }
    AMP_HIP_CHECK(hipMemcpyAsync(xy, d_xy.p, (size_t)vertices * 8, hipMemcpyDeviceToHost, st));       // everything computed: the outputs are written from here on
    AMP_HIP_CHECK(hipMemcpyAsync(ring_area2, d_a2.p, (size_t)rings * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipMemcpyAsync(ring_length, d_length.p, (size_t)rings * 8, hipMemcpyDeviceToHost, st));
    AMP_HIP_CHECK(hipStreamSynchronize(st));
    std::copy(hoff.begin(), hoff.end(), ring_off);
    std::copy(hlen.begin(), hlen.end(), ring_len);
    size_t r = 0;
    for (int p = 0; p <= n; ++p) {                                                       // ring_first[p] = the rings of the masks before p
        while (r < (size_t)rings && hmask[r] < p) ++r;                                   // ends: r grows to rings
        ring_first[p] = r;
    }
    return AMP_OK;
}

}  // namespace

extern "C" int amp_mask_contours(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                                 int connectivity, unsigned long long* ring_first, unsigned long long* ring_off, int* ring_len,
                                 long long* ring_area2, long long* ring_length, unsigned long long ring_cap, int* xy, unsigned long long xy_cap,
                                 unsigned long long* need) {
    amp::RunPlan plan;
    AMP_TRY_STATUS(amp::contours_check(pool, off, len, n, h, w, connectivity, ring_first, ring_off, ring_len, ring_area2, ring_length, xy, need, plan));
    if (n == 0) {
        need[0] = 0; need[1] = 0; ring_first[0] = 0;
        return AMP_OK;
    }
    amp::MpItems items;
    AMP_REQUIRE(amp::mp_build_items(plan, h, w, 1, items) && items.S.size() < AMP_CONTOUR_MAX_ITEMS,
                "amp_mask_contours: the masks of one call have more than 2^29 pieces");
    return ctx ? contours_device(ctx, items, h, connectivity, ring_first, ring_off, ring_len, ring_area2, ring_length, ring_cap, xy, xy_cap, need)
               : amp::contours_host(items, h, connectivity, ring_first, ring_off, ring_len, ring_area2, ring_length, ring_cap, xy, xy_cap, need);
}
