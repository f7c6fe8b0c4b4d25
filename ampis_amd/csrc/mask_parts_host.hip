// Host side of amp_mask_parts (mask_parts.h): the argument check, whose plan both paths evaluate, the capacity report, and the evaluation with
// a NULL context -- the connected components of the ones (colour 1) or of the zeros (colour 0) of every mask of a pool, the ones a rule picks
// flipped, the results as canonical COCO run lists.  On the items of mask_parts.h:
//   union    every COMPONENT item against the COMPONENT items of the column before it in the same mask whose rows meet its own (one row wider
//            on each side where diagonal neighbours count); the larger root goes under the smaller, so a root is its set's first item;
//   reduce   per root the area and, colour 0, whether the set touches the border of the tight box (then it is the outside, not a hole); per
//            mask the components, their pixels and the best one (largest area, then smallest root);
//   emit     every item's value in the result, a boundary where the value changes between items that meet, the differences as counts.
// Plain C++ throughout, integers only: the host-only sanitizer build of tests/sanitize compiles this file with g++.  mask_parts.hip computes the
// same bytes on the device.
#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "mask_parts.h"

namespace amp {

int mask_parts_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int colour, int connectivity,
                     int keep_largest, const unsigned long long* stats, const uint32_t* out_pool, const unsigned long long* out_off,
                     const int* out_len, const unsigned long long* need, RunPlan& runs) {
    AMP_REQUIRE(n >= 0, "amp_mask_parts: n = %d", n);
    AMP_TRY_STATUS(require_image_size("amp_mask_parts", h, w));
    AMP_REQUIRE(colour == 0 || colour == 1, "amp_mask_parts: colour = %d (1: parts of the ones, 0: holes of the zeros)", colour);
    AMP_REQUIRE(connectivity == 1 || connectivity == 2, "amp_mask_parts: connectivity = %d (1: 4 neighbours, 2: 8 neighbours)", connectivity);
    AMP_REQUIRE(keep_largest == 0 || (keep_largest == 1 && colour == 1), "amp_mask_parts: keep_largest = %d with colour = %d (0 or 1, parts only)",
                keep_largest, colour);
    AMP_REQUIRE(n == 0 || (pool && off && len && stats), "amp_mask_parts: null argument %s",
                !pool ? "pool" : !off ? "off" : !len ? "len" : "stats");
    AMP_REQUIRE(!out_pool || n == 0 || (out_off && out_len), "amp_mask_parts: null argument %s", !out_off ? "out_off" : "out_len");
    AMP_REQUIRE(!out_pool || need, "amp_mask_parts: null argument need");
    AMP_TRY_STATUS(plan_pool("amp_mask_parts", pool, off, len, n, h, w, runs));
    return AMP_OK;
}

int mask_parts_capacity(unsigned long long counts, unsigned long long out_cap, unsigned long long* need) {
    return counts_capacity("amp_mask_parts", "out_cap", counts, out_cap, need);
}

int mask_parts_host(const MpItems& it, int h, int colour, int connectivity, unsigned int threshold, int keep_largest,
                    unsigned long long* stats, uint32_t* out_pool, unsigned long long out_cap, unsigned long long* out_off, int* out_len,
                    unsigned long long* need) {
    const size_t R = it.S.size(), n = it.m.size();
    const std::vector<uint32_t>&S = it.S, &E = it.E;
    std::vector<uint32_t> parent(R), area(R, 0u);
    std::vector<uint8_t> touch(R, 0), value(R, 0);
    for (size_t i = 0; i < R; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }         // ends: parent[x] < x until the root
        return x;
    };
    const uint32_t d = (uint32_t)mp_reach(colour, connectivity), shift = (uint32_t)h;     // a piece of column q - 1 moved one column right
    for (size_t p = 0; p < n; ++p) {
        const MpMask& mk = it.m[p];
        for (int q = 1; q < mk.W; ++q) {
            uint32_t j = it.col[mk.col0 + (size_t)q - 1];
            const uint32_t jend = it.col[mk.col0 + (size_t)q], iend = it.col[mk.col0 + (size_t)q + 1];
            for (uint32_t i = jend; i < iend; ++i) {
                if (it.T[i] != MP_COMPONENT) continue;
                while (j < jend && E[j] + shift + d <= S[i]) ++j;                          // pieces that end above item i end above every later one
                for (uint32_t k = j; k < jend && S[k] + shift < E[i] + d; ++k) {
                    if (it.T[k] != MP_COMPONENT) continue;
                    uint32_t a = find(i), b = find(k);
                    if (a == b) continue;
                    if (a < b) std::swap(a, b);
                    parent[a] = b;
                }
            }
        }
    }
    std::vector<uint32_t> root(R);
    std::vector<u64> st(4 * n, 0ull), best(n, 0ull);
    for (size_t p = 0; p < n; ++p) {
        const MpMask& mk = it.m[p];
        const size_t i0 = (size_t)it.first[p], i1 = (size_t)it.first[p + 1];
        for (size_t i = i0; i < i1; ++i) {
            if (it.T[i] != MP_COMPONENT) continue;
            root[i] = find((uint32_t)i);
            area[root[i]] += E[i] - S[i];
            if (colour == 0 && mp_touches(mk, h, S[i], E[i])) touch[root[i]] = 1;
        }
        for (size_t i = i0; i < i1; ++i) {
            if (it.T[i] != MP_COMPONENT || root[i] != i || touch[i]) continue;
            st[4 * p] += 1;
            st[4 * p + 1] += area[i];
            best[p] = std::max(best[p], mp_best_key(area[i], (uint32_t)i));
        }
        st[4 * p + 2] = best[p] >> 32;
        for (size_t i = i0; i < i1; ++i) {
            bool flip = false;
            if (it.T[i] == MP_COMPONENT) {
                const uint32_t r = root[i];
                flip = mp_flip(colour, !touch[r], area[r], r, best[p], threshold, keep_largest);
                if (flip && r == i) st[4 * p + 3] += area[r];
            }
            value[i] = (uint8_t)mp_value(it.T[i], colour, flip);
        }
    }
    if (!out_pool) {
        std::copy(st.begin(), st.end(), stats);
        return AMP_OK;
    }
    std::vector<uint32_t> out;
    std::vector<unsigned long long> off(n + 1, 0ull);
    for (size_t p = 0; p < n; ++p) {
        const size_t i0 = (size_t)it.first[p], i1 = (size_t)it.first[p + 1];
        uint32_t prev = 0;                        // the boundary before
        for (size_t i = i0; i < i1; ++i) {
            const bool last = i + 1 == i1;        // the END item
            const MpBounds b = mp_bounds(it.T[i], value[i], S[i], E[i], i > i0, i > i0 ? value[i - 1] : 0, i > i0 ? E[i - 1] : 0u,
                                         last ? 0 : value[i + 1], last ? 0u : S[i + 1]);
            if (b.s) { out.push_back(S[i] - prev); prev = S[i]; }
            if (b.e) { out.push_back(E[i] - prev); prev = E[i]; }
        }
        off[p + 1] = out.size();
    }
    AMP_TRY_STATUS(mask_parts_capacity(out.size(), out_cap, need));
    std::copy(st.begin(), st.end(), stats);
    std::copy(out.begin(), out.end(), out_pool);
    for (size_t p = 0; p < n; ++p) {
        out_off[p] = off[p];
        out_len[p] = (int)(off[p + 1] - off[p]);
    }
    return AMP_OK;
}

}  // namespace amp
