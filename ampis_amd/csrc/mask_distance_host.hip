// Host side of amp_mask_distance (mask_distance.h): the argument check, whose plan and pieces both paths evaluate, the capacity report, the
// evaluation with a NULL context -- md_pixel for every pixel of every piece, the walk the kernel's lanes run --, and the outputs from the
// per-mask totals of either path.  Plain C++ throughout, integers only: the host-only sanitizer build of tests/sanitize compiles this file
// with g++.  mask_distance.hip computes the same bytes on the device.
#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "mask_distance.h"

namespace amp {

int mask_distance_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int border_value,
                        const unsigned long long* stats, const long long* boxes, const unsigned long long* curve, int ncurve, const uint32_t* map,
                        unsigned long long map_cap, const unsigned long long* map_off, const unsigned long long* need, RunPlan& plan, MpItems& items,
                        std::vector<u64>& offs) {
    AMP_REQUIRE(n >= 0, "amp_mask_distance: n = %d", n);
    AMP_TRY_STATUS(require_image_size("amp_mask_distance", h, w));
    AMP_REQUIRE(border_value == 0 || border_value == 1, "amp_mask_distance: border_value = %d (0 or 1)", border_value);
    AMP_REQUIRE(ncurve >= 0 && ncurve <= MD_MAX_CURVE, "amp_mask_distance: ncurve = %d (0 .. %d)", ncurve, MD_MAX_CURVE);
    AMP_REQUIRE(curve || ncurve == 0, "amp_mask_distance: null argument curve with ncurve = %d", ncurve);
    AMP_REQUIRE(map || map_cap == 0, "amp_mask_distance: map_cap = %llu with a null map", map_cap);
    AMP_REQUIRE(!map || need, "amp_mask_distance: null argument need");
    AMP_REQUIRE(n == 0 || (pool && off && len && stats && boxes && (!map || map_off)), "amp_mask_distance: null argument %s",
                !pool ? "pool" : !off ? "off" : !len ? "len" : !stats ? "stats" : !boxes ? "boxes" : "map_off");
    AMP_TRY_STATUS(plan_pool("amp_mask_distance", pool, off, len, n, h, w, plan));
    AMP_REQUIRE(mp_build_items(plan, h, w, 1, items), "amp_mask_distance: the masks of one call have more than 2^31 pieces");
    offs.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const RunMask& mk = plan.m[(size_t)i];
        offs[(size_t)i + 1] = offs[(size_t)i] + (u64)(mk.r1 - mk.r0) * (u64)(mk.c1 - mk.c0);
    }
    return AMP_OK;
}

int mask_distance_capacity(const std::vector<u64>& offs, unsigned long long map_cap, unsigned long long* need) {
    return counts_capacity("amp_mask_distance", "map_cap", offs.back(), map_cap, need);
}

void mask_distance_host(const MpItems& it, int h, int w, int border_value, int ncurve, const std::vector<u64>& offs, uint32_t* map, MdTotals& t) {
    const size_t n = it.m.size(), bins = (size_t)ncurve + 1;
    t.best.assign(n, 0); t.sum.assign(n, 0); t.area.assign(n, 0);
    t.hist.assign(ncurve ? n * bins : 0, 0);
    if (map) std::fill(map, map + offs[n], 0u);
    const MdView v{it.S.data(), it.E.data(), it.col.data(), h, w, border_value};
    for (size_t i = 0; i < n; ++i) {
        const MpMask& mk = it.m[i];
        for (size_t j = (size_t)it.first[i]; j + 1 < (size_t)it.first[i + 1]; ++j) {      // the pieces; the last item is the END item
            const int c = (int)(it.S[j] / (unsigned)h), s = (int)(it.S[j] - (unsigned)c * (unsigned)h), e = (int)(it.E[j] - (unsigned)c * (unsigned)h);
            for (int r = s; r < e; ++r) {
                const uint32_t d2 = md_pixel(v, mk, r, c, s, e);
                t.best[i] = std::max(t.best[i], md_best_key(d2, (uint32_t)c * (uint32_t)h + (uint32_t)r));
                if (d2 != AMP_DIST_NONE) t.sum[i] += d2;
                ++t.area[i];
                if (ncurve) ++t.hist[i * bins + (size_t)md_bin(d2, ncurve)];
                if (map) map[offs[i] + (u64)(r - mk.r0) * (u64)mk.W + (u64)(c - mk.c0)] = d2;
            }
        }
    }
}

void mask_distance_write(const RunPlan& plan, const MdTotals& t, int ncurve, const std::vector<u64>& offs, bool with_map,
                         unsigned long long* stats, long long* boxes, unsigned long long* curve, unsigned long long* map_off) {
    const size_t n = plan.m.size(), bins = (size_t)ncurve + 1;
    for (size_t i = 0; i < n; ++i) {
        const RunMask& mk = plan.m[i];
        const bool any = t.area[i] != 0;
        stats[4 * i] = any ? t.best[i] >> 32 : 0;
        stats[4 * i + 1] = any ? 0xffffffffull - (t.best[i] & 0xffffffffull) : 0;
        stats[4 * i + 2] = t.sum[i];
        stats[4 * i + 3] = t.area[i];
        boxes[4 * i] = mk.r0; boxes[4 * i + 1] = mk.c0; boxes[4 * i + 2] = mk.r1; boxes[4 * i + 3] = mk.c1;
        u64 above = 0;                                                                   // the pixels of the bins above r
        for (int r = ncurve - 1; r >= 0; --r) {
            above += t.hist[i * bins + (size_t)r + 1];
            curve[i * (size_t)ncurve + (size_t)r] = above;
        }
        if (with_map) map_off[i] = offs[i];
    }
}

}  // namespace amp
