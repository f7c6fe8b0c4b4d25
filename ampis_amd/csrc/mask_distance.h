// amp_mask_distance: what the host evaluation (mask_distance_host.hip) and the device kernel (mask_distance.hip) share -- the walk that finds
// the squared distance of one pixel, and the bin of the erosion curve it falls in.  Plain C++ that also compiles under g++ (the host-only
// sanitizer build), integers throughout.
//
// The masks are cut into PIECES, maximal vertical runs of ones of one column: the items of mask_parts.h at colour 1 (mp_build_items), with
// their index col[col0 + q] = the first piece of column q of the mask's tight box, col[col0 + W] = the END item.  For a pixel at row r of
// piece [s, e) of its own column the column distance is g = min(r - s + 1, e - r); with border_value 1 a side that is the image's edge
// (s == 0 or e == h) does not count.  d2 = min over the columns c' of (c - c')^2 + g_c'(r)^2 with g_c'(r) = 0 where (r, c') is not in the
// mask; with border_value 0 the columns -1 and w contribute (c - c')^2.  md_pixel walks the columns outwards from the pixel's own and stops
// as soon as dx^2 reaches the best value so far: every column not visited is at least that far, so the result is exact.  A pixel's work
// grows with its own distance -- one binary search per column of the walk --: O(pixels x inscribed radius) in the worst case.
//
// AMP_DIST_NONE stands for "no background": a piece that spans the whole column with border_value 1 has no column distance, and a mask that
// fills the image has none at all.  Every real value is below 2^31: dx <= 32767 and g <= 32768 with dx^2 + g^2 < 2^31 on h * w <= 2^30.
#pragma once
#include "../../include/ampis_hip.h"
#include "mask_parts.h"

namespace amp {

constexpr int MD_MAX_CURVE = AMP_MORPH_MAX_RADIUS + 1;

struct MdView {
    const uint32_t *S, *E, *col;      // MpItems' arrays of the whole pool
    int h, w, border;
};

// g^2 of row r in the piece of rows [s, e), s <= r < e; AMP_DIST_NONE when no side counts
AMP_HD uint32_t md_gap2(int r, int s, int e, int h, int border) {
    uint32_t g = AMP_DIST_NONE;
    if (!(border && s == 0)) g = (uint32_t)(r - s + 1);
    if (!(border && e == h) && (uint32_t)(e - r) < g) g = (uint32_t)(e - r);
    return g == AMP_DIST_NONE ? g : g * g;
}

// what column cc of the image (0 <= cc < w), dx columns away with dx2 = dx^2, offers the pixel at row r
AMP_HD uint32_t md_column(const MdView& v, const MpMask& mk, int r, int cc, uint32_t dx2) {
    const int q = cc - mk.c0;
    if (q < 0 || q >= mk.W) return dx2;
    const uint32_t cb = (uint32_t)cc * (uint32_t)v.h, pos = cb + (uint32_t)r, end = v.col[mk.col0 + (unsigned)q + 1];
    uint32_t lo = v.col[mk.col0 + (unsigned)q], hi = end;
    while (lo < hi) {                                                                    // ends: hi - lo halves; the first piece that ends beyond pos
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v.E[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    if (lo == end || v.S[lo] > pos) return dx2;                                          // (r, cc) is not in the mask
    const uint32_t g2 = md_gap2(r, (int)(v.S[lo] - cb), (int)(v.E[lo] - cb), v.h, v.border);
    return g2 == AMP_DIST_NONE ? g2 : dx2 + g2;
}

// d2 of the pixel at row r of column c, in the piece of rows [s, e) of that column
AMP_HD uint32_t md_pixel(const MdView& v, const MpMask& mk, int r, int c, int s, int e) {
    uint32_t best = md_gap2(r, s, e, v.h, v.border);
    for (int dx = 1;; ++dx) {                                                            // ends: dx grows; by column -1 or w (border 0) or both sides left (border 1)
        const uint32_t dx2 = (uint32_t)dx * (uint32_t)dx;
        if (dx2 >= best) break;
        const int cl = c - dx, cr = c + dx;
        if (v.border && cl < 0 && cr >= v.w) break;
        const uint32_t a = cl >= 0 ? md_column(v, mk, r, cl, dx2) : v.border ? AMP_DIST_NONE : dx2;
        const uint32_t b = cr < v.w ? md_column(v, mk, r, cr, dx2) : v.border ? AMP_DIST_NONE : dx2;
        best = a < best ? a : best;
        best = b < best ? b : best;
    }
    return best;
}

// the bin of the erosion curve: k = #{r in [0, ncurve) : r^2 < d2}; curve[r] = the pixels with k > r
AMP_HD int md_bin(uint32_t d2, int ncurve) {
    int lo = 0, hi = ncurve;
    while (lo < hi) {                                                                    // ends: hi - lo halves; the smallest r with r^2 >= d2
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(mid * mid) < d2) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a mask's deepest pixel as one word for an integer max: the largest d2, among equals the smallest position
AMP_HD u64 md_best_key(uint32_t d2, uint32_t pos) { return ((u64)d2 << 32) | (u64)(0xffffffffu - pos); }

// what the host and the device path fill per mask before the outputs are written
struct MdTotals {
    std::vector<u64> best, sum, area;         // [n]: md_best_key's maximum (0 for an empty mask), the sum of the real d2, the pixels
    std::vector<u64> hist;                    // [n][ncurve + 1]: the pixels by md_bin
};

// mask_distance_host.hip: the argument check builds the plan and the items; the capacity report; the evaluation on the host; the outputs
// from the totals of either path
int mask_distance_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int border_value,
                        const unsigned long long* stats, const long long* boxes, const unsigned long long* curve, int ncurve, const uint32_t* map,
                        unsigned long long map_cap, const unsigned long long* map_off, const unsigned long long* need, RunPlan& plan, MpItems& items,
                        std::vector<u64>& offs);
int mask_distance_capacity(const std::vector<u64>& offs, unsigned long long map_cap, unsigned long long* need);
void mask_distance_host(const MpItems& it, int h, int w, int border_value, int ncurve, const std::vector<u64>& offs, uint32_t* map, MdTotals& t);
void mask_distance_write(const RunPlan& plan, const MdTotals& t, int ncurve, const std::vector<u64>& offs, bool with_map,
                         unsigned long long* stats, long long* boxes, unsigned long long* curve, unsigned long long* map_off);

}  // namespace amp
