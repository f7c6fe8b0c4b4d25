// amp_mask_region_props: the integer arithmetic that the host evaluation (mask_analysis_host.hip) and the device kernels (region_props.hip)
// share, so the two paths cannot drift apart: closed-form moment sums of a run, the border and perimeter-class boards of one 64-row word, and
// the convex hull chain with its per-column fill.  Plain C++ (the host-only sanitizer builds compile it with g++), integers throughout; the
// word type and the bit counts are run_list.h's.
#pragma once
#include "run_list.h"

namespace amp {

// one mask of a call: its tight box in the image and where its scratch lies
struct RpMask {
    int H, W;                     // the tight box (0, 0 for an empty mask: no plane, no tile)
    int r0, c0;                   // its origin in the image
    int pitch;                    // 64-bit words per plane column = ceil(H / 64)
    int n;                        // its runs of ones, the long ones cut (region_props.hip)
    u64 run0;                     // where they start in the call's list of runs
    u64 plane;                    // word offset of the mask plane; the border plane follows it (W * pitch words each)
    u64 hull;                     // int offset of the hull scratch: lo[X], hi[X], lower stack, upper stack, 2 W + 1 ints each
};

AMP_HD u64 rp_sq_sum(u64 k) { return k * (k + 1) * (2 * k + 1) / 6; }      // 0^2 + ... + k^2; k <= 32767: below 2^46 before the division

// rows [ya, yb): acc += {N, sum r, sum c, sum r^2, sum r c, sum c^2}
// in each of `cols` columns whose indices sum to csum and their squares to c2sum (one column c: 1, c, c * c)
AMP_HD void rp_segment(u64 ya, u64 yb, u64 cols, u64 csum, u64 c2sum, u64* acc) {
    const u64 n = yb - ya;
    const u64 sr = (ya + yb - 1) * n / 2;
    const u64 srr = rp_sq_sum(yb - 1) - (ya ? rp_sq_sum(ya - 1) : 0ull);
    acc[0] += cols * n;
    acc[1] += cols * sr;
    acc[2] += csum * n;
    acc[3] += cols * srr;
    acc[4] += csum * sr;
    acc[5] += c2sum * n;
}

// pixels [s, e) of the column-major image (s < e <= h * w <= 2^30): the partial first column, the full columns between as one closed form,
// the partial last column.  Every total of a mask stays below 2^60 (h, w <= 32768, h * w <= 2^30).
AMP_HD void rp_run_sums(u64 s, u64 e, u64 h, u64* acc) {
    const u64 cf = s / h, cl = (e - 1) / h;
    const u64 ya = s - cf * h, yb = e - cl * h;                   // first row of the run in cf, one past its last row in cl
    if (cf == cl) { rp_segment(ya, yb, 1, cf, cf * cf, acc); return; }
    rp_segment(ya, h, 1, cf, cf * cf, acc);
    rp_segment(0, yb, 1, cl, cl * cl, acc);
    if (cl - cf > 1) {
        const u64 a = cf + 1, b = cl - 1, m = b - a + 1;
        rp_segment(0, h, m, (a + b) * m / 2, rp_sq_sum(b) - rp_sq_sum(a - 1), acc);
    }
}

// One 64-row word x of a column-major bit plane (bit b = row 64 wv + b) with its neighbours: above / below = the words wv - 1 / wv + 1 of the
// same column, left / right = word wv of the columns beside it (0 outside the plane).  up(x) holds at bit b the pixel of row b - 1.
AMP_HD u64 rp_up(u64 x, u64 above) { return (x << 1) | (above >> 63); }
AMP_HD u64 rp_down(u64 x, u64 below) { return (x >> 1) | (below << 63); }

// border = mask minus its erosion by the 4-connected cross, outside counting as 0
AMP_HD u64 rp_border_word(u64 x, u64 above, u64 below, u64 left, u64 right) {
    return x & ~(rp_up(x, above) & rp_down(x, below) & left & right);
}

// word wv of column q of a W-column plane, 0 outside it
AMP_HD u64 rp_word(const u64* plane, int W, int pitch, int q, int wv) {
    return (q < 0 || q >= W || wv < 0 || wv >= pitch) ? 0ull : plane[(size_t)q * pitch + wv];
}
AMP_HD u64 rp_border_at(const u64* mask, int W, int pitch, int q, int wv) {
    return rp_border_word(mask[(size_t)q * pitch + wv], rp_word(mask, W, pitch, q, wv - 1), rp_word(mask, W, pitch, q, wv + 1),
                          rp_word(mask, W, pitch, q - 1, wv), rp_word(mask, W, pitch, q + 1, wv));
}

// b[j][i]: the border words of column q - 1 + j, word wv - 1 + i (3 x 3 around the word classified).  out = the three predicate boards:
// P1: n4 in {2, 3} and nd in {0, 1, 2};  P2: (n4, nd) in {(0, 2), (1, 3)};  P3: (n4, nd) in {(1, 1), (1, 2)}, n4 / nd the numbers of
// 4-neighbours / diagonal neighbours on the border, counted bit-sliced over the 64 rows.
AMP_HD void rp_classify_word(const u64 b[3][3], u64* out) {
    const u64 x = b[1][1];
    const u64 U = rp_up(x, b[1][0]), D = rp_down(x, b[1][2]), L = b[0][1], R = b[2][1];
    const u64 UL = rp_up(b[0][1], b[0][0]), DL = rp_down(b[0][1], b[0][2]), UR = rp_up(b[2][1], b[2][0]), DR = rp_down(b[2][1], b[2][2]);
    // a + b + c + d as three bit planes: (s1 + s2) + 2 (c1 + c2); s1 & s2 implies c1 = c2 = 0, so the 4s plane is c1 & c2
    const u64 s1 = U ^ D, c1 = U & D, s2 = L ^ R, c2 = L & R;
    const u64 n0 = s1 ^ s2, n1 = c1 ^ c2 ^ (s1 & s2), n2 = c1 & c2;
    const u64 t1 = UL ^ DL, e1 = UL & DL, t2 = UR ^ DR, e2 = UR & DR;
    const u64 d0 = t1 ^ t2, d1 = e1 ^ e2 ^ (t1 & t2), d2 = e1 & e2;
    const u64 n4_0 = ~n0 & ~n1 & ~n2, n4_1 = n0 & ~n1 & ~n2, n4_23 = n1 & ~n2;
    const u64 nd_1 = d0 & ~d1 & ~d2, nd_2 = ~d0 & d1 & ~d2, nd_3 = d0 & d1, nd_le2 = ~d2 & ~(d0 & d1);
    out[0] = x & n4_23 & nd_le2;
    out[1] = x & ((n4_0 & nd_2) | (n4_1 & nd_3));
    out[2] = x & n4_1 & (nd_1 | nd_2);
}

AMP_HD void rp_classify_at(const u64* border, int W, int pitch, int q, int wv, u64* out) {
    u64 b[3][3];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) b[j][i] = rp_word(border, W, pitch, q - 1 + j, wv - 1 + i);
    rp_classify_word(b, out);
}

// ---- convex hull in half-pixel units: X = 2 column, Y = 2 row, both relative to the box origin ---------------------------------------------
// The hull of the pixels' edge midpoints is the hull of the diamonds of each column's topmost (t) and bottommost (b) pixel.  Of those, only the
// extreme point at each X can be a vertex: at X = 2 c the points 2 t - 1 (low) and 2 b + 1 (high), at X = 2 c -+ 1 the points 2 t and 2 b.
// Point index i = X + 1 runs over 0 .. 2 W; lo[i] / hi[i] = RP_NONE where no column contributes (the gap between two parts).
constexpr int RP_NONE = 1 << 30;

// top / bottom: first / last set row of a plane column (top > bottom: the column is empty)
AMP_HD void rp_column_extent(const u64* col, int pitch, int* top, int* bottom) {
    *top = RP_NONE; *bottom = -RP_NONE;
    for (int wv = 0; wv < pitch; ++wv)
        if (col[wv]) { *top = (wv << 6) + ctz(col[wv]); break; }
    for (int wv = pitch - 1; wv >= 0; --wv)
        if (col[wv]) { *bottom = (wv << 6) + 63 - clz(col[wv]); break; }
}

// lo / hi of point i from the extents of the one or two columns that touch it (odd i: column (i - 1) / 2 itself; even i: the columns
// i / 2 - 1 and i / 2 on either side)
AMP_HD void rp_point(int i, int W, const u64* plane, int pitch, int* lo, int* hi) {
    int t, b;
    *lo = RP_NONE; *hi = RP_NONE;
    if (i & 1) {
        rp_column_extent(plane + (size_t)(i >> 1) * pitch, pitch, &t, &b);
        if (t <= b) { *lo = 2 * t - 1; *hi = 2 * b + 1; }
        return;
    }
    int l = RP_NONE, u = -RP_NONE;
    for (int c = (i >> 1) - 1; c <= (i >> 1); ++c) {
        if (c < 0 || c >= W) continue;
        rp_column_extent(plane + (size_t)c * pitch, pitch, &t, &b);
        if (t <= b) { l = t < l ? t : l; u = b > u ? b : u; }
    }
    if (l <= u) { *lo = 2 * l; *hi = 2 * u; }
}

// Monotone chain over the points (i, y[i]), i = 0 .. n - 1 ascending, y[i] == RP_NONE skipped.  sign = +1: the lower chain (minimal Y), -1: the
// upper.  stk receives the point indices of the chain; returns their number.  Collinear points are dropped.  One pass, each point pushed and
// popped at most once.
AMP_HD int rp_chain(const int* y, int n, int sign, int* stk) {
    int k = 0;
    for (int i = 0; i < n; ++i) {
        if (y[i] == RP_NONE) continue;
        while (k >= 2) {
            const long long ax = stk[k - 1] - stk[k - 2], ay = y[stk[k - 1]] - y[stk[k - 2]];
            const long long bx = i - stk[k - 2], by = y[i] - y[stk[k - 2]];
            if ((ax * by - ay * bx) * sign > 0) break;          // a strict turn towards the inside: the last vertex stays
            --k;
        }
        stk[k++] = i;
    }
    return k;
}

AMP_HD long long rp_floor_div(long long a, long long b) {      // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Chain edge (i1, y1) - (i2, y2), i1 < i2: summed over the pixel-centre columns X = 2 c (odd point index i) with i1 < i <= i2, the bound
// on the centre row r (Y = 2 r) that the edge sets: upper chain floor(Y(X) / 2), lower chain ceil(Y(X) / 2), Y(X) = y1 + (y2 - y1) (i - i1) /
// (i2 - i1).  |numerator| < 2^36.
AMP_HD long long rp_edge_sum(int i1, int y1, int i2, int y2, bool upper) {
    const long long dx = i2 - i1, dy = y2 - y1;
    long long s = 0;
    for (int i = (i1 + 1) | 1; i <= i2; i += 2) {
        const long long num = (long long)y1 * dx + dy * (i - i1);       // Y(X) * dx
        s += upper ? rp_floor_div(num, 2 * dx) : -rp_floor_div(-num, 2 * dx);
    }
    return s;
}

}  // namespace amp
