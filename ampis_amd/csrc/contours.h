// amp_mask_contours: what the host walk (contours_host.hip) and the device kernels (contours.hip) share -- the NODES of a pool of masks and their
// successor function.  Plain C++ that also compiles under g++ (the host-only sanitizer build), integers throughout.
//
// The masks are cut into the colour-1 items of mask_parts.h: vertical pieces [S, E) of one column, adjacent pieces of a column joined, and one
// END item per mask.  Pixel (r, c) is the square [c, c + 1] x [r, r + 1]; a boundary edge is directed with the one on its right hand, y down.
// The directed HORIZONTAL unit edges are the nodes, two per piece i of column c, rows [a, b):
//   node 2 i      the top edge, (c, a) -> (c + 1, a), heading east;
//   node 2 i + 1  the bottom edge, (c + 1, b) -> (c, b), heading west.
// The two nodes of an END item are dead: they belong to no ring.  ct_successor follows the boundary from a node's head to the next node: either
// straight on (the neighbouring column has a piece end of the same kind at the same y: no corner), or along ONE vertical segment of the column
// line x, from y0 (the node's row) to y1, which gives the two corners (x, y0), (x, y1).  A vertical segment ends only at a piece end of one of
// the two columns beside it, so y1 is the nearer of two candidates; where they coincide the vertex is a saddle and the connectivity decides:
// left on to the diagonal pixel for 2, right along the own pixel for 1.  The cases, with the four pixels around the head vertex:
//   top edge, head (c + 1, a), SW = 1 (the piece), NW = 0; ne / se = column c + 1 at rows a - 1 / a
//     ne = 0, se = 1                    straight: the top edge of the piece of column c + 1 that starts at a
//     ne = 1 and (se = 1 or k = 2)      north (se = 0: a saddle, left): up to the start t of the piece of column c + 1 that holds row a - 1 or the
//                                       end e of the piece above in column c, whichever is nearer (larger); t > e: that piece's top edge; e > t:
//                                       the bottom edge of the piece above; t = e: a saddle, k = 2 the bottom edge (left), k = 1 the top edge
//     otherwise                         south (ne = 1: a saddle, right): down to the own end b or the start s of the next piece of column c + 1,
//                                       whichever is nearer (smaller); b < s: the own bottom edge; s < b: that piece's top edge; s = b: a
//                                       saddle, k = 2 the top edge (left), k = 1 the own bottom edge
//   bottom edge, head (c, b), NE = 1 (the piece), SE = 0; nw / sw = column c - 1 at rows b - 1 / b: the same turned by half a turn
//     nw = 1, sw = 0                    straight: the bottom edge of the piece of column c - 1 that ends at b
//     sw = 1 and (nw = 1 or k = 2)      south: down to the end e of the piece of column c - 1 that holds row b or the start s of the next piece
//                                       of column c; e < s: that piece's bottom edge; s < e: the next piece's top edge; e = s: k = 2 the top edge
//     otherwise                         north: up to the own start a or the end e of the last piece of column c - 1 above row b; a > e: the own
//                                       top edge; e > a: that piece's bottom edge; e = a: k = 2 that bottom edge, k = 1 the own top edge
// Every vertical segment has length >= 1 and both its ends are corners, because the step before and the step after are horizontal.
#pragma once
#include "mask_parts.h"

namespace amp {

struct CtStep {
    unsigned int next;            // the successor node
    int turn;                     // 0: straight on, no corner; 1: the two corners (x, y0), (x, y1)
    int x, y0, y1;
};

// the first item of [lo, hi) that ends beyond position p (the item ends ascend); hi when there is none
AMP_HD unsigned int ct_first_ending_after(const uint32_t* E, unsigned int lo, unsigned int hi, long long p) {
    while (lo < hi) {                                                                    // ends: hi - lo halves
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if ((long long)E[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The successor of a live node of mask mk (S, E, col: the items of mask_parts.h, colour 1).  k = the connectivity, 1 or 2.
AMP_HD CtStep ct_successor(const uint32_t* S, const uint32_t* E, const uint32_t* col, const MpMask& mk, int h, int k, unsigned int node) {
    const unsigned int i = node >> 1;
    const long long H = h, A = S[i], B = E[i];
    const int c = (int)(A / H), q = c - mk.c0;
    const long long cb = (long long)c * H;
    const unsigned int olo = col[mk.col0 + (unsigned)q], ohi = col[mk.col0 + (unsigned)q + 1];    // the pieces of the own column
    const long long none_above = -1, none_below = 1ll << 40;
    CtStep st;
    st.turn = 1;
    if (!(node & 1)) {                                                                   // top edge, head (c + 1, a)
        const bool has = q + 1 < mk.W;
        const unsigned int nlo = has ? col[mk.col0 + (unsigned)q + 1] : 0u, nhi = has ? col[mk.col0 + (unsigned)q + 2] : 0u;
        const unsigned int j = ct_first_ending_after(E, nlo, nhi, A + H - 1);            // the piece that holds row a - 1 of column c + 1, or the next one
        const bool ne = j < nhi && (long long)S[j] <= A + H - 1;
        const bool se = j < nhi && (ne ? (long long)E[j] > A + H : (long long)S[j] == A + H);
        st.x = c + 1; st.y0 = (int)(A - cb);
        if (!ne && se) { st.next = 2 * j; st.turn = 0; st.y1 = st.y0; return st; }
        if (ne && (se || k == 2)) {                                                      // north
            const long long t = (long long)S[j] - H, e = i > olo ? (long long)E[i - 1] : none_above;
            const bool top = t > e || (t == e && k == 1);
            st.next = top ? 2 * j : 2 * (i - 1) + 1;
            st.y1 = (int)((t > e ? t : e) - cb);
            return st;
        }
        const unsigned int n1 = ne ? j + 1 : j;                                          // south: the next piece of column c + 1 below row a
        const long long s = n1 < nhi ? (long long)S[n1] - H : none_below;
        const bool top = s < B || (s == B && k == 2);
        st.next = top ? 2 * n1 : 2 * i + 1;
        st.y1 = (int)((s < B ? s : B) - cb);
        return st;
    }
    const bool has = q > 0;                                                              // bottom edge, head (c, b)
    const unsigned int nlo = has ? col[mk.col0 + (unsigned)q - 1] : 0u, nhi = has ? col[mk.col0 + (unsigned)q] : 0u;
    const unsigned int j = ct_first_ending_after(E, nlo, nhi, B - 1 - H);                // the piece that holds row b - 1 of column c - 1, or the next one
    const bool nw = j < nhi && (long long)S[j] <= B - 1 - H;
    const bool sw = j < nhi && (nw ? (long long)E[j] > B - H : (long long)S[j] == B - H);
    st.x = c; st.y0 = (int)(B - cb);
    if (nw && !sw) { st.next = 2 * j + 1; st.turn = 0; st.y1 = st.y0; return st; }
    if (sw && (nw || k == 2)) {                                                          // south
        const long long e = (long long)E[j] + H, s = i + 1 < ohi ? (long long)S[i + 1] : none_below;
        const bool bottom = e < s || (e == s && k == 1);
        st.next = bottom ? 2 * j + 1 : 2 * (i + 1);
        st.y1 = (int)((e < s ? e : s) - cb);
        return st;
    }
    const long long e = j > nlo ? (long long)E[j - 1] + H : none_above;                  // north: the last piece of column c - 1 above row b
    const bool bottom = e > A || (e == A && k == 2);
    st.next = bottom ? 2 * (j - 1) + 1 : 2 * i;
    st.y1 = (int)((e > A ? e : A) - cb);
    return st;
}

// what a turn adds to its ring's sums: twice the area is 2 * sum x * (y1 - y0) over the vertical segments (the shoelace sum of a rectilinear
// ring: its horizontal segments add nothing), the crack length is the vertical lengths plus one per node
AMP_HD long long ct_area2(const CtStep& s) { return 2ll * s.x * (long long)(s.y1 - s.y0); }
AMP_HD long long ct_vlen(const CtStep& s) { return s.y1 > s.y0 ? s.y1 - s.y0 : s.y0 - s.y1; }
// a corner as one word for an integer min: by x, then y (x, y <= 32768)
AMP_HD unsigned int ct_key(int x, int y) { return ((unsigned int)x << 16) | (unsigned int)y; }

#define AMP_CONTOUR_MAX_ITEMS (1ull << 29)       // node numbers stay below 2^30, corner numbers and so every ring_len below 2^31

// contours_host.hip: the argument check builds the plan; both paths report the counts they need through contours_capacity before they write
// anything else
int contours_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int connectivity,
                   const unsigned long long* ring_first, const unsigned long long* ring_off, const int* ring_len, const long long* ring_area2,
                   const long long* ring_length, const int* xy, const unsigned long long* need, RunPlan& runs);
int contours_capacity(unsigned long long vertices, unsigned long long rings, unsigned long long xy_cap, unsigned long long ring_cap,
                      unsigned long long* need);
int contours_host(const MpItems& it, int h, int connectivity, unsigned long long* ring_first, unsigned long long* ring_off, int* ring_len,
                  long long* ring_area2, long long* ring_length, unsigned long long ring_cap, int* xy, unsigned long long xy_cap,
                  unsigned long long* need);

}  // namespace amp
