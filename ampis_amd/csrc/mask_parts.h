// amp_mask_parts: what the host evaluation (mask_parts_host.hip) and the device kernels (mask_parts.hip) share -- the ITEMS of a pool of
// masks and the rules on them.  Plain C++ that also compiles under g++ (the host-only sanitizer build), integers throughout.
//
// An item is a vertical piece [S, E) of one column of the column-major image, col * h + row.  Per mask, in column-major order:
//   colour 1  the runs of ones of the plan cut at column ends, adjacent pieces of one column joined: every item is a COMPONENT item;
//   colour 0  every column of the tight box cut into its pieces, alternately zeros and ones: the gaps are the COMPONENT items, the pieces of
//             ones are FILL items that only take part in the emission.  Whole empty columns are one gap;
//   and one END item S = E = h * w that closes the mask, so every mask has an item and the closing count needs no special case.
// Components are the sets of COMPONENT items united across neighbouring columns of one mask.  A component of colour 0 that touches the
// border rows or columns of the tight box is the outside, not a hole.  The emission walks the items of a mask in order with a value each
// (mp_value) and writes a boundary wherever the value changes between neighbours that meet (E of one = S of the next).
#pragma once
#include "run_list.h"

namespace amp {

enum MpKind : uint8_t { MP_FILL = 0, MP_COMPONENT = 1, MP_END = 2 };

struct MpMask {
    int r0, c0, H, W;             // the tight box; H = W = 0 for an empty mask
    unsigned int col0;            // col[col0 + q] = the first item of box column q, col[col0 + W] = the END item
    unsigned int pad;
};

struct MpItems {
    std::vector<uint32_t> S, E;
    std::vector<uint8_t> T;       // MpKind
    std::vector<uint32_t> col;
    std::vector<u64> first;       // [n + 1]: the items of mask m are [first[m], first[m + 1]); the last one is its END item
    std::vector<MpMask> m;
};

// The items of every mask of the plan.  false: more than 2^31 - 1 of them.
inline bool mp_build_items(const RunPlan& pl, int h, int w, int colour, MpItems& it) {
    const size_t n = pl.m.size();
    const uint32_t image = (uint32_t)((u64)h * (u64)w), uh = (uint32_t)h;
    it.S.clear(); it.E.clear(); it.T.clear(); it.col.clear();
    it.first.assign(n + 1, 0); it.m.assign(n, MpMask{0, 0, 0, 0, 0, 0});
    for (size_t p = 0; p < n; ++p) {
        const RunMask& mk = pl.m[p];
        MpMask& e = it.m[p];
        e.r0 = mk.r0; e.c0 = mk.c0; e.H = mk.r1 - mk.r0; e.W = mk.c1 - mk.c0;
        e.col0 = (unsigned int)it.col.size();
        it.first[p] = it.S.size();
        it.col.resize(it.col.size() + (size_t)e.W + 1, 0u);
        int q = 0;                                // the box column being filled
        uint32_t pos = 0;                         // colour 0: everything of column q above pos is written
        auto open_column = [&]() {
            it.col[e.col0 + (size_t)q] = (uint32_t)it.S.size();
            pos = (uint32_t)(e.c0 + q) * uh + (uint32_t)e.r0;
        };
        auto close_column = [&]() {               // colour 0: the gap down to the box's last row
            const uint32_t end = (uint32_t)(e.c0 + q) * uh + (uint32_t)mk.r1;
            if (colour == 0 && pos < end) { it.S.push_back(pos); it.E.push_back(end); it.T.push_back(MP_COMPONENT); }
        };
        auto piece = [&](uint32_t a, uint32_t b) {            // ones [a, b) of one column, in ascending order
            const int c = (int)(a / uh);
            while (e.c0 + q < c) { close_column(); ++q; open_column(); }     // ends: q grows to c - c0 < W
            if (colour == 0 && pos < a) { it.S.push_back(pos); it.E.push_back(a); it.T.push_back(MP_COMPONENT); }
            it.S.push_back(a); it.E.push_back(b); it.T.push_back(colour ? MP_COMPONENT : MP_FILL);
            pos = b;
        };
        if (mk.n > 0) {
            open_column();
            uint32_t pa = 0, pb = 0;              // the piece not yet written: later pieces of its column may still join it
            for (int k = 0; k < mk.n; ++k) {
                const uint32_t s = pl.S[mk.ro + k], t = pl.E[mk.ro + k];
                for (uint32_t c = s / uh; c <= (t - 1) / uh; ++c) {          // ends: c grows to the run's last column
                    const uint32_t a = s > c * uh ? s : c * uh, b = t < (c + 1) * uh ? t : (c + 1) * uh;
                    if (pb > pa && pb == a && a % uh != 0) { pb = b; continue; }         // a zero-length run of zeros lay between them
                    if (pb > pa) piece(pa, pb);
                    pa = a; pb = b;
                }
            }
            if (pb > pa) piece(pa, pb);
            close_column();                       // the ones reach the last box column, so q = W - 1 here
            ++q;
        }
        it.col[e.col0 + (size_t)e.W] = (uint32_t)it.S.size();
        it.S.push_back(image); it.E.push_back(image); it.T.push_back(MP_END);
        if (it.S.size() >= (1ull << 31)) return false;
    }
    it.first[n] = it.S.size();
    return true;
}

// how far apart the rows of two COMPONENT items of neighbouring columns may be: 1 where diagonal neighbours count (ones at connectivity 2,
// zeros -- the dual neighbourhood -- at connectivity 1)
AMP_HD int mp_reach(int colour, int connectivity) { return (colour == 1) == (connectivity == 2) ? 1 : 0; }

// does the gap [s, e) of box column q touch the border of the tight box?
AMP_HD bool mp_touches(const MpMask& mk, int h, unsigned int s, unsigned int e) {
    const unsigned int cb = s / (unsigned)h * (unsigned)h;
    const int q = (int)(s / (unsigned)h) - mk.c0;
    return q == 0 || q == mk.W - 1 || s == cb + (unsigned)mk.r0 || e == cb + (unsigned)(mk.r0 + mk.H);
}

// a mask's best component as one word for an integer max: the largest area, among equals the smallest root -- the component whose first
// pixel comes first in column-major order
AMP_HD u64 mp_best_key(unsigned int area, unsigned int root) { return ((u64)area << 32) | (u64)(0xffffffffu - root); }
AMP_HD unsigned int mp_best_root(u64 key) { return 0xffffffffu - (unsigned int)(key & 0xffffffffu); }

// is the component flipped?  counts: colour 0 only, false for the outside
AMP_HD bool mp_flip(int colour, bool counts, unsigned int area, unsigned int root, u64 best, unsigned int threshold, int keep_largest) {
    if (colour == 0) return counts && area < threshold;
    return (keep_largest && root != mp_best_root(best)) || area < threshold;
}

// the value of an item in the result: a kept part or a filled hole is 1, a FILL item is 1, the END item 0
AMP_HD int mp_value(int kind, int colour, bool flip) { return kind == MP_COMPONENT ? (colour ? !flip : flip) : kind == MP_FILL ? 1 : 0; }

// The boundaries item j writes, given its neighbours inside the mask (has_prev false for a mask's first item; an item that is not the END
// item has a next one).  Two pieces of ones are joined where they meet.  The END item writes the closing h * w unless the ones reach it.
struct MpBounds { bool s, e; };
AMP_HD MpBounds mp_bounds(int kind, int v, unsigned int s, unsigned int e, bool has_prev, int v_prev, unsigned int e_prev, int v_next,
                          unsigned int s_next) {
    MpBounds b;
    const bool joined = has_prev && v_prev && e_prev == s;
    if (kind == MP_END) { b.s = !joined; b.e = false; return b; }
    b.s = v && !joined;
    b.e = v && !(v_next && s_next == e);
    return b;
}

// mask_parts_host.hip: the argument check builds the plan; both paths report the counts they need through mask_parts_capacity before they
// write anything else
int mask_parts_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int colour, int connectivity,
                     int keep_largest, const unsigned long long* stats, const uint32_t* out_pool, const unsigned long long* out_off,
                     const int* out_len, const unsigned long long* need, RunPlan& runs);
int mask_parts_capacity(unsigned long long counts, unsigned long long out_cap, unsigned long long* need);
int mask_parts_host(const MpItems& it, int h, int colour, int connectivity, unsigned int threshold, int keep_largest,
                    unsigned long long* stats, uint32_t* out_pool, unsigned long long out_cap, unsigned long long* out_off, int* out_len,
                    unsigned long long* need);

}  // namespace amp
