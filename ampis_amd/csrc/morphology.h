// amp_mask_morphology: what the host sweep (morphology_host.hip) and the device kernels (morphology.hip) share -- the RUNS of a pool of masks
// and the rules on them.  Plain C++ that also compiles under g++ (the host-only sanitizer build), integers throughout.
//
// A run is a maximal run of ones [S, E) of the column-major image, col * h + row: the runs of the plan with neighbours joined where a
// zero-length run of zeros lay between them, so a run is cut into PIECES -- maximal vertical runs of one column -- at the column ends it crosses
// and nowhere else.  One PASS turns the runs of every mask into the boundaries of its result: piece [s, e) of column x sends to every output
// column x + dx inside the image (|dx| <= r) the interval mo_interval gives at the half height hh[|dx|] with weight 1, in a band also itself to
// its own column with weight MO_OWN; the cover of a pixel is the sum of the weights of the intervals that hold it, and mo_class tells from the
// cover and the threshold mo_threshold of the pixel's column whether the pixel is set.  A boundary lies wherever the class changes between
// neighbours in column-major order, except at h * w.  All intervals stay inside one column, so the cover is 0 wherever a column starts with
// nothing open.  DILATE, ERODE, BAND_IN and BAND_OUT are one pass; OPEN is the pass ERODE, then DILATE on its result; CLOSE is DILATE, then
// ERODE.
//
// MO_OWN is 2^32 and the cover a 64-bit integer: the grown pieces of one source column may overlap, so a dilation's cover is bounded only by
// the events of the call (below 2^31), and a weight of 2^16 could be reached without the mask's own piece.
#pragma once
#include "../../include/ampis_hip.h"
#include "run_list.h"

namespace amp {

constexpr long long MO_OWN = 1ll << 32;
#define AMP_MORPH_MAX_EVENTS (1ull << 31)

struct MoRuns {
    std::vector<uint32_t> S, E;   // the runs of all masks, mask after mask
    std::vector<u64> first;       // [n + 1]: the runs of mask m are [first[m], first[m + 1])
};

// the half heights hh[0 .. r] of the structuring element by |dx|
inline void mo_half_heights(int shape, int r, std::vector<int>& hh) {
    hh.assign((size_t)r + 1, r);
    for (int d = 0; d <= r; ++d) {
        if (shape == AMP_MORPH_DIAMOND) hh[(size_t)d] = r - d;
        if (shape != AMP_MORPH_DISK) continue;
        const long long v = (long long)r * r - (long long)d * d;
        long long t = 0;
        while ((t + 1) * (t + 1) <= v) ++t;                                              // ends: t grows to isqrt(v) <= r
        hh[(size_t)d] = (int)t;
    }
}

// the first of an opening's or closing's two passes and the second (-1: there is none)
AMP_HD int mo_first_pass(int op) { return op == AMP_MORPH_OPEN ? AMP_MORPH_ERODE : op == AMP_MORPH_CLOSE ? AMP_MORPH_DILATE : op; }
AMP_HD int mo_second_pass(int op) { return op == AMP_MORPH_OPEN ? AMP_MORPH_DILATE : op == AMP_MORPH_CLOSE ? AMP_MORPH_ERODE : -1; }
AMP_HD bool mo_is_band(int pass) { return pass == AMP_MORPH_BAND_IN || pass == AMP_MORPH_BAND_OUT; }
AMP_HD bool mo_grows(int pass) { return pass == AMP_MORPH_DILATE || pass == AMP_MORPH_BAND_OUT; }

// the columns col + dx, |dx| <= r, inside an image of w columns (0 <= col < w)
AMP_HD int mo_offsets(int col, int r, int w) { return (col + r < w - 1 ? col + r : w - 1) - (col - r > 0 ? col - r : 0) + 1; }

// the cover at which a pixel of column col survives an erosion; col == w (the position h * w, where the cover is 0) never reaches it
AMP_HD long long mo_threshold(int col, int r, int w, int border) { return border && col < w ? mo_offsets(col, r, w) : 2ll * r + 1; }

// is a pixel of cover `cover` set, K = mo_threshold of its column?  Never at cover 0.
AMP_HD bool mo_class(int pass, long long cover, long long K) {
    if (pass == AMP_MORPH_DILATE) return cover >= 1;
    if (pass == AMP_MORPH_ERODE) return cover == K;
    if (pass == AMP_MORPH_BAND_IN) return cover >= MO_OWN && cover - MO_OWN != K;
    return cover >= 1 && cover < MO_OWN;
}

// the rows [*a, *b) that the piece [s, e) of a column of height h sends to a column at half height hh; false: none
AMP_HD bool mo_interval(int pass, int border, int h, int s, int e, int hh, int* a, int* b) {
    if (mo_grows(pass)) {
        *a = s - hh > 0 ? s - hh : 0;
        *b = e + hh < h ? e + hh : h;
        return true;
    }
    *a = border && s == 0 ? s : s + hh;
    *b = border && e == h ? e : e - hh;
    return *a < *b;
}

// morphology_host.hip: the argument check builds the runs; both paths report the counts they need through morphology_capacity before they
// write anything else
int morphology_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int op, int shape, int radius,
                     int border_value, const uint32_t* out_pool, const unsigned long long* out_off, const int* out_len, const long long* boxes,
                     const unsigned long long* areas, const unsigned long long* need, MoRuns& runs);
int morphology_capacity(unsigned long long counts, unsigned long long out_cap, unsigned long long* need);
int morphology_events(unsigned long long events, int pass_index);
int morphology_host(const MoRuns& runs, int n, int h, int w, int op, int shape, int radius, int border_value, uint32_t* out_pool,
                    unsigned long long out_cap, unsigned long long* out_off, int* out_len, long long* boxes, unsigned long long* areas,
                    unsigned long long* need);

}  // namespace amp
