// Host side of amp_mask_morphology (morphology.h): the argument check, whose runs both paths evaluate, the capacity and the event reports, and
// the evaluation with a NULL context.  Per mask and pass a sweep over the output columns: the intervals that the pieces of the source columns
// x - dx send to column x are gathered as (row, weight) events, sorted by row and summed; where the class of the cover changes a boundary is
// toggled.  A column that ends set and a next one that starts set toggle the same position twice, which cancels, so the runs come out joined
// across column ends as amp_rle_encode writes them.  The buffers are kept from column to column and from mask to mask: nothing is allocated
// per pixel.  Box and area come from run_list.h's walk over the finished list.  Plain C++ throughout, integers only: the host-only sanitizer
// build of tests/sanitize compiles this file with g++.  morphology.hip computes the same bytes on the device.
#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "morphology.h"

namespace amp {

int morphology_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int op, int shape, int radius,
                     int border_value, const uint32_t* out_pool, const unsigned long long* out_off, const int* out_len, const long long* boxes,
                     const unsigned long long* areas, const unsigned long long* need, MoRuns& runs) {
    AMP_REQUIRE(n >= 0, "amp_mask_morphology: n = %d", n);
    AMP_TRY_STATUS(require_image_size("amp_mask_morphology", h, w));
    AMP_REQUIRE(op >= AMP_MORPH_DILATE && op <= AMP_MORPH_BAND_OUT, "amp_mask_morphology: op = %d (0 dilate, 1 erode, 2 open, 3 close, 4 inner band, 5 outer band)", op);
    AMP_REQUIRE(shape >= AMP_MORPH_SQUARE && shape <= AMP_MORPH_DISK, "amp_mask_morphology: shape = %d (0 square, 1 diamond, 2 disk)", shape);
    AMP_REQUIRE(border_value == 0 || border_value == 1, "amp_mask_morphology: border_value = %d (0 or 1)", border_value);
    AMP_REQUIRE(radius >= 0 && radius <= AMP_MORPH_MAX_RADIUS, "amp_mask_morphology: radius = %d (0 .. %d)", radius, AMP_MORPH_MAX_RADIUS);
    AMP_REQUIRE(need, "amp_mask_morphology: null argument need");
    AMP_REQUIRE(n == 0 || (pool && off && len && out_pool && out_off && out_len && boxes && areas), "amp_mask_morphology: null argument %s",
                !pool ? "pool" : !off ? "off" : !len ? "len" : !out_pool ? "out_pool" : !out_off ? "out_off" : !out_len ? "out_len" : !boxes ? "boxes" : "areas");
    RunPlan plan;
    AMP_TRY_STATUS(plan_pool("amp_mask_morphology", pool, off, len, n, h, w, plan));
    runs.S.clear(); runs.E.clear();
    runs.first.assign((size_t)n + 1, 0);
    const int pass = mo_first_pass(op);
    unsigned long long events = 0;
    for (int p = 0; p < n; ++p) {
        const RunMask& mk = plan.m[(size_t)p];
        runs.first[(size_t)p] = runs.S.size();
        for (int k = 0; k < mk.n; ++k) {
            const uint32_t s = plan.S[mk.ro + (size_t)k], e = plan.E[mk.ro + (size_t)k];
            if (k > 0 && runs.E.back() == s) { runs.E.back() = e; continue; }            // a zero-length run of zeros lay between them
            runs.S.push_back(s); runs.E.push_back(e);
        }
        for (size_t j = (size_t)runs.first[(size_t)p]; j < runs.S.size(); ++j)
            for (int c = (int)(runs.S[j] / (unsigned)h); c <= (int)((runs.E[j] - 1) / (unsigned)h); ++c) {      // ends: c grows to the run's last column
                events += 2ull * (unsigned long long)(mo_offsets(c, radius, w) + (mo_is_band(pass) ? 1 : 0));
                AMP_REQUIRE(events < AMP_MORPH_MAX_EVENTS,
                            "amp_mask_morphology: the call has 2^31 events or more by mask %d (2 x the output columns inside the image of every piece, at most 2^31 - 1)", p);
            }
    }
    runs.first[(size_t)n] = runs.S.size();
    return AMP_OK;
}

int morphology_capacity(unsigned long long counts, unsigned long long out_cap, unsigned long long* need) {
    return counts_capacity("amp_mask_morphology", "out_cap", counts, out_cap, need);
}

int morphology_events(unsigned long long events, int pass_index) {
    AMP_REQUIRE(events < AMP_MORPH_MAX_EVENTS, "amp_mask_morphology: pass %d of the call emits %llu events (at most 2^31 - 1)", pass_index, events);
    return AMP_OK;
}

namespace {

struct MoPiece { int col, s, e; };

struct MoScratch {
    std::vector<MoPiece> pieces;                          // the pieces of one mask, by column
    std::vector<size_t> colfirst;                         // [columns + 1]: where the pieces of every column of the mask's column range start
    std::vector<std::pair<int, long long>> ev;            // the events of one output column: (row, weight)
};

// One pass over the runs [S[j], E[j]), j < k, of one mask: bnd = the boundaries of the result, ascending, none at h * w.  *events grows by
// the events the pass emits.
void pass_mask(const uint32_t* S, const uint32_t* E, size_t k, int h, int w, int pass, int r, int border, const int* hh, MoScratch& sc,
               std::vector<uint32_t>& bnd, unsigned long long* events) {
    bnd.clear();
    if (k == 0) return;
    sc.pieces.clear();
    const int c_lo = (int)(S[0] / (unsigned)h), c_hi = (int)((E[k - 1] - 1) / (unsigned)h);
    sc.colfirst.assign((size_t)(c_hi - c_lo) + 2, 0);
    for (size_t j = 0; j < k; ++j) {
        const int cf = (int)(S[j] / (unsigned)h), cl = (int)((E[j] - 1) / (unsigned)h);
        for (int c = cf; c <= cl; ++c) {                                                 // ends: c grows to the run's last column
            const long long cb = (long long)c * h;
            sc.pieces.push_back(MoPiece{c, c == cf ? (int)(S[j] - cb) : 0, c == cl ? (int)(E[j] - cb) : h});
            ++sc.colfirst[(size_t)(c - c_lo) + 1];
        }
    }
    for (size_t q = 1; q < sc.colfirst.size(); ++q) sc.colfirst[q] += sc.colfirst[q - 1];
    auto toggle = [&](uint32_t p) { if (!bnd.empty() && bnd.back() == p) bnd.pop_back(); else bnd.push_back(p); };
    const int x_lo = std::max(c_lo - r, 0), x_hi = std::min(c_hi + r, w - 1);
    for (int x = x_lo; x <= x_hi; ++x) {
        sc.ev.clear();
        for (int c = std::max(x - r, c_lo); c <= std::min(x + r, c_hi); ++c) {
            const int d = c > x ? c - x : x - c;
            for (size_t i = sc.colfirst[(size_t)(c - c_lo)]; i < sc.colfirst[(size_t)(c - c_lo) + 1]; ++i) {
                int a, b;
                if (!mo_interval(pass, border, h, sc.pieces[i].s, sc.pieces[i].e, hh[d], &a, &b)) continue;
                sc.ev.emplace_back(a, 1ll); sc.ev.emplace_back(b, -1ll);
            }
        }
        if (mo_is_band(pass) && x >= c_lo && x <= c_hi)
            for (size_t i = sc.colfirst[(size_t)(x - c_lo)]; i < sc.colfirst[(size_t)(x - c_lo) + 1]; ++i) {
                sc.ev.emplace_back(sc.pieces[i].s, MO_OWN); sc.ev.emplace_back(sc.pieces[i].e, -MO_OWN);
            }
        *events += sc.ev.size();
        std::sort(sc.ev.begin(), sc.ev.end(), [](const std::pair<int, long long>& p, const std::pair<int, long long>& q) { return p.first < q.first; });
        const long long K = mo_threshold(x, r, w, border);
        long long cover = 0;
        bool cls = false;
        for (size_t i = 0; i < sc.ev.size();) {                                         // ends: i grows by one group of equal rows or more
            const int row = sc.ev[i].first;
            for (; i < sc.ev.size() && sc.ev[i].first == row; ++i) cover += sc.ev[i].second;
            const bool now = mo_class(pass, cover, K);
            if (now != cls) toggle((uint32_t)((long long)x * h + row));
            cls = now;
        }                                                                                // every interval is closed by row h: the cover is 0 again
    }
    if (!bnd.empty() && bnd.back() == (uint32_t)((u64)h * (u64)w)) bnd.pop_back();
}

}  // namespace

int morphology_host(const MoRuns& runs, int n, int h, int w, int op, int shape, int radius, int border_value, uint32_t* out_pool,
                    unsigned long long out_cap, unsigned long long* out_off, int* out_len, long long* boxes, unsigned long long* areas,
                    unsigned long long* need) {
    const uint32_t area = (uint32_t)((u64)h * (u64)w);
    std::vector<int> hh;
    mo_half_heights(shape, radius, hh);
    MoScratch sc;
    std::vector<uint32_t> bnd, S2, E2, out;               // a pass's boundaries, the runs between the passes; the counts of all masks back to back
    std::vector<unsigned long long> offs((size_t)n + 1, 0);
    unsigned long long ev1 = 0, ev2 = 0;
    for (int i = 0; i < n; ++i) {
        const size_t j0 = (size_t)runs.first[(size_t)i], k = (size_t)(runs.first[(size_t)i + 1] - runs.first[(size_t)i]);
        pass_mask(runs.S.data() + j0, runs.E.data() + j0, k, h, w, mo_first_pass(op), radius, border_value, hh.data(), sc, bnd, &ev1);
        if (mo_second_pass(op) >= 0) {
            S2.clear(); E2.clear();
            for (size_t j = 0; j < bnd.size(); j += 2) {
                S2.push_back(bnd[j]); E2.push_back(j + 1 < bnd.size() ? bnd[j + 1] : area);
            }
            pass_mask(S2.data(), E2.data(), S2.size(), h, w, mo_second_pass(op), radius, border_value, hh.data(), sc, bnd, &ev2);
            AMP_TRY_STATUS(morphology_events(ev2, 2));
        }
        offs[(size_t)i] = out.size();
        uint32_t at = 0;
        for (uint32_t b : bnd) { out.push_back(b - at); at = b; }
        out.push_back(area - at);
    }
    offs[(size_t)n] = out.size();
    AMP_TRY_STATUS(morphology_capacity(out.size(), out_cap, need));
    RunPlan pl;
    for (int i = 0; i < n; ++i) {
        out_off[i] = offs[(size_t)i];
        out_len[i] = (int)(offs[(size_t)i + 1] - offs[(size_t)i]);
        pl.reset(1);
        u64 covered = 0;
        const RunListFault f = plan_add_mask(pl, 0, out.data() + offs[(size_t)i], out_len[i], h, w, false, &covered);
        if (f != RUNS_OK) {                       // cannot happen: every list above closes at h * w
            set_error("amp_mask_morphology: the runs of result %d cover %llu of %d x %d pixels", i, covered, h, w);
            return AMP_ERR_ARG;
        }
        const RunMask& m = pl.m[0];
        boxes[4 * i] = m.r0; boxes[4 * i + 1] = m.c0; boxes[4 * i + 2] = m.r1; boxes[4 * i + 3] = m.c1;
        areas[i] = m.area;
    }
    std::copy(out.begin(), out.end(), out_pool);
    return AMP_OK;
}

}  // namespace amp
