// Host side of amp_flatten_instances (flatten.h): the argument check, whose plan and priority order both paths evaluate, the capacity report,
// and the evaluation with a NULL context -- the owner of every pixel among overlapping run-list masks, per instance the run list of the pixels
// it owns, the label image and the statistics.  One sweep over the column-major positions:
//   events   every run [s, e) of the instance at place p of the priority order opens at s and closes at e; the events are sorted by position;
//   sweep    between two neighbouring event positions the set of covering instances is constant: the segment's owner is the smallest place in
//            the set, its pixels go to pixels[min(covering, 2)], to the owner's area and box, and its ends to the owner's boundary list, joined
//            with the segment before where they meet (also across a column end, as amp_rle_encode joins);
//   emit     per instance the differences of its boundaries as counts, the closing h * w unless the ones reach it; the single run h * w for
//            an instance that owns nothing.
// Memory is linear in the runs (and the label image when it is asked for); no dense mask per instance.  Plain C++ throughout, integers
// only: the host-only sanitizer build of tests/sanitize compiles this file with g++.  flatten.hip computes the same bytes on the device.
#include <algorithm>
#include <set>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "flatten.h"

namespace amp {

int flatten_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const uint32_t* rank,
                  const uint32_t* counts, unsigned long long counts_cap, const unsigned long long* counts_off, const int* counts_len,
                  const unsigned long long* stats, const int* boxes, const unsigned long long* pixels, const unsigned long long* need,
                  RunPlan& runs, std::vector<int>& order) {
    AMP_REQUIRE(n >= 0, "amp_flatten_instances: n = %d", n);
    AMP_TRY_STATUS(require_image_size("amp_flatten_instances", h, w));
    AMP_REQUIRE(pixels, "amp_flatten_instances: null argument pixels");
    AMP_REQUIRE(n == 0 || (pool && off && len && stats && boxes), "amp_flatten_instances: null argument %s",
                !pool ? "pool" : !off ? "off" : !len ? "len" : !stats ? "stats" : "boxes");
    AMP_REQUIRE(!counts || n == 0 || (counts_off && counts_len), "amp_flatten_instances: null argument %s",
                !counts_off ? "counts_off" : "counts_len");
    AMP_REQUIRE(!counts || need, "amp_flatten_instances: null argument need");
    AMP_REQUIRE(counts || counts_cap == 0, "amp_flatten_instances: counts_cap = %llu with counts NULL (no list is emitted)", counts_cap);
    AMP_TRY_STATUS(plan_pool("amp_flatten_instances", pool, off, len, n, h, w, runs));
    flatten_order(rank, n, order);
    return AMP_OK;
}

int flatten_capacity(unsigned long long counts, unsigned long long counts_cap, unsigned long long* need) {
    return counts_capacity("amp_flatten_instances", "counts_cap", counts, counts_cap, need);
}

int flatten_host(const RunPlan& runs, const std::vector<int>& order, int h, int w, int* labels, uint32_t* counts, unsigned long long counts_cap,
                 unsigned long long* counts_off, int* counts_len, unsigned long long* stats, int* boxes, unsigned long long* pixels,
                 unsigned long long* need) {
    const size_t n = runs.m.size();
    const uint32_t image = (uint32_t)((u64)h * (u64)w), uh = (uint32_t)h;
    // an event: position << 32 | place << 1 | opens.  At one position a place's closing event sorts before its opening one, so a mask whose
    // runs meet (a zero-length run of zeros between them) stays in the set.
    std::vector<u64> ev;
    for (size_t p = 0; p < n; ++p) {
        const RunMask& mk = runs.m[(size_t)order[p]];
        for (int k = 0; k < mk.n; ++k) {
            ev.push_back(((u64)runs.S[mk.ro + k] << 32) | ((u64)p << 1) | 1ull);
            ev.push_back(((u64)runs.E[mk.ro + k] << 32) | ((u64)p << 1));
        }
    }
    std::sort(ev.begin(), ev.end());

    struct Seg { uint32_t s, e; int owner; };
    std::vector<Seg> segs;                        // the owned segments, only for the label image
    std::vector<std::vector<uint32_t>> bnd(counts ? n : 0);
    std::vector<unsigned long long> owned(n, 0ull), px(3, 0ull);
    std::vector<int> box(4 * n, 0);
    std::set<uint32_t> active;                    // the places of the instances that cover the current position
    uint32_t x = 0;
    for (size_t i = 0; i < ev.size();) {
        const uint32_t y = (uint32_t)(ev[i] >> 32);
        if (y > x) {
            px[active.size() < 2 ? active.size() : 2] += y - x;
            if (!active.empty()) {
                const int o = order[*active.begin()];
                const int cf = (int)(x / uh), cl = (int)((y - 1) / uh);
                const int ra = cf == cl ? (int)(x % uh) : 0, rb = cf == cl ? (int)((y - 1) % uh) + 1 : h;      // across a column end: the last and the first row
                int* b = &box[4 * (size_t)o];
                if (owned[(size_t)o] == 0) { b[0] = ra; b[1] = cf; b[2] = rb; b[3] = cl + 1; }
                else { b[0] = std::min(b[0], ra); b[1] = std::min(b[1], cf); b[2] = std::max(b[2], rb); b[3] = std::max(b[3], cl + 1); }
                owned[(size_t)o] += y - x;
                if (counts) {
                    std::vector<uint32_t>& v = bnd[(size_t)o];
                    if (!v.empty() && v.back() == x) v.back() = y; else { v.push_back(x); v.push_back(y); }
                }
                if (labels) {
                    if (!segs.empty() && segs.back().owner == o && segs.back().e == x) segs.back().e = y; else segs.push_back(Seg{x, y, o});
                }
            }
            x = y;
        }
        for (; i < ev.size() && (uint32_t)(ev[i] >> 32) == y; ++i) {                     // ends: i grows
            const uint32_t p = (uint32_t)(ev[i] & 0xffffffffull) >> 1;
            if (ev[i] & 1ull) active.insert(p); else active.erase(p);
        }
    }
    px[0] += image - x;                           // behind the last event nothing is covered

    unsigned long long total = 0;
    if (counts) {
        for (size_t i = 0; i < n; ++i) total += bnd[i].empty() ? 1 : bnd[i].size() + (bnd[i].back() != image ? 1 : 0);
        AMP_TRY_STATUS(flatten_capacity(total, counts_cap, need));
        unsigned long long at = 0;
        for (size_t i = 0; i < n; ++i) {
            counts_off[i] = at;
            uint32_t prev = 0;
            for (uint32_t b : bnd[i]) { counts[at++] = b - prev; prev = b; }
            if (bnd[i].empty() || prev != image) counts[at++] = image - prev;
            counts_len[i] = (int)(at - counts_off[i]);
        }
    }
    for (size_t i = 0; i < n; ++i) {
        stats[2 * i] = runs.m[i].area;
        stats[2 * i + 1] = owned[i];
        for (int k = 0; k < 4; ++k) boxes[4 * i + k] = box[4 * i + k];
    }
    for (int k = 0; k < 3; ++k) pixels[k] = px[(size_t)k];
    if (labels) {
        std::fill(labels, labels + (size_t)image, 0);
        for (const Seg& s : segs) {
            size_t r = s.s % uh, c = s.s / uh;
            for (uint32_t q = s.s; q < s.e; ++q) {                                       // ends: q grows to the segment's end
                labels[r * (size_t)w + c] = s.owner + 1;
                if (++r == uh) { r = 0; ++c; }
            }
        }
    }
    return AMP_OK;
}

}  // namespace amp
