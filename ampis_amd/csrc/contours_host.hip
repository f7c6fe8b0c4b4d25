// Host side of amp_mask_contours (contours.h): the argument check, whose plan both paths evaluate, the capacity report, and the evaluation with a
// NULL context -- the boundary rings of every mask of a pool as corner lists on pixel corners.  A sequential walk of the successor function of
// contours.h over the nodes of each mask: every node not yet seen starts a ring, the walk collects the corners of its turns until it is back,
// the ring is turned so that its smallest corner comes first, and the rings of a mask are sorted by that corner.  Plain C++ throughout,
// integers only: the host-only sanitizer build of tests/sanitize compiles this file with g++.  contours.hip computes the same bytes on the device.
#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "contours.h"

namespace amp {

int contours_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int connectivity,
                   const unsigned long long* ring_first, const unsigned long long* ring_off, const int* ring_len, const long long* ring_area2,
                   const long long* ring_length, const int* xy, const unsigned long long* need, RunPlan& runs) {
    AMP_REQUIRE(n >= 0, "amp_mask_contours: n = %d", n);
    AMP_TRY_STATUS(require_image_size("amp_mask_contours", h, w));
    AMP_REQUIRE(connectivity == 1 || connectivity == 2, "amp_mask_contours: connectivity = %d (1: 4 neighbours, 2: 8 neighbours)", connectivity);
    AMP_REQUIRE(n == 0 || (pool && off && len), "amp_mask_contours: null argument %s", !pool ? "pool" : !off ? "off" : "len");
    AMP_REQUIRE(ring_first && ring_off && ring_len && ring_area2 && ring_length && xy && need, "amp_mask_contours: null argument %s",
                !ring_first ? "ring_first" : !ring_off ? "ring_off" : !ring_len ? "ring_len" : !ring_area2 ? "ring_area2"
                : !ring_length ? "ring_length" : !xy ? "xy" : "need");
    AMP_TRY_STATUS(plan_pool("amp_mask_contours", pool, off, len, n, h, w, runs));
    return AMP_OK;
}

int contours_capacity(unsigned long long vertices, unsigned long long rings, unsigned long long xy_cap, unsigned long long ring_cap,
                      unsigned long long* need) {
    need[0] = vertices; need[1] = rings;
    if (vertices > xy_cap || rings > ring_cap) {
        set_error("amp_mask_contours: xy_cap = %llu, ring_cap = %llu; %llu vertices in %llu rings are needed", xy_cap, ring_cap, vertices, rings);
        return AMP_ERR_NOMEM;
    }
    return AMP_OK;
}

namespace {
struct HostRing {
    unsigned int key;             // ct_key of the first corner
    size_t at, len;               // its corners in the mask's list, as x, y pairs
    long long area2, length;
};
}  // namespace

int contours_host(const MpItems& it, int h, int connectivity, unsigned long long* ring_first, unsigned long long* ring_off, int* ring_len,
                  long long* ring_area2, long long* ring_length, unsigned long long ring_cap, int* xy, unsigned long long xy_cap,
                  unsigned long long* need) {
    const size_t n = it.m.size(), R = it.S.size();
    const uint32_t *S = it.S.data(), *E = it.E.data(), *col = it.col.data();
    std::vector<uint8_t> seen(2 * R, 0);
    std::vector<int> out, ring;                   // every ring's corners in its final order, mask after mask; the ring being walked
    std::vector<HostRing> rings, mine;
    std::vector<unsigned long long> first(n + 1, 0ull);
    for (size_t p = 0; p < n; ++p) {
        const MpMask& mk = it.m[p];
        mine.clear();
        std::vector<int> tmp;                     // the mask's rings in the order they are found
        for (size_t v0 = 2 * (size_t)it.first[p]; v0 + 2 < 2 * (size_t)it.first[p + 1]; ++v0) {      // the mask's last item is its END item
            if (seen[v0]) continue;
            ring.clear();
            HostRing r{0u, tmp.size() / 2, 0, 0, 0};
            unsigned int v = (unsigned int)v0;
            do {                                  // ends: the successor is a permutation of the mask's live nodes, so the walk returns to v0
                seen[v] = 1;
                const CtStep s = ct_successor(S, E, col, mk, h, connectivity, v);
                r.length += 1;
                if (s.turn) {
                    ring.push_back(s.x); ring.push_back(s.y0); ring.push_back(s.x); ring.push_back(s.y1);
                    r.area2 += ct_area2(s);
                    r.length += ct_vlen(s);
                }
                v = s.next;
            } while (v != (unsigned int)v0);
            const size_t k = ring.size() / 2;
            size_t best = 0;
            for (size_t j = 1; j < k; ++j)
                if (ct_key(ring[2 * j], ring[2 * j + 1]) < ct_key(ring[2 * best], ring[2 * best + 1])) best = j;
            r.key = ct_key(ring[2 * best], ring[2 * best + 1]);
            r.len = k;
            for (size_t j = 0; j < k; ++j) {
                const size_t src = (best + j) % k;
                tmp.push_back(ring[2 * src]); tmp.push_back(ring[2 * src + 1]);
            }
            mine.push_back(r);
        }
        std::sort(mine.begin(), mine.end(), [](const HostRing& a, const HostRing& b) { return a.key < b.key; });     // the keys of a mask differ
        for (const HostRing& r : mine) {
            HostRing o = r;
            o.at = out.size() / 2;
            out.insert(out.end(), tmp.begin() + 2 * (ptrdiff_t)r.at, tmp.begin() + 2 * (ptrdiff_t)(r.at + r.len));
            rings.push_back(o);
        }
        first[p + 1] = rings.size();
    }
    AMP_TRY_STATUS(contours_capacity(out.size() / 2, rings.size(), xy_cap, ring_cap, need));
    std::copy(first.begin(), first.end(), ring_first);
    std::copy(out.begin(), out.end(), xy);
    for (size_t r = 0; r < rings.size(); ++r) {
        ring_off[r] = rings[r].at; ring_len[r] = (int)rings[r].len; ring_area2[r] = rings[r].area2; ring_length[r] = rings[r].length;
    }
    return AMP_OK;
}

}  // namespace amp
