// Host-only AddressSanitizer / UBSan run of amp_mask_parts' argument check, item builder and host evaluation (ampis_amd/csrc/mask_parts.h,
// mask_parts_host.hip: amp::mask_parts_check / amp::mp_build_items / amp::mask_parts_host, what the call runs with a NULL context): the hand
// shapes of tests/mask_parts_cases.py restated (one pixel, empty, full, a full 64 x 3 image, rings, a ring in a ring with a speck, a C closed by
// the border, a hole that meets the outside by a corner, checkerboards, serpentine and its complement, a mask on all four borders) and random
// masks at both colours and connectivities, every result compared with a per-pixel flood fill written here, every buffer of exactly the
// capacity asked for, and the refusals.  Built and run by tests/test_mask_parts_sanitize.py like the label-runs run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// what amp_mask_parts does with a NULL context
static int call(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int colour, int conn,
                unsigned int threshold, int keep_largest, unsigned long long* stats, uint32_t* out_pool, unsigned long long out_cap,
                unsigned long long* out_off, int* out_len, unsigned long long* need) {
    amp::RunPlan plan;
    int st = amp::mask_parts_check(pool, off, len, n, h, w, colour, conn, keep_largest, stats, out_pool, out_off, out_len, need, plan);
    if (st != AMP_OK) return st;
    if (n == 0) { if (out_pool) need[0] = 0; return AMP_OK; }
    amp::MpItems items;
    if (!amp::mp_build_items(plan, h, w, colour, items)) return AMP_ERR_ARG;
    return amp::mask_parts_host(items, h, colour, conn, threshold, keep_largest, stats, out_pool, out_cap, out_off, out_len, need);
}

// by definition: the components of colour `colour` by flood fill, holes = components of the zeros with no pixel on the image border; the rule;
// stats {components, pixels, largest, flipped} and the dense result
static void reference(const std::vector<int>& m, int h, int w, int colour, int conn, unsigned int threshold, int keep_largest,
                      unsigned long long stats[4], std::vector<int>* result) {
    const bool diagonal = (colour == 1) == (conn == 2);
    std::vector<int> lab((size_t)h * w, 0), stack;
    std::vector<unsigned int> area(1, 0u), first(1, 0u);
    std::vector<char> outside(1, 0);
    int n = 0;
    for (int x = 0; x < w; ++x)                  // column-major: a component's number follows its first pixel col * h + row
        for (int y = 0; y < h; ++y) {
            const int i = y * w + x;
            if (m[i] != colour || lab[i]) continue;
            lab[i] = ++n;
            area.push_back(0u); first.push_back((unsigned)(x * h + y)); outside.push_back(0);
            stack.assign(1, i);
            while (!stack.empty()) {
                const int p = stack.back(), r = p / w, c = p % w;
                stack.pop_back();
                ++area[n];
                if (r == 0 || r == h - 1 || c == 0 || c == w - 1) outside[n] = 1;
                for (int dr = -1; dr <= 1; ++dr)
                    for (int dc = -1; dc <= 1; ++dc) {
                        if ((!dr && !dc) || (!diagonal && dr && dc)) continue;
                        const int yy = r + dr, xx = c + dc;
                        if (yy < 0 || yy >= h || xx < 0 || xx >= w || m[yy * w + xx] != colour || lab[yy * w + xx]) continue;
                        lab[yy * w + xx] = n;
                        stack.push_back(yy * w + xx);
                    }
            }
        }
    int best = 0;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (int k = 1; k <= n; ++k) {
        if (colour == 0 && outside[k]) continue;
        ++stats[0]; stats[1] += area[k];
        if (area[k] > stats[2]) { stats[2] = area[k]; best = k; }   // numbered by first pixel: the first of equals stays the best
    }
    std::vector<char> flip((size_t)n + 1, 0);
    for (int k = 1; k <= n; ++k) {
        if (colour == 0) flip[k] = !outside[k] && area[k] < threshold;
        else flip[k] = (keep_largest && k != best) || area[k] < threshold;
        if (flip[k]) stats[3] += area[k];
    }
    *result = m;
    for (size_t i = 0; i < m.size(); ++i)
        if (lab[i] && flip[lab[i]]) (*result)[i] = !colour;
}

static int one_case(const std::vector<std::vector<int>>& masks, int h, int w, int colour, int conn, unsigned int threshold, int keep_largest, bool loose) {
    const int n = (int)masks.size();
    std::vector<uint32_t> pool_v;
    std::vector<unsigned long long> off_v;
    std::vector<int> len_v;
    std::vector<std::vector<uint32_t>> want;
    std::vector<unsigned long long> want_stats(4 * (size_t)n);
    for (int p = 0; p < n; ++p) {
        const std::vector<uint32_t> c = encode(masks[p], h, w, loose);
        off_v.push_back(pool_v.size()); len_v.push_back((int)c.size());
        pool_v.insert(pool_v.end(), c.begin(), c.end());
        std::vector<int> res;
        reference(masks[p], h, w, colour, conn, threshold, keep_largest, &want_stats[4 * (size_t)p], &res);
        want.push_back(encode(res, h, w, false));
    }
    // every buffer on the heap with exactly its size: one element more is an AddressSanitizer report
    uint32_t* pool = new uint32_t[pool_v.size()];
    unsigned long long *off = new unsigned long long[n], *stats = new unsigned long long[4 * (size_t)n], *out_off = new unsigned long long[n];
    int *len = new int[n], *out_len = new int[n];
    std::copy(pool_v.begin(), pool_v.end(), pool); std::copy(off_v.begin(), off_v.end(), off); std::copy(len_v.begin(), len_v.end(), len);
    unsigned long long need[1] = {77};
    uint32_t probe = 5;
    int rc = 1;
    uint32_t* out = nullptr;
    do {
        std::fill(stats, stats + 4 * (size_t)n, 9ull);
        int st = call(pool, off, len, n, h, w, colour, conn, threshold, keep_largest, stats, &probe, 0, out_off, out_len, need);
        if (st != AMP_ERR_NOMEM || probe != 5 || stats[0] != 9) break;                  // refused, only the need written
        const size_t total = (size_t)need[0];
        size_t sum = 0;
        for (const auto& c : want) sum += c.size();
        if (total != sum) break;
        out = new uint32_t[total];
        if (call(pool, off, len, n, h, w, colour, conn, threshold, keep_largest, stats, out, total, out_off, out_len, need) != AMP_OK) break;
        bool ok = need[0] == total;
        size_t at = 0;
        for (int p = 0; p < n && ok; ++p) {
            ok &= out_off[p] == at && (size_t)out_len[p] == want[p].size();
            for (size_t j = 0; j < want[p].size() && ok; ++j) ok &= out[at + j] == want[p][j];
            for (int k = 0; k < 4; ++k) ok &= stats[4 * (size_t)p + k] == want_stats[4 * (size_t)p + k];
            at += want[p].size();
        }
        if (!ok) break;
        if (call(pool, off, len, n, h, w, colour, conn, threshold, keep_largest, stats, out, total - 1, out_off, out_len, need) != AMP_ERR_NOMEM) break;
        std::fill(stats, stats + 4 * (size_t)n, 9ull);
        if (call(pool, off, len, n, h, w, colour, conn, threshold, keep_largest, stats, nullptr, 0, nullptr, nullptr, nullptr) != AMP_OK) break;       // statistics only
        for (size_t k = 0; k < 4 * (size_t)n; ++k) ok &= stats[k] == want_stats[k];
        if (!ok) break;
        rc = 0;
    } while (0);
    delete[] pool; delete[] off; delete[] stats; delete[] out_off; delete[] len; delete[] out_len; delete[] out;
    if (rc) fprintf(stderr, "case %d x %d, %d masks, colour %d connectivity %d threshold %u keep_largest %d failed (%s)\n", h, w, n, colour, conn,
                    threshold, keep_largest, amp::g_err);
    return rc;
}

static int every_rule(const std::vector<std::vector<int>>& masks, int h, int w, bool loose = false) {
    const unsigned int thresholds[] = {0u, 1u, 2u, 5u, 9u, 10u, 17u, 0xffffffffu};
    for (int conn = 1; conn <= 2; ++conn)
        for (unsigned int t : thresholds) {
            CHECK(one_case(masks, h, w, 0, conn, t, 0, loose) == 0);
            CHECK(one_case(masks, h, w, 1, conn, t, 0, loose) == 0);
            CHECK(one_case(masks, h, w, 1, conn, t, 1, loose) == 0);
        }
    return 0;
}

static std::vector<int> shape(int h, int w, int pattern) {
    std::vector<int> m((size_t)h * w, 0);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            int v = 0;
            if (pattern == 1) v = 1;                                                                 // full
            if (pattern == 2) v = (r + c) % 2 == 0;                                                 // checkerboard
            if (pattern == 3) v = c % 2 == 0 || r == ((c / 2) % 2 ? 0 : h - 1);                     // serpentine
            if (pattern == 4) v = !(c % 2 == 0 || r == ((c / 2) % 2 ? 0 : h - 1));                  // its complement
            if (pattern == 5) v = r == 0 || c == 0 || r == h - 1 || c == w - 1 || (r == h / 2 && c > 1 && c < w - 2);     // on all four borders
            if (pattern == 6) {                                                                      // a ring in a ring with a speck, as far as it fits
                const int d = std::min(std::min(r, h - 1 - r), std::min(c, w - 1 - c));
                v = d == 1 || d == 3 || (r == h / 2 && c == w / 2 && d > 4);
            }
            if (pattern == 7) v = (r >= 1 && r < h - 1 && c >= 0 && c < w - 2) && !(r >= 2 && r < h - 2 && c < w - 3);    // a C closed by the border
            if (pattern == 8) v = (r >= 1 && r < 5 && c >= 1 && c < 5) && !((r == 2 && c == 2) || (r == 1 && c == 1));     // a hole meets the outside by a corner
            m[(size_t)r * w + c] = v;
        }
    return m;
}

static int shapes() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {8, 8}, {64, 3}, {63, 5}, {65, 5}, {15, 15}, {65, 33}, {130, 40}, {9, 12}};
    for (const auto& s : sizes) {
        const int h = s[0], w = s[1];
        std::vector<std::vector<int>> all;
        for (int pattern = 0; pattern < 9; ++pattern) {
            all.push_back(shape(h, w, pattern));
            if (h * w <= 225) CHECK(every_rule({all.back()}, h, w) == 0);
        }
        CHECK(every_rule(all, h, w) == 0);                           // the shapes of one size in one call
        CHECK(every_rule(all, h, w, true) == 0);                     // ... with zero-length runs in the input
    }
    return 0;
}

static int refusals() {
    uint32_t pool[4] = {2, 3, 1, 0};
    unsigned long long off[1] = {0}, stats[4] = {5, 5, 5, 5}, out_off[1] = {5}, need[1] = {5};
    int len[1] = {3}, out_len[1] = {5};
    uint32_t out[8];
#define REFUSED(POOL, LEN0, N, H, W, COLOUR, CONN, KEEP, STATS, OUT, OUTOFF, NEED)                                                         \
    do { len[0] = LEN0; CHECK(call(POOL, off, len, N, H, W, COLOUR, CONN, 0u, KEEP, STATS, OUT, 8, OUTOFF, out_len, NEED) == AMP_ERR_ARG); } while (0)
    REFUSED(pool, 3, -1, 2, 3, 1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 0, 3, 1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, -1, 1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 32769, 1, 1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 32768, 32768 + 1, 1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 2, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, -1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 1, 0, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 1, 3, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 1, 2, 2, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 0, 2, 1, stats, out, out_off, need);
    REFUSED(nullptr, 3, 1, 2, 3, 1, 2, 0, stats, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 1, 2, 0, nullptr, out, out_off, need);
    REFUSED(pool, 3, 1, 2, 3, 1, 2, 0, stats, out, nullptr, need);
    REFUSED(pool, 3, 1, 2, 3, 1, 2, 0, stats, out, out_off, nullptr);
    REFUSED(pool, 0, 1, 2, 3, 1, 2, 0, stats, out, out_off, need);           // an empty run list
    REFUSED(pool, 2, 1, 2, 3, 1, 2, 0, stats, out, out_off, need);           // 5 of 6 pixels
    REFUSED(pool, 3, 1, 1, 5, 1, 2, 0, stats, out, out_off, need);           // 6 pixels in an image of 5
    CHECK(stats[0] == 5 && out_off[0] == 5 && out_len[0] == 5 && need[0] == 5);
    len[0] = 3;
    CHECK(call(pool, off, len, 1, 2, 3, 1, 2, 0u, 0, stats, out, 8, out_off, out_len, need) == AMP_OK && need[0] == 3 && stats[0] == 1 && stats[1] == 3);
    CHECK(call(pool, off, len, 0, 2, 3, 1, 2, 0u, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == AMP_OK);      // no mask: nothing is read
    return 0;
}

int main() {
    CHECK(shapes() == 0);
    CHECK(refusals() == 0);
    for (int it = 0; it < 300; ++it) {
        const int h = 1 + rnd() % (it % 3 ? 40 : 130), w = 1 + rnd() % 40, n = 1 + rnd() % 12;
        const unsigned int density = it % 2 ? 30 + 20 * (rnd() % 3) : 85 + rnd() % 12;
        std::vector<std::vector<int>> masks((size_t)n, std::vector<int>((size_t)h * w));
        for (auto& m : masks)
            for (auto& v : m) v = rnd() % 100 < density;
        const unsigned int thresholds[] = {0u, 1u, 2u, 3u, 5u, 9u, 30u, 0xffffffffu};
        const int colour = it % 4 < 2;
        CHECK(one_case(masks, h, w, colour, 1 + (it / 4) % 2, thresholds[rnd() % 8], colour ? (int)(rnd() % 2) : 0, it % 5 == 0) == 0);
    }
    printf("MASK PARTS SANITIZE OK\n");
    return 0;
}
