// Host-only AddressSanitizer / UBSan run of amp_mask_distance's argument check and host evaluation (ampis_amd/csrc/mask_distance.h,
// mask_distance_host.hip: amp::mask_distance_check / mask_distance_capacity / mask_distance_host / mask_distance_write, what the call runs with
// a NULL context): hand shapes (empty, full, 1 x 1, 1 x 9, 9 x 1, corner pixels, a checkerboard, a frame, a cross that touches all four
// sides, a full image with one far pixel missing) and random masks at four densities, tight and with zero-length runs, at both border values
// and ncurve 0, 1, 5 and 1025, with and without the map.  Every squared distance is checked per pixel with code written here -- all pairs: the
// smallest squared distance to a pixel that is not in the mask, the ring outside the image included with border_value 0 --, together with
// the statistics, the box and the curve; every buffer has exactly the capacity asked for, one word less is refused with nothing written, and
// bad arguments are refused.  Built and run by tests/test_mask_distance_sanitize.py like the morphology run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/mask_distance.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// what amp_mask_distance does with a NULL context
static int call(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int border, unsigned long long* stats,
                long long* boxes, unsigned long long* curve, int ncurve, uint32_t* map, unsigned long long map_cap, unsigned long long* map_off,
                unsigned long long* need) {
    amp::RunPlan plan;
    amp::MpItems items;
    std::vector<amp::u64> offs;
    int st = amp::mask_distance_check(pool, off, len, n, h, w, border, stats, boxes, curve, ncurve, map, map_cap, map_off, need, plan, items, offs);
    if (st != AMP_OK) return st;
    if (map && (st = amp::mask_distance_capacity(offs, map_cap, need)) != AMP_OK) return st;
    if (n == 0) return AMP_OK;
    amp::MdTotals t;
    amp::mask_distance_host(items, h, w, border, ncurve, offs, map, t);
    amp::mask_distance_write(plan, t, ncurve, offs, map != nullptr, stats, boxes, curve, map_off);
    return AMP_OK;
}

typedef std::vector<std::vector<int>> Masks;

// all pairs; 0 outside the mask, AMP_DIST_NONE where there is no background
static std::vector<unsigned long long> dense_d2(const std::vector<int>& m, int h, int w, int border) {
    std::vector<unsigned long long> out((size_t)h * w, 0);
    const int lo = border ? 0 : -1, hy = border ? h : h + 1, hx = border ? w : w + 1;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            if (!m[(size_t)y * w + x]) continue;
            unsigned long long best = AMP_DIST_NONE;
            for (int yy = lo; yy < hy; ++yy)
                for (int xx = lo; xx < hx; ++xx) {
                    const bool inside = yy >= 0 && yy < h && xx >= 0 && xx < w;
                    if (inside && m[(size_t)yy * w + xx]) continue;
                    best = std::min(best, (unsigned long long)((yy - y) * (yy - y) + (xx - x) * (xx - x)));
                }
            out[(size_t)y * w + x] = best;
        }
    return out;
}

static int one_case(const Masks& masks, int h, int w, int border, int ncurve, bool with_map, bool loose) {
    const int n = (int)masks.size();
    std::vector<uint32_t> pool_v;
    std::vector<unsigned long long> off_v;
    std::vector<int> len_v;
    for (int i = 0; i < n; ++i) {
        const std::vector<uint32_t> c = encode(masks[i], h, w, loose);
        off_v.push_back(pool_v.size()); len_v.push_back((int)c.size());
        pool_v.insert(pool_v.end(), c.begin(), c.end());
    }
    // every buffer on the heap with exactly its size: one element more is an AddressSanitizer report
    uint32_t* pool = new uint32_t[pool_v.size()];
    unsigned long long *off = new unsigned long long[n], *stats = new unsigned long long[4 * (size_t)n], *map_off = new unsigned long long[n];
    unsigned long long* curve = new unsigned long long[(size_t)n * ncurve];
    int* len = new int[n];
    long long* boxes = new long long[4 * (size_t)n];
    std::copy(pool_v.begin(), pool_v.end(), pool); std::copy(off_v.begin(), off_v.end(), off); std::copy(len_v.begin(), len_v.end(), len);
    auto reset = [&]() {
        for (int i = 0; i < n; ++i) {
            map_off[i] = 77;
            for (int k = 0; k < 4; ++k) { stats[4 * i + k] = 77; boxes[4 * i + k] = 77; }
            for (int k = 0; k < ncurve; ++k) curve[(size_t)i * ncurve + k] = 77;
        }
    };
    auto clean = [&]() {
        bool ok = true;
        for (int i = 0; i < n; ++i) {
            ok = ok && map_off[i] == 77;
            for (int k = 0; k < 4; ++k) ok = ok && stats[4 * i + k] == 77 && boxes[4 * i + k] == 77;
            for (int k = 0; k < ncurve; ++k) ok = ok && curve[(size_t)i * ncurve + k] == 77;
        }
        return ok;
    };
    reset();
    unsigned long long need[1] = {77};
    int rc = 1;
    uint32_t *map = nullptr, *map2 = nullptr;
    do {
        unsigned long long N = 0;
        int st;
        if (with_map) {
            uint32_t none[1] = {77};
            st = call(pool, off, len, n, h, w, border, stats, boxes, ncurve ? curve : nullptr, ncurve, none, 0, map_off, need);     // the need
            N = need[0];
            if ((N > 0 && st != AMP_ERR_NOMEM) || (N == 0 && st != AMP_OK) || none[0] != 77) { fprintf(stderr, "need: status %d, %llu (%s)\n", st, N, amp::g_err); break; }
            if (N > 0 && !clean()) { fprintf(stderr, "a refused call wrote its outputs\n"); break; }
            map = new uint32_t[N];
            if (N) {                                                 // one word short: refused, the need again, nothing written
                map2 = new uint32_t[N - 1];
                need[0] = 77;
                reset();
                st = call(pool, off, len, n, h, w, border, stats, boxes, ncurve ? curve : nullptr, ncurve, map2, N - 1, map_off, need);
                if (st != AMP_ERR_NOMEM || need[0] != N || !clean()) { fprintf(stderr, "short capacity: status %d\n", st); break; }
            }
        }
        st = call(pool, off, len, n, h, w, border, stats, boxes, ncurve ? curve : nullptr, ncurve, map, N, with_map ? map_off : nullptr,
                  with_map ? need : nullptr);                        // exactly the need
        if (st != AMP_OK || (with_map && need[0] != N)) { fprintf(stderr, "exact capacity: status %d (%s)\n", st, amp::g_err); break; }
        bool good = true;
        unsigned long long at = 0;
        for (int i = 0; i < n && good; ++i) {
            const std::vector<unsigned long long> want = dense_d2(masks[i], h, w, border);
            int r0 = h, r1 = 0, c0 = w, c1 = 0;
            unsigned long long area = 0, sum = 0, top = 0, pos = 0;
            std::vector<unsigned long long> cv((size_t)ncurve, 0);
            for (int x = 0; x < w; ++x)                              // column-major: the first of equals stays
                for (int y = 0; y < h; ++y) {
                    if (!masks[i][(size_t)y * w + x]) continue;
                    const unsigned long long d = want[(size_t)y * w + x];
                    ++area; r0 = std::min(r0, y); r1 = std::max(r1, y + 1); c0 = std::min(c0, x); c1 = std::max(c1, x + 1);
                    if (d != AMP_DIST_NONE) sum += d;
                    if (d > top) { top = d; pos = (unsigned long long)x * h + y; }
                    for (int r = 0; r < ncurve && (unsigned long long)r * r < d; ++r) ++cv[(size_t)r];
                }
            if (!area) r0 = r1 = c0 = c1 = 0;
            good = stats[4 * i] == top && stats[4 * i + 1] == pos && stats[4 * i + 2] == sum && stats[4 * i + 3] == area && boxes[4 * i] == r0 &&
                   boxes[4 * i + 1] == c0 && boxes[4 * i + 2] == r1 && boxes[4 * i + 3] == c1;
            for (int r = 0; r < ncurve; ++r) good = good && curve[(size_t)i * ncurve + r] == cv[(size_t)r];
            if (with_map) {
                good = good && map_off[i] == at;
                for (int y = r0; y < r1 && good; ++y)
                    for (int x = c0; x < c1; ++x) good = good && map[at + (unsigned long long)(y - r0) * (c1 - c0) + (x - c0)] == want[(size_t)y * w + x];
                at += (unsigned long long)(r1 - r0) * (c1 - c0);
            }
            if (!good) fprintf(stderr, "mask %d of %d, %d x %d, border %d, ncurve %d: wrong result\n", i, n, h, w, border, ncurve);
        }
        if (!good || (with_map && at != N)) break;
        rc = 0;
    } while (0);
    delete[] pool; delete[] off; delete[] len; delete[] stats; delete[] map_off; delete[] curve; delete[] boxes; delete[] map; delete[] map2;
    return rc;
}

static std::vector<int> blank(int h, int w, int v = 0) { return std::vector<int>((size_t)h * w, v); }

static int every_setting(const Masks& m, int h, int w, bool loose, int* cases) {
    const int curves[] = {0, 1, 5, 1025};
    for (int border = 0; border < 2; ++border)
        for (int k = 0; k < 4; ++k)
            for (int with_map = 0; with_map < 2; ++with_map) {
                CHECK(one_case(m, h, w, border, curves[k], with_map != 0, loose) == 0);
                ++*cases;
            }
    return 0;
}

int main() {
    int cases = 0;
    for (int loose = 0; loose < 2; ++loose) {
        const int sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 7}, {5, 6}, {20, 3}, {12, 13}, {3, 30}, {70, 4}};
        for (const auto& hw : sizes) {
            const int h = hw[0], w = hw[1];
            Masks m;
            m.push_back(blank(h, w)); m.push_back(blank(h, w, 1));
            std::vector<int> board = blank(h, w), corners = blank(h, w), frame = blank(h, w, 1), cross = blank(h, w), slot = blank(h, w, 1);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    board[(size_t)y * w + x] = (x + y) % 2 == 0;
                    if ((y == 0 || y == h - 1) && (x == 0 || x == w - 1)) corners[(size_t)y * w + x] = 1;
                    if (y > 1 && y < h - 2 && x > 1 && x < w - 2) frame[(size_t)y * w + x] = 0;
                    if (y == h / 2 || x == w / 2) cross[(size_t)y * w + x] = 1;
                }
            slot[(size_t)(h / 2) * w + (w - 1)] = 0;                 // the only background of the image, in its last column
            m.push_back(board); m.push_back(corners); m.push_back(frame); m.push_back(cross); m.push_back(slot);
            if (every_setting(m, h, w, loose != 0, &cases)) return 1;
            CHECK(one_case(Masks(), h, w, 0, 3, true, false) == 0);
            ++cases;
        }
        for (int t = 0; t < 24; ++t) {
            const int h = 1 + (int)(rnd() % 20), w = 1 + (int)(rnd() % 20), n = 1 + (int)(rnd() % 3);
            const unsigned int density = 3 + 2 * (t % 4);                               // 0.3, 0.5, 0.7, 0.9
            Masks m;
            for (int i = 0; i < n; ++i) {
                std::vector<int> one = blank(h, w);
                for (int& v : one) v = rnd() % 10 < density;
                m.push_back(one);
            }
            if (every_setting(m, h, w, loose != 0, &cases)) return 1;
        }
    }

    // refusals: AMP_ERR_ARG, and nothing is read or written beyond the buffers
    const uint32_t good[3] = {2, 3, 1};
    const unsigned long long off0[1] = {0};
    const int len3[1] = {3}, len0[1] = {0}, len2[1] = {2};
    uint32_t map[8];
    unsigned long long stats[4], curve[2], map_off[1], need[1];
    long long boxes[4];
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_OK && need[0] == 4 && stats[3] == 3 && curve[0] == 3);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, nullptr, 0, nullptr, 0, nullptr, nullptr) == AMP_OK && stats[0] == 1);
    CHECK(call(good, off0, len3, -1, 2, 3, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 0, 3, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 32769, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 2, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, -1, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, curve, -1, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, curve, AMP_MORPH_MAX_RADIUS + 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, nullptr, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, curve, 2, nullptr, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, curve, 2, map, 8, nullptr, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, boxes, curve, 2, map, 8, map_off, nullptr) == AMP_ERR_ARG);
    CHECK(call(nullptr, off0, len3, 1, 2, 3, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, nullptr, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, stats, nullptr, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len0, 1, 2, 3, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);              // an empty run list
    CHECK(call(good, off0, len2, 1, 2, 3, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);              // short: 5 of 6 pixels
    CHECK(call(good, off0, len3, 1, 2, 2, 0, stats, boxes, curve, 2, map, 8, map_off, need) == AMP_ERR_ARG);              // over: 6 of 4 pixels
    printf("MASK DISTANCE SANITIZE OK (%d cases)\n", cases);
    return 0;
}
