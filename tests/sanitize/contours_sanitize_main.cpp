// Host-only AddressSanitizer / UBSan run of amp_mask_contours' argument check and host evaluation (ampis_amd/csrc/contours.h, contours_host.hip:
// amp::contours_check / amp::mp_build_items / amp::contours_host, what the call runs with a NULL context): hand shapes (empty, full, 1 x 1,
// 1 x 9, 9 x 1, corner pixels, diagonal pixels, a checkerboard, a frame, a hole with an island) and random masks at four densities, tight and
// with zero-length runs, at both connectivities.  Every result is checked per pixel with code written here -- every ring is a closed
// rectilinear chain of corners that starts at its smallest corner, the rings of a mask ascend by that corner, the parity of all vertical
// segments left of a pixel is the pixel, the areas sum to twice the mask's and the lengths to its crack perimeter --, every buffer has exactly
// the capacity asked for, one element less is refused with nothing written, and bad arguments are refused.  Built and run by
// tests/test_mask_contours_sanitize.py like the flatten run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/contours.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// what amp_mask_contours does with a NULL context
static int call(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int connectivity,
                unsigned long long* ring_first, unsigned long long* ring_off, int* ring_len, long long* ring_area2, long long* ring_length,
                unsigned long long ring_cap, int* xy, unsigned long long xy_cap, unsigned long long* need) {
    amp::RunPlan plan;
    int st = amp::contours_check(pool, off, len, n, h, w, connectivity, ring_first, ring_off, ring_len, ring_area2, ring_length, xy, need, plan);
    if (st != AMP_OK) return st;
    if (n == 0) { need[0] = 0; need[1] = 0; ring_first[0] = 0; return AMP_OK; }
    amp::MpItems items;
    if (!amp::mp_build_items(plan, h, w, 1, items)) return AMP_ERR_ARG;
    return amp::contours_host(items, h, connectivity, ring_first, ring_off, ring_len, ring_area2, ring_length, ring_cap, xy, xy_cap, need);
}

typedef std::vector<std::vector<int>> Masks;

static int one_case(const Masks& masks, int h, int w, int connectivity, bool loose) {
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
    unsigned long long *off = new unsigned long long[n], *first = new unsigned long long[n + 1];
    int* len = new int[n];
    std::copy(pool_v.begin(), pool_v.end(), pool); std::copy(off_v.begin(), off_v.end(), off); std::copy(len_v.begin(), len_v.end(), len);
    unsigned long long need[2] = {77, 77};
    int rc = 1;
    unsigned long long *r_off = nullptr, *r_off2 = nullptr;
    int *r_len = nullptr, *xy = nullptr, *r_len2 = nullptr, *xy2 = nullptr;
    long long *r_a2 = nullptr, *r_lg = nullptr, *r_a22 = nullptr, *r_lg2 = nullptr;
    do {
        unsigned long long none_u[1];
        int none_i[1];
        long long none_l[1];
        int st = call(pool, off, len, n, h, w, connectivity, first, none_u, none_i, none_l, none_l, 0, none_i, 0, need);      // the need
        const unsigned long long V = need[0], R = need[1];
        if ((st != AMP_OK) != (V > 0) || (V > 0 && st != AMP_ERR_NOMEM) || (V == 0) != (R == 0)) { fprintf(stderr, "need: status %d, %llu, %llu (%s)\n", st, V, R, amp::g_err); break; }
        r_off = new unsigned long long[R]; r_len = new int[R]; r_a2 = new long long[R]; r_lg = new long long[R]; xy = new int[2 * V];
        st = call(pool, off, len, n, h, w, connectivity, first, r_off, r_len, r_a2, r_lg, R, xy, V, need);                      // exactly the need
        if (st != AMP_OK || need[0] != V || need[1] != R) { fprintf(stderr, "exact capacity: status %d (%s)\n", st, amp::g_err); break; }
        if (V) {                                                     // one vertex or one ring short: refused, the need again
            r_off2 = new unsigned long long[R]; r_len2 = new int[R]; r_a22 = new long long[R]; r_lg2 = new long long[R]; xy2 = new int[2 * V];
            need[0] = need[1] = 77;
            st = call(pool, off, len, n, h, w, connectivity, first, r_off2, r_len2, r_a22, r_lg2, R, xy2, V - 1, need);
            if (st != AMP_ERR_NOMEM || need[0] != V || need[1] != R) { fprintf(stderr, "short xy: status %d\n", st); break; }
            st = call(pool, off, len, n, h, w, connectivity, first, r_off2, r_len2, r_a22, r_lg2, R - 1, xy2, V, need);
            if (st != AMP_ERR_NOMEM || need[0] != V || need[1] != R) { fprintf(stderr, "short rings: status %d\n", st); break; }
        }
        bool good = first[0] == 0 && first[n] == R;
        unsigned long long at = 0;
        for (int i = 0; i < n && good; ++i) {
            good = first[i] <= first[i + 1];
            std::vector<int> parity((size_t)h * w, 0);
            long long area = 0, a2 = 0, lg = 0, crack = 0;
            unsigned int before = 0;
            for (unsigned long long r = first[i]; r < first[i + 1] && good; ++r) {
                const int k = r_len[r];
                good = r_off[r] == at && k >= 4 && k % 2 == 0 && at + (unsigned long long)k <= V;
                if (!good) break;
                const int* p = xy + 2 * at;
                long long s = 0, l = 0;
                for (int j = 0; j < k && good; ++j) {
                    const int x0 = p[2 * j], y0 = p[2 * j + 1], x1 = p[2 * ((j + 1) % k)], y1 = p[2 * ((j + 1) % k) + 1];
                    const int x2 = p[2 * ((j + 2) % k)], y2 = p[2 * ((j + 2) % k) + 1];
                    good = x0 >= 0 && x0 <= w && y0 >= 0 && y0 <= h && ((x0 == x1) != (y0 == y1)) && ((x0 == x1) != (x1 == x2)) && ((y0 == y1) != (y1 == y2));
                    good = good && (j == 0 || amp::ct_key(x0, y0) > amp::ct_key(p[0], p[1]) || (x0 == p[0] && y0 == p[1]));
                    s += (long long)x0 * y1 - (long long)x1 * y0;
                    l += abs(x1 - x0) + abs(y1 - y0);
                    if (x0 == x1)                                    // a vertical segment toggles everything to its right
                        for (int y = std::min(y0, y1); y < std::max(y0, y1); ++y)
                            for (int x = x0; x < w; ++x) parity[(size_t)y * w + x] ^= 1;
                }
                const unsigned int key = amp::ct_key(p[0], p[1]);
                good = good && s == r_a2[r] && l == r_lg[r] && s != 0 && (r == first[i] || key > before);
                before = key;
                a2 += s; lg += l;
                at += (unsigned long long)k;
            }
            for (int y = 0; y < h && good; ++y)
                for (int x = 0; x < w; ++x) {
                    const int v = masks[i][(size_t)y * w + x];
                    area += v;
                    crack += (v != (x ? masks[i][(size_t)y * w + x - 1] : 0)) + (v != (y ? masks[i][(size_t)(y - 1) * w + x] : 0));
                    if (x == w - 1) crack += v;
                    if (y == h - 1) crack += v;
                    if (parity[(size_t)y * w + x] != v) good = false;
                }
            good = good && a2 == 2 * area && lg == crack;
            if (!good) fprintf(stderr, "mask %d of %d, %d x %d, connectivity %d: wrong rings\n", i, n, h, w, connectivity);
        }
        if (!good || at != V) break;
        rc = 0;
    } while (0);
    delete[] pool; delete[] off; delete[] first; delete[] len;
    delete[] r_off; delete[] r_len; delete[] r_a2; delete[] r_lg; delete[] xy;
    delete[] r_off2; delete[] r_len2; delete[] r_a22; delete[] r_lg2; delete[] xy2;
    return rc;
}

static std::vector<int> blank(int h, int w, int v = 0) { return std::vector<int>((size_t)h * w, v); }

int main() {
    int cases = 0;
    for (int k = 1; k <= 2; ++k)
        for (int loose = 0; loose < 2; ++loose) {
            const int sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 7}, {5, 6}, {66, 3}, {12, 13}};
            for (const auto& hw : sizes) {
                const int h = hw[0], w = hw[1];
                Masks m;
                m.push_back(blank(h, w)); m.push_back(blank(h, w, 1));
                std::vector<int> board = blank(h, w), corners = blank(h, w), frame = blank(h, w, 1), diag = blank(h, w);
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        board[(size_t)y * w + x] = (x + y) % 2 == 0;
                        if ((y == 0 || y == h - 1) && (x == 0 || x == w - 1)) corners[(size_t)y * w + x] = 1;
                        if (y > 1 && y < h - 2 && x > 1 && x < w - 2) frame[(size_t)y * w + x] = (y == h / 2 && x == w / 2 && h > 6 && w > 6);
                        if (x == y || x + 1 == y + 3) diag[(size_t)y * w + x] = 1;
                    }
                m.push_back(board); m.push_back(corners); m.push_back(frame); m.push_back(diag);
                CHECK(one_case(m, h, w, k, loose != 0) == 0);
                CHECK(one_case(Masks(), h, w, k, false) == 0);
                cases += 2;
            }
            for (int t = 0; t < 60; ++t) {
                const int h = 1 + (int)(rnd() % 24), w = 1 + (int)(rnd() % 24), n = 1 + (int)(rnd() % 4);
                const unsigned int density = 3 + 2 * (t % 4);                           // 0.3, 0.5, 0.7, 0.9
                Masks m;
                for (int i = 0; i < n; ++i) {
                    std::vector<int> one = blank(h, w);
                    for (int& v : one) v = rnd() % 10 < density;
                    m.push_back(one);
                }
                CHECK(one_case(m, h, w, k, loose != 0) == 0);
                ++cases;
            }
        }

    // refusals: AMP_ERR_ARG, and nothing is read or written beyond the buffers
    const uint32_t good[3] = {2, 3, 1};
    const unsigned long long off0[1] = {0};
    const int len3[1] = {3}, len0[1] = {0}, len2[1] = {2};
    unsigned long long first[2], r_off[2], need[2];
    int r_len[2], xy[16];
    long long r_a2[2], r_lg[2];
    CHECK(call(good, off0, len3, 1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_OK && need[0] == 6 && need[1] == 1);     // an L of three pixels
    CHECK(call(good, off0, len3, -1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 0, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 32769, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 3, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(nullptr, off0, len3, 1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 2, nullptr, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, nullptr, 8, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, nullptr) == AMP_ERR_ARG);
    CHECK(call(good, off0, len0, 1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);      // an empty run list
    CHECK(call(good, off0, len2, 1, 2, 3, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);      // short: 5 of 6 pixels
    CHECK(call(good, off0, len3, 1, 2, 2, 2, first, r_off, r_len, r_a2, r_lg, 2, xy, 8, need) == AMP_ERR_ARG);      // over: 6 of 4 pixels
    printf("CONTOURS SANITIZE OK (%d cases)\n", cases);
    return 0;
}
