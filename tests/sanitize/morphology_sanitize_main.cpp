// Host-only AddressSanitizer / UBSan run of amp_mask_morphology's argument check and host evaluation (ampis_amd/csrc/morphology.h,
// morphology_host.hip: amp::morphology_check / amp::morphology_host, what the call runs with a NULL context): hand shapes (empty, full, 1 x 1,
// 1 x 9, 9 x 1, corner pixels, a checkerboard, a frame, a cross that touches all four borders) and random masks at four densities, tight and
// with zero-length runs, at every op, shape and border value and radii 0 .. 3, 7 and one beyond both sides.  Every result is checked per
// pixel with code written here -- the definition by offsets: a pixel is in the dilation when some offset of the element leads to the mask, in
// the erosion when every offset does, the outside counting as border_value --, together with box and area; every buffer has exactly the
// capacity asked for, one word less is refused with nothing written, and bad arguments are refused.  Built and run by
// tests/test_morphology_sanitize.py like the contours run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/morphology.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// what amp_mask_morphology does with a NULL context
static int call(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int op, int shape, int radius, int border,
                uint32_t* out_pool, unsigned long long out_cap, unsigned long long* out_off, int* out_len, long long* boxes,
                unsigned long long* areas, unsigned long long* need) {
    amp::MoRuns runs;
    int st = amp::morphology_check(pool, off, len, n, h, w, op, shape, radius, border, out_pool, out_off, out_len, boxes, areas, need, runs);
    if (st != AMP_OK) return st;
    if (n == 0) return amp::morphology_capacity(0, out_cap, need);
    return amp::morphology_host(runs, n, h, w, op, shape, radius, border, out_pool, out_cap, out_off, out_len, boxes, areas, need);
}

typedef std::vector<std::vector<int>> Masks;

static bool in_element(int shape, int r, int dx, int dy) {
    const int ax = abs(dx), ay = abs(dy);
    if (ax > r || ay > r) return false;
    if (shape == AMP_MORPH_SQUARE) return true;
    if (shape == AMP_MORPH_DIAMOND) return ax + ay <= r;
    return dx * dx + dy * dy <= r * r;
}

// the definition by offsets; outside: what a pixel beyond the image counts as
static std::vector<int> dense_pass(const std::vector<int>& m, int h, int w, bool grow, int shape, int r, int outside) {
    std::vector<int> out((size_t)h * w, 0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            bool any = false, all = true;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    if (!in_element(shape, r, dx, dy)) continue;
                    const int yy = y + dy, xx = x + dx;
                    const int v = yy < 0 || yy >= h || xx < 0 || xx >= w ? outside : m[(size_t)yy * w + xx];
                    any = any || v; all = all && v;
                }
            out[(size_t)y * w + x] = grow ? any : all;
        }
    return out;
}

static std::vector<int> dense_op(const std::vector<int>& m, int h, int w, int op, int shape, int r, int border) {
    std::vector<int> d = dense_pass(m, h, w, true, shape, r, 0), e = dense_pass(m, h, w, false, shape, r, border), out = m;
    if (op == AMP_MORPH_DILATE) return d;
    if (op == AMP_MORPH_ERODE) return e;
    if (op == AMP_MORPH_OPEN) return dense_pass(e, h, w, true, shape, r, 0);
    if (op == AMP_MORPH_CLOSE) return dense_pass(d, h, w, false, shape, r, border);
    for (size_t i = 0; i < out.size(); ++i) out[i] = op == AMP_MORPH_BAND_IN ? (m[i] && !e[i]) : (d[i] && !m[i]);
    return out;
}

static int one_case(const Masks& masks, int h, int w, int op, int shape, int r, int border, bool loose) {
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
    unsigned long long *off = new unsigned long long[n], *out_off = new unsigned long long[n], *areas = new unsigned long long[n];
    int *len = new int[n], *out_len = new int[n];
    long long* boxes = new long long[4 * (size_t)n];
    std::copy(pool_v.begin(), pool_v.end(), pool); std::copy(off_v.begin(), off_v.end(), off); std::copy(len_v.begin(), len_v.end(), len);
    for (int i = 0; i < n; ++i) { out_off[i] = 77; out_len[i] = 77; areas[i] = 77; boxes[4 * i] = boxes[4 * i + 1] = boxes[4 * i + 2] = boxes[4 * i + 3] = 77; }
    unsigned long long need[1] = {77};
    int rc = 1;
    uint32_t *out = nullptr, *out2 = nullptr;
    do {
        uint32_t none[1] = {77};
        int st = call(pool, off, len, n, h, w, op, shape, r, border, none, 0, out_off, out_len, boxes, areas, need);          // the need
        const unsigned long long N = need[0];
        if ((n > 0 && st != AMP_ERR_NOMEM) || (n == 0 && st != AMP_OK) || N < (unsigned long long)n || none[0] != 77) { fprintf(stderr, "need: status %d, %llu (%s)\n", st, N, amp::g_err); break; }
        bool clean = true;
        for (int i = 0; i < n; ++i) clean = clean && out_off[i] == 77 && out_len[i] == 77 && areas[i] == 77 && boxes[4 * i] == 77;
        if (!clean) { fprintf(stderr, "a refused call wrote its outputs\n"); break; }
        out = new uint32_t[N];
        st = call(pool, off, len, n, h, w, op, shape, r, border, out, N, out_off, out_len, boxes, areas, need);               // exactly the need
        if (st != AMP_OK || need[0] != N) { fprintf(stderr, "exact capacity: status %d (%s)\n", st, amp::g_err); break; }
        if (N) {                                                     // one word short: refused, the need again
            out2 = new uint32_t[N - 1];
            need[0] = 77;
            unsigned long long o2[1] = {77};
            st = call(pool, off, len, n, h, w, op, shape, r, border, out2, N - 1, n ? out_off : o2, out_len, boxes, areas, need);
            if (st != AMP_ERR_NOMEM || need[0] != N) { fprintf(stderr, "short capacity: status %d\n", st); break; }
        }
        bool good = true;
        unsigned long long at = 0;
        for (int i = 0; i < n && good; ++i) {
            const std::vector<int> want = dense_op(masks[i], h, w, op, shape, r, border);
            good = out_off[i] == at && out_len[i] >= 1 && at + (unsigned long long)out_len[i] <= N;
            if (!good) break;
            std::vector<int> got((size_t)h * w, 0);                  // decoded column-major into the row-major array
            unsigned long long pos = 0, area = 0;
            for (int j = 0; j < out_len[i] && good; ++j) {
                const uint32_t c = out[at + j];
                good = pos + c <= (unsigned long long)h * w && (c > 0 || j == 0);        // canonical: only the first count may be 0
                for (unsigned long long p = pos; good && p < pos + c && (j & 1); ++p) got[(size_t)(p % h) * w + (size_t)(p / h)] = 1;
                pos += c;
            }
            good = good && pos == (unsigned long long)h * w;
            int r0 = h, r1 = 0, c0 = w, c1 = 0;
            for (int y = 0; y < h && good; ++y)
                for (int x = 0; x < w; ++x) {
                    if (got[(size_t)y * w + x] != want[(size_t)y * w + x]) good = false;
                    if (!want[(size_t)y * w + x]) continue;
                    ++area; r0 = std::min(r0, y); r1 = std::max(r1, y + 1); c0 = std::min(c0, x); c1 = std::max(c1, x + 1);
                }
            if (!area) r0 = r1 = c0 = c1 = 0;
            good = good && areas[i] == area && boxes[4 * i] == r0 && boxes[4 * i + 1] == c0 && boxes[4 * i + 2] == r1 && boxes[4 * i + 3] == c1;
            if (!good) fprintf(stderr, "mask %d of %d, %d x %d, op %d, shape %d, radius %d, border %d: wrong result\n", i, n, h, w, op, shape, r, border);
            at += (unsigned long long)out_len[i];
        }
        if (!good || at != N) break;
        rc = 0;
    } while (0);
    delete[] pool; delete[] off; delete[] len; delete[] out_off; delete[] out_len; delete[] areas; delete[] boxes; delete[] out; delete[] out2;
    return rc;
}

static std::vector<int> blank(int h, int w, int v = 0) { return std::vector<int>((size_t)h * w, v); }

static int every_setting(const Masks& m, int h, int w, bool loose, const int* radii, int n_radii, int* cases) {
    for (int op = AMP_MORPH_DILATE; op <= AMP_MORPH_BAND_OUT; ++op)
        for (int shape = AMP_MORPH_SQUARE; shape <= AMP_MORPH_DISK; ++shape)
            for (int border = 0; border < 2; ++border)
                for (int k = 0; k < n_radii; ++k) {
                    CHECK(one_case(m, h, w, op, shape, radii[k], border, loose) == 0);
                    ++*cases;
                }
    return 0;
}

int main() {
    int cases = 0;
    const int radii[] = {0, 1, 2, 3, 7, 21}, few[] = {1, 3};
    for (int loose = 0; loose < 2; ++loose) {
        const int sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 7}, {5, 6}, {20, 3}, {12, 13}};
        for (const auto& hw : sizes) {
            const int h = hw[0], w = hw[1];
            Masks m;
            m.push_back(blank(h, w)); m.push_back(blank(h, w, 1));
            std::vector<int> board = blank(h, w), corners = blank(h, w), frame = blank(h, w, 1), cross = blank(h, w);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    board[(size_t)y * w + x] = (x + y) % 2 == 0;
                    if ((y == 0 || y == h - 1) && (x == 0 || x == w - 1)) corners[(size_t)y * w + x] = 1;
                    if (y > 1 && y < h - 2 && x > 1 && x < w - 2) frame[(size_t)y * w + x] = 0;
                    if (y == h / 2 || x == w / 2) cross[(size_t)y * w + x] = 1;
                }
            m.push_back(board); m.push_back(corners); m.push_back(frame); m.push_back(cross);
            if (every_setting(m, h, w, loose != 0, radii, 6, &cases)) return 1;
            CHECK(one_case(Masks(), h, w, AMP_MORPH_OPEN, AMP_MORPH_DISK, 2, 0, false) == 0);
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
            if (every_setting(m, h, w, loose != 0, few, 2, &cases)) return 1;
        }
    }

    // refusals: AMP_ERR_ARG, and nothing is read or written beyond the buffers
    const uint32_t good[3] = {2, 3, 1};
    const unsigned long long off0[1] = {0};
    const int len3[1] = {3}, len0[1] = {0}, len2[1] = {2};
    uint32_t out[8];
    unsigned long long out_off[1], areas[1], need[1];
    int out_len[1];
    long long boxes[4];
    CHECK(call(good, off0, len3, 1, 2, 3, AMP_MORPH_DILATE, AMP_MORPH_SQUARE, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_OK && need[0] == 2 && areas[0] == 6);
    CHECK(call(good, off0, len3, -1, 2, 3, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 0, 3, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 32769, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, -1, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 6, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 3, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 0, -1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 0, AMP_MORPH_MAX_RADIUS + 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 0, 1, 2, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(nullptr, off0, len3, 1, 2, 3, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 0, 1, 0, nullptr, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 0, 1, 0, out, 8, out_off, out_len, nullptr, areas, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, nullptr) == AMP_ERR_ARG);
    CHECK(call(good, off0, len0, 1, 2, 3, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);         // an empty run list
    CHECK(call(good, off0, len2, 1, 2, 3, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);         // short: 5 of 6 pixels
    CHECK(call(good, off0, len3, 1, 2, 2, 0, 0, 1, 0, out, 8, out_off, out_len, boxes, areas, need) == AMP_ERR_ARG);         // over: 6 of 4 pixels
    printf("MORPHOLOGY SANITIZE OK (%d cases)\n", cases);
    return 0;
}
