// Host-only AddressSanitizer / UBSan run of amp_mask_intensity's argument check and host evaluation (ampis_amd/csrc/mask_intensity.h,
// mask_intensity_host.hip: amp::mask_intensity_check / mask_intensity_capacity / mask_intensity_host / mask_intensity_write, what the call runs
// with a NULL context): hand shapes (empty, full, 1 x 1, 1 x 9, 9 x 1, a checkerboard, whole columns, a run across a column end) and random
// masks at four densities, tight and with zero-length runs, under random images of both depths and 1 .. 4 channels, without a histogram and
// at the smallest and the largest hist_shift of the depth.  Every value is checked with code written here -- a loop over all pixels of the
// dense mask --; every buffer has exactly the capacity asked for, one word less is refused with nothing written, and bad arguments are
// refused.  Built and run by tests/test_mask_intensity_sanitize.py like the distance run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/mask_intensity.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// what amp_mask_intensity does with a NULL context
static int call(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const void* image, int channels, int depth,
                int hist_shift, unsigned long long* vals, uint32_t* hist, unsigned long long hist_cap, unsigned long long* need) {
    amp::RunPlan plan;
    amp::u64 nbins = 0;
    int st = amp::mask_intensity_check(pool, off, len, n, h, w, image, channels, depth, hist_shift, vals, hist, need, plan, nbins);
    if (st != AMP_OK) return st;
    if (nbins && (st = amp::mask_intensity_capacity(n, channels, nbins, hist_cap, need)) != AMP_OK) return st;
    if (n == 0) return AMP_OK;
    std::vector<amp::u64> raw;
    amp::mask_intensity_host(plan, h, w, image, channels, depth, hist_shift, nbins, raw, hist);
    amp::mask_intensity_write(plan, channels, raw, vals);
    return AMP_OK;
}

typedef std::vector<std::vector<int>> Masks;

template <typename T>
static int one_case(const Masks& masks, int h, int w, int C, int hist_shift, bool loose) {
    const int n = (int)masks.size(), depth = 8 * (int)sizeof(T);
    const size_t nbins = hist_shift < 0 ? 0 : (size_t)1 << (depth - hist_shift);
    std::vector<uint32_t> pool_v;
    std::vector<unsigned long long> off_v;
    std::vector<int> len_v;
    for (int i = 0; i < n; ++i) {
        const std::vector<uint32_t> c = encode(masks[i], h, w, loose);
        off_v.push_back(pool_v.size()); len_v.push_back((int)c.size());
        pool_v.insert(pool_v.end(), c.begin(), c.end());
    }
    // every buffer on the heap with exactly its size: one element more is an AddressSanitizer report
    const size_t px = (size_t)h * w * C, nvals = (size_t)n * C * 8, N = (size_t)n * C * nbins;
    uint32_t* pool = new uint32_t[pool_v.size()];
    unsigned long long *off = new unsigned long long[n], *vals = new unsigned long long[nvals];
    int* len = new int[n];
    T* img = new T[px];
    uint32_t *hist = nullptr, *hist2 = nullptr;
    std::copy(pool_v.begin(), pool_v.end(), pool); std::copy(off_v.begin(), off_v.end(), off); std::copy(len_v.begin(), len_v.end(), len);
    for (size_t i = 0; i < px; ++i) img[i] = (T)(rnd() % 5 == 0 ? (rnd() & 1 ? 0u : ~0u) : rnd());      // the extremes are common
    auto reset = [&]() { for (size_t i = 0; i < nvals; ++i) vals[i] = 77; };
    auto clean = [&]() { bool ok = true; for (size_t i = 0; i < nvals; ++i) ok = ok && vals[i] == 77; return ok; };
    reset();
    unsigned long long need[1] = {77};
    int rc = 1;
    do {
        int st;
        if (nbins) {
            uint32_t none[1] = {77};
            st = call(pool, off, len, n, h, w, img, C, depth, hist_shift, vals, none, 0, need);                           // the need
            if ((N > 0 && st != AMP_ERR_NOMEM) || (N == 0 && st != AMP_OK) || need[0] != N || none[0] != 77) { fprintf(stderr, "need: status %d (%s)\n", st, amp::g_err); break; }
            if (N > 0 && !clean()) { fprintf(stderr, "a refused call wrote its outputs\n"); break; }
            hist = new uint32_t[N];
            if (N) {                                                 // one word short: refused, the need again, nothing written
                hist2 = new uint32_t[N - 1];
                need[0] = 77;
                st = call(pool, off, len, n, h, w, img, C, depth, hist_shift, vals, hist2, N - 1, need);
                if (st != AMP_ERR_NOMEM || need[0] != N || !clean()) { fprintf(stderr, "short capacity: status %d\n", st); break; }
            }
        }
        st = call(pool, off, len, n, h, w, img, C, depth, hist_shift, vals, hist, N, nbins ? need : nullptr);             // exactly the need
        if (st != AMP_OK || (nbins && need[0] != N)) { fprintf(stderr, "exact capacity: status %d (%s)\n", st, amp::g_err); break; }
        bool good = true;
        for (int i = 0; i < n && good; ++i)
            for (int ch = 0; ch < C && good; ++ch) {
                unsigned long long want[8] = {0, 0, 0, 0, 0, ~0ull, 0, 0};
                std::vector<uint32_t> bins(nbins, 0);
                for (int y = 0; y < h; ++y)                          // all pixels
                    for (int x = 0; x < w; ++x) {
                        if (!masks[i][(size_t)y * w + x]) continue;
                        const unsigned long long v = img[((size_t)y * w + x) * C + ch];
                        ++want[0]; want[1] += v; want[2] += v * v; want[3] += (unsigned long long)y * v; want[4] += (unsigned long long)x * v;
                        want[5] = std::min(want[5], v); want[6] = std::max(want[6], v);
                        if (nbins) ++bins[(size_t)(v >> hist_shift)];
                    }
                if (!want[0]) want[5] = 0;
                for (int k = 0; k < 8; ++k) good = good && vals[((size_t)i * C + ch) * 8 + k] == want[k];
                for (size_t b = 0; b < nbins; ++b) good = good && hist[((size_t)i * C + ch) * nbins + b] == bins[b];
                if (!good) fprintf(stderr, "mask %d of %d, channel %d of %d, %d x %d, depth %d, hist_shift %d: wrong result\n", i, n, ch, C, h, w, depth, hist_shift);
            }
        if (!good) break;
        rc = 0;
    } while (0);
    delete[] pool; delete[] off; delete[] len; delete[] vals; delete[] img; delete[] hist; delete[] hist2;
    return rc;
}

static std::vector<int> blank(int h, int w, int v = 0) { return std::vector<int>((size_t)h * w, v); }

static int every_setting(const Masks& m, int h, int w, bool loose, int* cases) {
    for (int C = 1; C <= 4; ++C) {
        const int s8[] = {-1, 0, 8}, s16[] = {-1, 4, 16};
        for (int k = 0; k < 3; ++k) {
            CHECK(one_case<uint8_t>(m, h, w, C, s8[k], loose) == 0);
            CHECK(one_case<uint16_t>(m, h, w, C, s16[k], loose) == 0);
            *cases += 2;
        }
    }
    return 0;
}

int main() {
    int cases = 0;
    for (int loose = 0; loose < 2; ++loose) {
        const int sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 7}, {5, 6}, {20, 3}, {3, 30}, {70, 4}};
        for (const auto& hw : sizes) {
            const int h = hw[0], w = hw[1];
            Masks m;
            m.push_back(blank(h, w)); m.push_back(blank(h, w, 1));
            std::vector<int> board = blank(h, w), columns = blank(h, w), across = blank(h, w);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    board[(size_t)y * w + x] = (x + y) % 2 == 0;
                    columns[(size_t)y * w + x] = x % 3 != 1;                               // whole columns: runs that end exactly at a column end
                    across[(size_t)y * w + x] = (x == w / 2 && y >= h / 2) || (x == w / 2 + 1 && y <= h / 2);      // one run across a column end
                }
            m.push_back(board); m.push_back(columns); m.push_back(across);
            if (every_setting(m, h, w, loose != 0, &cases)) return 1;
            CHECK(one_case<uint8_t>(Masks(), h, w, 2, 0, false) == 0);
            ++cases;
        }
        for (int t = 0; t < 16; ++t) {
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
    const uint8_t img[6] = {1, 2, 3, 4, 5, 6};                                           // 2 x 3: the mask is (0, 1), (1, 1), (0, 2)
    uint32_t hist[2];
    unsigned long long vals[8], need[1];
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, 7, vals, hist, 2, need) == AMP_OK && need[0] == 2 && vals[0] == 3 && vals[1] == 2 + 5 + 3 && hist[0] == 3);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, -1, vals, nullptr, 0, nullptr) == AMP_OK && vals[5] == 2 && vals[6] == 5 && vals[3] == 5 && vals[4] == 2 + 5 + 6);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, 7, vals, hist, 1, need) == AMP_ERR_NOMEM && need[0] == 2);
    CHECK(call(good, off0, len3, -1, 2, 3, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 0, 3, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 32769, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 0, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 5, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 12, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, -2, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, 9, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 16, 3, vals, hist, 2, need) == AMP_ERR_ARG);                           // 8192 bins
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, 7, vals, nullptr, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, 7, vals, hist, 2, nullptr) == AMP_ERR_ARG);
    CHECK(call(nullptr, off0, len3, 1, 2, 3, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, nullptr, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len3, 1, 2, 3, img, 1, 8, 7, nullptr, hist, 2, need) == AMP_ERR_ARG);
    CHECK(call(good, off0, len0, 1, 2, 3, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);                            // an empty run list
    CHECK(call(good, off0, len2, 1, 2, 3, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);                            // short: 5 of 6 pixels
    CHECK(call(good, off0, len3, 1, 2, 2, img, 1, 8, 7, vals, hist, 2, need) == AMP_ERR_ARG);                            // over: 6 of 4 pixels
    printf("MASK INTENSITY SANITIZE OK (%d cases)\n", cases);
    return 0;
}
