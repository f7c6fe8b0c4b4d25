// Host-only AddressSanitizer / UBSan run of amp_flatten_instances' argument check and host evaluation (ampis_amd/csrc/flatten.h,
// flatten_host.hip: amp::flatten_check / amp::flatten_host, what the call runs with a NULL context): the hand shapes of tests/flatten_cases.py
// restated (1 x 1, 1 x 70, 70 x 1, 64 x 64, 65 x 65, 130 x 40, 40 x 130; a full mask under and over the others, identical masks, rings, a mask
// cut at column ends, empty masks, no mask, equal / descending / extreme ranks, many masks on one block, single pixels, a checkerboard) and
// random masks, every result compared with a per-pixel evaluation written here, every buffer of exactly the capacity asked for, and the
// refusals.  Built and run by tests/test_flatten_sanitize.py like the mask-parts run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/flatten.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// what amp_flatten_instances does with a NULL context
static int call(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const uint32_t* rank, int* labels,
                uint32_t* counts, unsigned long long counts_cap, unsigned long long* counts_off, int* counts_len, unsigned long long* stats,
                int* boxes, unsigned long long* pixels, unsigned long long* need) {
    amp::RunPlan plan;
    std::vector<int> order;
    int st = amp::flatten_check(pool, off, len, n, h, w, rank, counts, counts_cap, counts_off, counts_len, stats, boxes, pixels, need, plan, order);
    if (st != AMP_OK) return st;
    return amp::flatten_host(plan, order, h, w, labels, counts, counts_cap, counts_off, counts_len, stats, boxes, pixels, need);
}

typedef std::vector<std::vector<int>> Masks;

static int one_case(const Masks& masks, int h, int w, const std::vector<uint32_t>* rank, bool loose) {
    const int n = (int)masks.size();
    const size_t image = (size_t)h * w;
    // by definition, per pixel: the covering instance of smallest (rank, index)
    std::vector<int> want_labels(image, 0);
    std::vector<unsigned long long> want_stats(2 * (size_t)n, 0ull), want_pixels(3, 0ull);
    std::vector<int> want_boxes(4 * (size_t)n, 0);
    for (size_t p = 0; p < image; ++p) {
        int best = -1, cover = 0;
        for (int i = 0; i < n; ++i) {
            if (!masks[i][p]) continue;
            ++cover; ++want_stats[2 * (size_t)i];
            if (best < 0 || (rank && (*rank)[i] < (*rank)[best])) best = i;
        }
        ++want_pixels[cover < 2 ? cover : 2];
        if (best < 0) continue;
        want_labels[p] = best + 1;
        const int r = (int)(p / w), c = (int)(p % w);
        int* b = &want_boxes[4 * (size_t)best];
        if (want_stats[2 * (size_t)best + 1]++ == 0) { b[0] = r; b[1] = c; b[2] = r + 1; b[3] = c + 1; }
        else { b[0] = std::min(b[0], r); b[1] = std::min(b[1], c); b[2] = std::max(b[2], r + 1); b[3] = std::max(b[3], c + 1); }
    }
    std::vector<std::vector<uint32_t>> want;
    std::vector<uint32_t> pool_v;
    std::vector<unsigned long long> off_v;
    std::vector<int> len_v;
    size_t sum = 0;
    for (int i = 0; i < n; ++i) {
        const std::vector<uint32_t> c = encode(masks[i], h, w, loose);
        off_v.push_back(pool_v.size()); len_v.push_back((int)c.size());
        pool_v.insert(pool_v.end(), c.begin(), c.end());
        std::vector<int> vis(image);
        for (size_t p = 0; p < image; ++p) vis[p] = want_labels[p] == i + 1;
        want.push_back(encode(vis, h, w, false));
        sum += want.back().size();
    }
    // every buffer on the heap with exactly its size: one element more is an AddressSanitizer report
    uint32_t* pool = new uint32_t[pool_v.size()];
    uint32_t* rk = rank ? new uint32_t[n] : nullptr;
    unsigned long long *off = new unsigned long long[n], *stats = new unsigned long long[2 * (size_t)n], *counts_off = new unsigned long long[n];
    int *len = new int[n], *counts_len = new int[n], *boxes = new int[4 * (size_t)n], *labels = new int[image];
    unsigned long long* pixels = new unsigned long long[3];
    std::copy(pool_v.begin(), pool_v.end(), pool); std::copy(off_v.begin(), off_v.end(), off); std::copy(len_v.begin(), len_v.end(), len);
    if (rank) std::copy(rank->begin(), rank->end(), rk);
    unsigned long long need[1] = {77};
    uint32_t probe = 5;
    int rc = 1;
    uint32_t* out = nullptr;
    do {
        std::fill(stats, stats + 2 * (size_t)n, 9ull);
        pixels[0] = 9;
        if (sum > 0) {
            int st = call(pool, off, len, n, h, w, rk, labels, &probe, 0, counts_off, counts_len, stats, boxes, pixels, need);
            if (st != AMP_ERR_NOMEM || probe != 5 || pixels[0] != 9 || (n && stats[0] != 9)) break;    // refused, only the need written
            if (need[0] != sum) break;
        }
        if (sum > 2 * pool_v.size()) break;                          // the capacity the header states
        out = new uint32_t[sum ? sum : 1];
        if (call(pool, off, len, n, h, w, rk, labels, out, sum, counts_off, counts_len, stats, boxes, pixels, need) != AMP_OK) break;
        bool ok = need[0] == sum;
        size_t at = 0;
        for (int i = 0; i < n && ok; ++i) {
            ok &= counts_off[i] == at && (size_t)counts_len[i] == want[i].size();
            for (size_t j = 0; j < want[i].size() && ok; ++j) ok &= out[at + j] == want[i][j];
            for (int k = 0; k < 2; ++k) ok &= stats[2 * (size_t)i + k] == want_stats[2 * (size_t)i + k];
            for (int k = 0; k < 4; ++k) ok &= boxes[4 * (size_t)i + k] == want_boxes[4 * (size_t)i + k];
            at += want[i].size();
        }
        for (size_t p = 0; p < image && ok; ++p) ok &= labels[p] == want_labels[p];
        for (int k = 0; k < 3; ++k) ok &= pixels[k] == want_pixels[k];
        if (!ok) break;
        if (sum > 0 && call(pool, off, len, n, h, w, rk, labels, out, sum - 1, counts_off, counts_len, stats, boxes, pixels, need) != AMP_ERR_NOMEM) break;
        std::fill(stats, stats + 2 * (size_t)n, 9ull);
        if (call(pool, off, len, n, h, w, rk, nullptr, nullptr, 0, nullptr, nullptr, stats, boxes, pixels, nullptr) != AMP_OK) break;       // statistics only
        for (size_t k = 0; k < 2 * (size_t)n; ++k) ok &= stats[k] == want_stats[k];
        if (!ok) break;
        rc = 0;
    } while (0);
    delete[] pool; delete[] rk; delete[] off; delete[] stats; delete[] counts_off; delete[] len; delete[] counts_len; delete[] boxes;
    delete[] labels; delete[] pixels; delete[] out;
    if (rc) fprintf(stderr, "case %d x %d, %d masks, ranks %d, loose %d failed (%s)\n", h, w, n, rank ? 1 : 0, (int)loose, amp::g_err);
    return rc;
}

// every rank pattern of the hand cases on one set of masks
static int every_order(const Masks& masks, int h, int w) {
    const int n = (int)masks.size();
    std::vector<uint32_t> equal((size_t)n, 7u), down((size_t)n), ends((size_t)n), some((size_t)n);
    for (int i = 0; i < n; ++i) { down[i] = (uint32_t)(n - i); ends[i] = i % 2 ? 0u : 0xffffffffu; some[i] = rnd() % 3; }
    CHECK(one_case(masks, h, w, nullptr, false) == 0);
    CHECK(one_case(masks, h, w, nullptr, true) == 0);
    CHECK(one_case(masks, h, w, &equal, false) == 0);
    CHECK(one_case(masks, h, w, &down, false) == 0);
    CHECK(one_case(masks, h, w, &ends, true) == 0);
    CHECK(one_case(masks, h, w, &some, false) == 0);
    return 0;
}

static std::vector<int> shape(int h, int w, int pattern) {
    std::vector<int> m((size_t)h * w, 0);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const int d = std::min(std::min(r, h - 1 - r), std::min(c, w - 1 - c));
            int v = 0;
            if (pattern == 1) v = 1;                                                                 // full
            if (pattern == 2) v = (r + c) % 2 == 0;                                                 // checkerboard
            if (pattern == 3) v = (r + c) % 2 != 0;                                                 // the other half of it
            if (pattern == 4) v = d >= 1 && d < 5;                                                  // a ring
            if (pattern == 5) v = d >= 3 && d < 7;                                                  // a ring in it that shares two rings
            if (pattern == 6) v = c == w / 2;                                                       // a whole column: cuts at column ends
            if (pattern == 7) v = r < 2 || r >= h - 2;                                              // runs across the column ends
            if (pattern == 8) v = c >= 60 && c < 69;                                                // across the tile edge
            if (pattern == 9) v = r >= 61 && r < 67;
            m[(size_t)r * w + c] = v;
        }
    return m;
}

static int shapes() {
    const int sizes[][2] = {{1, 1}, {1, 70}, {70, 1}, {64, 64}, {65, 65}, {130, 40}, {40, 130}, {5, 4}, {66, 3}, {9, 11}};
    for (const auto& s : sizes) {
        const int h = s[0], w = s[1];
        Masks all;
        for (int pattern = 0; pattern < 10; ++pattern) all.push_back(shape(h, w, pattern));            // pattern 0: an empty mask first
        all.push_back(shape(h, w, 4));                                                                 // two identical masks
        all.push_back(shape(h, w, 0));                                                                 // an empty mask last
        CHECK(every_order(all, h, w) == 0);
        CHECK(every_order({shape(h, w, 2), shape(h, w, 3)}, h, w) == 0);                               // the checkerboard split between two
        CHECK(every_order({shape(h, w, 7), shape(h, w, 6)}, h, w) == 0);
        CHECK(every_order({shape(h, w, 0), shape(h, w, 0)}, h, w) == 0);                               // nothing is owned
        CHECK(every_order({shape(h, w, 1)}, h, w) == 0);
    }
    CHECK(one_case(Masks(), 6, 7, nullptr, false) == 0);                                               // no mask
    Masks block(300, std::vector<int>(70 * 70, 0)), dots(71 * 71, std::vector<int>(71 * 71, 0));
    for (int i = 0; i < 300; ++i) {
        for (int r = 30; r < 38; ++r)
            for (int c = 30; c < 38; ++c) block[i][(size_t)r * 70 + c] = 1;
        block[i][(size_t)(10 + i / 60) * 70 + i % 60] = 1;
    }
    std::vector<uint32_t> rank(300);
    for (auto& v : rank) v = rnd() % 40;
    CHECK(one_case(block, 70, 70, &rank, false) == 0);
    for (int i = 0; i < 71 * 71; ++i) dots[i][(size_t)((i * 37) % (71 * 71))] = 1;                     // 37 and 5041 share no factor: a permutation
    CHECK(one_case(dots, 71, 71, nullptr, false) == 0);
    return 0;
}

static int refusals() {
    uint32_t pool[4] = {2, 3, 1, 0}, rank[1] = {3}, out[8];
    unsigned long long off[1] = {0}, stats[2] = {5, 5}, counts_off[1] = {5}, need[1] = {5}, pixels[3] = {5, 5, 5};
    int len[1] = {3}, counts_len[1] = {5}, boxes[4] = {5, 5, 5, 5}, labels[6] = {5, 5, 5, 5, 5, 5};
#define REFUSED(POOL, LEN0, N, H, W, OUT, CAP, OUTOFF, STATS, BOXES, PIXELS, NEED)                                                          \
    do { len[0] = LEN0; CHECK(call(POOL, off, len, N, H, W, rank, labels, OUT, CAP, OUTOFF, counts_len, STATS, BOXES, PIXELS, NEED) == AMP_ERR_ARG); } while (0)
    REFUSED(pool, 3, -1, 2, 3, out, 8, counts_off, stats, boxes, pixels, need);
    REFUSED(pool, 3, 1, 0, 3, out, 8, counts_off, stats, boxes, pixels, need);
    REFUSED(pool, 3, 1, 2, -1, out, 8, counts_off, stats, boxes, pixels, need);
    REFUSED(pool, 3, 1, 32769, 1, out, 8, counts_off, stats, boxes, pixels, need);
    REFUSED(pool, 3, 1, 32768, 32768 + 1, out, 8, counts_off, stats, boxes, pixels, need);
    REFUSED(nullptr, 3, 1, 2, 3, out, 8, counts_off, stats, boxes, pixels, need);
    REFUSED(pool, 3, 1, 2, 3, out, 8, nullptr, stats, boxes, pixels, need);
    REFUSED(pool, 3, 1, 2, 3, out, 8, counts_off, nullptr, boxes, pixels, need);
    REFUSED(pool, 3, 1, 2, 3, out, 8, counts_off, stats, nullptr, pixels, need);
    REFUSED(pool, 3, 1, 2, 3, out, 8, counts_off, stats, boxes, nullptr, need);
    REFUSED(pool, 3, 1, 2, 3, out, 8, counts_off, stats, boxes, pixels, nullptr);
    REFUSED(pool, 3, 1, 2, 3, nullptr, 8, counts_off, stats, boxes, pixels, need);     // a capacity without counts
    REFUSED(pool, 0, 1, 2, 3, out, 8, counts_off, stats, boxes, pixels, need);         // an empty run list
    REFUSED(pool, 2, 1, 2, 3, out, 8, counts_off, stats, boxes, pixels, need);         // 5 of 6 pixels
    REFUSED(pool, 3, 1, 1, 5, out, 8, counts_off, stats, boxes, pixels, need);         // 6 pixels in an image of 5
    CHECK(stats[0] == 5 && counts_off[0] == 5 && counts_len[0] == 5 && need[0] == 5 && pixels[0] == 5 && boxes[0] == 5 && labels[0] == 5);
    len[0] = 3;
    CHECK(call(pool, off, len, 1, 2, 3, rank, labels, out, 8, counts_off, counts_len, stats, boxes, pixels, need) == AMP_OK);
    CHECK(need[0] == 3 && stats[0] == 3 && stats[1] == 3 && pixels[0] == 3 && pixels[1] == 3 && pixels[2] == 0 && labels[2] == 1 && labels[0] == 0);
    CHECK(call(nullptr, nullptr, nullptr, 0, 2, 3, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, pixels, nullptr) == AMP_OK);      // no mask: nothing is read
    CHECK(pixels[0] == 6 && pixels[1] == 0);
    return 0;
}

int main() {
    CHECK(shapes() == 0);
    CHECK(refusals() == 0);
    for (int it = 0; it < 300; ++it) {
        const int h = 1 + rnd() % (it % 3 ? 40 : 140), w = 1 + rnd() % (it % 3 == 1 ? 140 : 40), n = 1 + rnd() % 12;
        const unsigned int density = it % 2 ? 5 + 25 * (rnd() % 3) : 85 + rnd() % 12;
        Masks masks((size_t)n, std::vector<int>((size_t)h * w));
        for (auto& m : masks)
            for (auto& v : m) v = rnd() % 100 < density;
        std::vector<uint32_t> rank((size_t)n);
        for (auto& v : rank) v = it % 7 == 0 ? rnd() : rnd() % 4;
        CHECK(one_case(masks, h, w, it % 4 ? &rank : nullptr, it % 5 == 0) == 0);
    }
    printf("FLATTEN SANITIZE OK\n");
    return 0;
}
