// Host-only AddressSanitizer / UBSan run of what the four mask analyses share (ampis_amd/csrc/run_list.h): the painter against a per-pixel
// loop -- the sizes of tests/run_list_cases.py, every run [s, e) of a sample that covers all word and column borders, the tight box, the full
// image and random crops inside and around the image --, the walk over a run list (boxes and areas against the pixels, the refusals, and
// hostile lengths that must be refused before anything is read), and the hostile `off / len` that the four argument checks of
// ampis_amd/csrc/mask_analysis_host.hip must refuse without reading a run.  Built and run by tests/test_run_list_sanitize.py like the other
// five sanitizer programs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// pixels [s, e) into the plane (r0, c0, H, W), bit by bit; the plane has exactly W * pitch words: a word too far is a heap overflow
static std::vector<amp::u64> paint_by_pixel(unsigned int s, unsigned int e, int h, int r0, int c0, int H, int W) {
    const int pitch = (H + 63) >> 6;
    std::vector<amp::u64> plane((size_t)W * pitch, 0ull);
    for (unsigned int x = s; x < e; ++x) {
        const int r = (int)(x % (unsigned)h) - r0, c = (int)(x / (unsigned)h) - c0;
        if (r >= 0 && r < H && c >= 0 && c < W) plane[(size_t)c * pitch + (r >> 6)] |= 1ull << (r & 63);
    }
    return plane;
}

template <bool CLIP>
static bool painter_agrees(unsigned int s, unsigned int e, int h, int r0, int c0, int H, int W) {
    const int pitch = (H + 63) >> 6;
    std::vector<amp::u64> plane((size_t)W * pitch, 0ull);
    amp::paint_run<CLIP>(s, e, h, plane.data(), r0, c0, H, W, pitch, amp::OrPlain());
    return plane == paint_by_pixel(s, e, h, r0, c0, H, W);
}

static int painter(int h, int w) {
    const unsigned int area = (unsigned)h * (unsigned)w;
    std::vector<unsigned int> cuts = {0, 1, area - 1, area};                      // run ends worth trying: the image's, every column's, every word's
    for (int c = 0; c < w; ++c)
        for (int r : {0, 1, 62, 63, 64, 65, 127, 128, h - 1})
            if (r < h) cuts.push_back((unsigned)c * h + r);
    for (unsigned int s : cuts)
        for (unsigned int e : cuts) {
            if (s >= e || e > area) continue;
            CHECK(painter_agrees<false>(s, e, h, 0, 0, h, w));                    // the full image
            CHECK(painter_agrees<true>(s, e, h, 0, 0, h, w));
            const int cf = s / h, cl = (e - 1) / h;                               // the run's tight box
            const int r0 = cf == cl ? (int)(s % h) : 0, r1 = cf == cl ? (int)((e - 1) % h) + 1 : h;
            CHECK(painter_agrees<false>(s, e, h, r0, cf, r1 - r0, cl - cf + 1));
            for (int k = 0; k < 4; ++k) {                                         // crops that cut the run, or miss it
                const int a0 = rnd() % h, a1 = a0 + 1 + rnd() % (h - a0), b0 = rnd() % w, b1 = b0 + 1 + rnd() % (w - b0);
                CHECK(painter_agrees<true>(s, e, h, a0, b0, a1 - a0, b1 - b0));
            }
        }
    return 0;
}

// random run lists with zero-length runs: the plan against the pixels
static int walk(int h, int w) {
    const unsigned int area = (unsigned)h * (unsigned)w;
    for (int it = 0; it < 40; ++it) {
        std::vector<uint32_t> c;
        unsigned int pos = 0;
        while (pos < area) {
            unsigned int n = rnd() % 4 == 0 ? 0 : 1 + rnd() % (it % 2 ? 3 * h : 5);
            n = std::min(n, area - pos);
            c.push_back(n);
            pos += n;
        }
        if (it % 5 == 0) c.push_back(0);                                          // a closing empty run
        std::vector<uint8_t> bit(area, 0);
        pos = 0;
        for (size_t j = 0; j < c.size(); ++j) { if (j & 1) std::fill(bit.begin() + pos, bit.begin() + pos + c[j], 1); pos += c[j]; }
        int r0 = h, r1 = -1, c0 = w, c1 = -1;
        unsigned int ones = 0;
        for (unsigned int x = 0; x < area; ++x)
            if (bit[x]) { const int r = x % h, q = x / h; r0 = std::min(r0, r); r1 = std::max(r1, r); c0 = std::min(c0, q); c1 = std::max(c1, q); ++ones; }
        for (int prefix = 0; prefix < 2; ++prefix) {
            amp::RunPlan pl;
            pl.reset(2);
            amp::u64 covered = 0;
            const std::vector<uint32_t> exact(c);                                 // exactly len entries: one read too far is a heap overflow
            CHECK(amp::plan_add_mask(pl, 1, exact.data(), (int)exact.size(), h, w, prefix != 0, &covered) == amp::RUNS_OK && covered == area);
            const amp::RunMask& m = pl.m[1];
            CHECK(pl.m[0].n == -1 && m.n >= 0 && m.area == ones && pl.S.size() == (size_t)m.n + 1 && pl.E.size() == pl.S.size());
            CHECK(pl.P.size() == (prefix ? pl.S.size() : 0));
            CHECK(pl.S[m.n] == 0xffffffffu && pl.E[m.n] == 0xffffffffu);
            if (ones) CHECK(m.r0 == r0 && m.c0 == c0 && m.r1 == r1 + 1 && m.c1 == c1 + 1);
            else CHECK(m.n == 0 && m.r0 == 0 && m.c0 == 0 && m.r1 == 0 && m.c1 == 0);
            std::vector<uint8_t> back(area, 0);
            unsigned int before = 0;
            for (int k = 0; k < m.n; ++k) {
                CHECK(pl.S[k] < pl.E[k] && pl.E[k] <= area && (k == 0 || pl.E[k - 1] <= pl.S[k]));
                if (prefix) CHECK(pl.P[k] == before);
                before += pl.E[k] - pl.S[k];
                std::fill(back.begin() + pl.S[k], back.begin() + pl.E[k], 1);
            }
            CHECK(back == bit && (!prefix || pl.P[m.n] == ones));
        }
        // the refusals, each on a buffer of exactly the entries that may be read
        amp::RunPlan pl;
        pl.reset(1);
        amp::u64 covered = 77;
        CHECK(amp::plan_add_mask(pl, 0, nullptr, 0, h, w, false, &covered) == amp::RUNS_EMPTY);
        CHECK(amp::plan_add_mask(pl, 0, nullptr, -5, h, w, false, &covered) == amp::RUNS_EMPTY);
        std::vector<uint32_t> shorter(c);
        size_t last = shorter.size() - 1;
        while (shorter[last] == 0) --last;
        shorter[last] -= 1;                                                       // one pixel short
        CHECK(amp::plan_add_mask(pl, 0, shorter.data(), (int)shorter.size(), h, w, false, &covered) == amp::RUNS_SHORT && covered == area - 1);
        std::vector<uint32_t> over(c);
        over[rnd() % over.size()] += 1;                                           // one pixel over
        CHECK(amp::plan_add_mask(pl, 0, over.data(), (int)over.size(), h, w, false, &covered) == amp::RUNS_OVER);
        const std::vector<uint32_t> huge(1, 0xffffffffu);                         // one entry exists, a thousand are claimed: refused at the first
        CHECK(amp::plan_add_mask(pl, 0, huge.data(), 1000, h, w, true, &covered) == amp::RUNS_OVER);
        CHECK(pl.m[0].n == -1);                                                   // a refused mask is never planned
    }
    return 0;
}

// off / len that point nowhere: the four checks refuse an empty list before they read a run
static int hostile(int h, int w) {
    const unsigned long long far[2] = {1ull << 40, ~0ull >> 4};
    const int none[2] = {0, -3}, zero[2] = {0, 0}, first[2] = {0, 1}, one = 1;
    const uint32_t pool[1] = {0};
    const int box[4] = {0, h, 0, w};
    uint32_t out[8];
    unsigned long long off2[8], px[8], need = 0;
    long long bbox[4];
    std::vector<int> crop;
    amp::RunPlan a, b;
    CHECK(amp::edge_distance_check(pool, far, none, 1, pool, far, none, 1, zero, zero, box, 1, h, w, out, 8, off2, out, 8, off2, crop, a) == AMP_ERR_ARG);
    CHECK(amp::region_props_check(pool, far, none, 2, h, w, bbox, px, a) == AMP_ERR_ARG);
    CHECK(amp::overlap_groups_check(pool, far, none, pool, far, none, first, first, &h, &w, one, out, 8, px, px, a, b) == AMP_ERR_ARG);
    CHECK(amp::seg_class_map_check(pool, far, none, 1, pool, far, none, 1, zero, zero, 1, h, w, 0, out, 8, off2, px, a, b, &need) == AMP_ERR_ARG);
    return 0;
}

int main() {
    for (int h : {1, 63, 64, 65, 129})
        for (int w : {1, 2, 5}) {
            CHECK(painter(h, w) == 0);
            CHECK(walk(h, w) == 0);
            CHECK(hostile(h, w) == 0);
        }
    printf("RUN LIST SANITIZE OK\n");
    return 0;
}
