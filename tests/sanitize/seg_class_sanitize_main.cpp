// Host-only AddressSanitizer / UBSan run of amp_seg_class_map's argument checks, plan and host evaluation (ampis_amd/csrc/mask_analysis_host.hip:
// amp::seg_class_map_check / amp::seg_class_map_host, what the call runs with a NULL context): the shapes of tests/seg_class_cases.py restated
// (one row, one column, 63 / 64 / 65 / 129 rows, masks owning the first and the last pixel, full columns, no pair, repeated pairs, empty masks)
// and random groups of random masks, every class decoded and compared with a per-pixel evaluation, the counts buffer of exactly the capacity
// asked for, and hostile input.  Built and run by tests/test_seg_class_sanitize.py like the overlap run beside it.  The device kernels index only
// what these checks let through.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

struct Pool {
    std::vector<uint32_t> pool;
    std::vector<unsigned long long> off;
    std::vector<int> len;
    std::vector<std::vector<uint8_t>> bits;       // column-major bytes of every mask
};

// kind 0 empty, 1 full, 2 the first pixel and the last, 3 full columns, otherwise a noisy box
static int add_mask(Pool& p, int h, int w, int kind) {
    std::vector<uint8_t> m((size_t)h * w, 0);
    const int y0 = rnd() % h, x0 = rnd() % w, y1 = y0 + 1 + rnd() % h, x1 = x0 + 1 + rnd() % w;
    const unsigned int noise = rnd() % 10, holes = rnd() % 30;
    for (int x = 0; x < w; ++x)
        for (int y = 0; y < h; ++y) {
            const bool in = y >= y0 && y < y1 && x >= x0 && x < x1;
            m[(size_t)x * h + y] = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? ((x == 0 && y == 0) || (x == w - 1 && y == h - 1) || (y == h - 1) || (y == 0 && x > 0))
                                 : kind == 3 ? (x >= x0 && x < x1) : ((in && rnd() % 100 >= holes) || rnd() % 100 < noise);
        }
    std::vector<uint32_t> c((size_t)h * w + 2);
    int k = 0;
    if (amp_rle_encode(m.data(), h, w, c.data(), (int)c.size(), &k) != AMP_OK) return 1;
    p.off.push_back(p.pool.size()); p.len.push_back(k);
    p.pool.insert(p.pool.end(), c.begin(), c.begin() + k);
    p.bits.push_back(m);
    return 0;
}

static int one_case(int h, int w, int ng, int np, int n, int it) {
    Pool G, P;
    for (int i = 0; i < ng; ++i) CHECK(add_mask(G, h, w, (it + i) % 7) == 0);
    for (int i = 0; i < np; ++i) CHECK(add_mask(P, h, w, (it + 3 * i + 1) % 7) == 0);
    std::vector<int> pg, pq;
    for (int i = 0; i < n; ++i) { pg.push_back(rnd() % ng); pq.push_back(rnd() % np); }
    if (n > 2) { pg[n - 1] = pg[0]; pq[n - 1] = pq[0]; }                          // the same pair twice
    const size_t area = (size_t)h * w;
    std::vector<uint8_t> code(area, 0);
    for (int i = 0; i < n; ++i)
        for (size_t q = 0; q < area; ++q) {
            const int a = G.bits[pg[i]][q], b = P.bits[pq[i]][q];
            code[q] |= (uint8_t)((a & b) | ((a & !b) << 1) | ((!a & b) << 2));
        }
    for (int mode = 0; mode < 2; ++mode) {
        const int K = mode ? 7 : 4;
        amp::RunPlan g, p;
        unsigned long long need = 0, coff[8], px[8];
        uint32_t probe = 0;
        int st = amp::seg_class_map_check(G.pool.data(), G.off.data(), G.len.data(), ng, P.pool.data(), P.off.data(), P.len.data(), np, pg.data(),
                                          pq.data(), n, h, w, mode, &probe, 0, coff, px, g, p, &need);
        CHECK(st == AMP_ERR_NOMEM && need >= (unsigned long long)K);              // capacity 0: refused, the need reported
        std::vector<uint32_t> counts((size_t)need, 99u);                          // exactly the need
        g = amp::RunPlan(); p = amp::RunPlan();
        CHECK(amp::seg_class_map_check(G.pool.data(), G.off.data(), G.len.data(), ng, P.pool.data(), P.off.data(), P.len.data(), np, pg.data(),
                                       pq.data(), n, h, w, mode, counts.data(), need, coff, px, g, p, &need) == AMP_OK);
        CHECK(amp::seg_class_map_host(g, p, pg.data(), pq.data(), n, h, w, mode, counts.data(), coff, px) == AMP_OK);
        CHECK(coff[0] == 0 && coff[K] <= need);
        unsigned long long want_px[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t q = 0; q < area; ++q) ++want_px[code[q]];
        for (int c = 0; c < 8; ++c) CHECK(px[c] == want_px[c]);
        for (int k = 0; k < K; ++k) {
            CHECK(coff[k] < coff[k + 1]);
            size_t pos = 0;
            for (unsigned long long j = coff[k]; j < coff[k + 1]; ++j) {
                const int val = (int)((j - coff[k]) & 1);
                CHECK(j == coff[k] || counts[j] > 0);                             // only the first count may be 0
                for (uint32_t t = 0; t < counts[j]; ++t, ++pos) {
                    CHECK(pos < area);
                    const int c = code[pos];
                    const int in = mode ? c == k + 1 : k < 3 ? c == (1 << k) : (c == 3 || c >= 5);
                    CHECK(in == val);
                }
            }
            CHECK(pos == area);
        }
        // hostile input: every one refused by the check
#define REFUSED(GP, GL, PG, N, HH, WW, MODE, CAP)                                                                                             \
        CHECK(amp::seg_class_map_check(GP, G.off.data(), GL, ng, P.pool.data(), P.off.data(), P.len.data(), np, PG, pq.data(), N, HH, WW, MODE, \
                                       counts.data(), CAP, coff, px, g, p, &need) != AMP_OK)
        if (n > 0) {
            std::vector<uint32_t> bad = G.pool;
            bad[G.off[pg[0]]] += 1;                                               // runs that do not sum to h * w
            REFUSED(bad.data(), G.len.data(), pg.data(), n, h, w, mode, counts.size());
            bad = G.pool;
            bad[G.off[pg[0]]] = 0xffffffffu;                                      // a run far beyond the image
            REFUSED(bad.data(), G.len.data(), pg.data(), n, h, w, mode, counts.size());
            std::vector<int> len2 = G.len, far = pg;
            len2[pg[0]] = 0;                                                      // an empty run list
            REFUSED(G.pool.data(), len2.data(), pg.data(), n, h, w, mode, counts.size());
            far[n - 1] = ng;                                                      // a pair index out of range
            REFUSED(G.pool.data(), G.len.data(), far.data(), n, h, w, mode, counts.size());
            far[n - 1] = -1;
            REFUSED(G.pool.data(), G.len.data(), far.data(), n, h, w, mode, counts.size());
            REFUSED(nullptr, G.len.data(), pg.data(), n, h, w, mode, counts.size());
            REFUSED(G.pool.data(), G.len.data(), pg.data(), n, h + 1, w, mode, counts.size());
        }
        REFUSED(G.pool.data(), G.len.data(), pg.data(), n, 32769, w, mode, counts.size());
        REFUSED(G.pool.data(), G.len.data(), pg.data(), n, h, 0, mode, counts.size());
        REFUSED(G.pool.data(), G.len.data(), pg.data(), -1, h, w, mode, counts.size());
        REFUSED(G.pool.data(), G.len.data(), pg.data(), n, h, w, 2, counts.size());
        REFUSED(G.pool.data(), G.len.data(), pg.data(), n, h, w, mode, counts.size() - 1);
    }
    return 0;
}

int main() {
    const int shapes[][2] = {{8, 8}, {1, 41}, {37, 1}, {1, 1}, {63, 5}, {64, 5}, {65, 5}, {129, 3}, {20, 30}};
    int it = 0;
    for (const auto& s : shapes)
        for (int n : {0, 1, 3, 64}) CHECK(one_case(s[0], s[1], 3, 4, n, it++) == 0);
    for (; it < 200; ++it) {
        const int h = 1 + rnd() % (it % 3 ? 40 : 96), w = 1 + rnd() % 40;
        CHECK(one_case(h, w, 1 + rnd() % 6, 1 + rnd() % 6, rnd() % 12, it) == 0);
    }
    printf("SEG CLASS SANITIZE OK\n");
    return 0;
}
