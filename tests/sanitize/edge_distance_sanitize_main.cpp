// Host-only AddressSanitizer / UBSan run of mask_edge_distance's argument checks and host evaluation (ampis_amd/csrc/mask_analysis_host.hip:
// amp::edge_distance_check / amp::edge_distance_host, what amp_mask_edge_distance runs with a NULL context), on random masks with boxes from
// empty to beyond the image -- every value compared with an exhaustive search -- and on hostile input.  Built and run by
// tests/test_edge_distance_sanitize.py like the codec's own sanitizer run (rle_sanitize_main.cpp).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

struct Pools {
    std::vector<uint32_t> pool;
    std::vector<unsigned long long> off;
    std::vector<int> len;
};

static int add_mask(Pools& p, const std::vector<uint8_t>& colmajor, int h, int w) {
    std::vector<uint32_t> c((size_t)h * w + 2);
    int m = 0;
    if (amp_rle_encode(colmajor.data(), h, w, c.data(), (int)c.size(), &m) != AMP_OK) return 1;
    p.off.push_back(p.pool.size());
    p.len.push_back(m);
    p.pool.insert(p.pool.end(), c.begin(), c.begin() + m);
    return 0;
}

// squared distances of q & ~t to t inside [r1, r2) x [c1, c2) by exhaustive search, row-major
static void brute(const std::vector<uint8_t>& q, const std::vector<uint8_t>& t, int h, int r1, int r2, int c1, int c2, std::vector<uint32_t>& out) {
    for (int r = r1; r < r2; ++r)
        for (int c = c1; c < c2; ++c) {
            if (!q[(size_t)c * h + r] || t[(size_t)c * h + r]) continue;
            uint32_t best = 0xffffffffu;
            for (int rr = r1; rr < r2; ++rr)
                for (int cc = c1; cc < c2; ++cc)
                    if (t[(size_t)cc * h + rr]) best = std::min(best, (uint32_t)((rr - r) * (rr - r) + (cc - c) * (cc - c)));
            out.push_back(best);
        }
}

int main() {
    for (int it = 0; it < 120; ++it) {
        const int h = 1 + rnd() % 70, w = 1 + rnd() % 75, nm = 1 + rnd() % 4, n = rnd() % 7;
        std::vector<std::vector<uint8_t>> G, P;
        Pools gp, pp;
        for (int i = 0; i < nm; ++i) {
            std::vector<uint8_t> g((size_t)h * w, 0), p((size_t)h * w, 0);
            const int y0 = rnd() % h, x0 = rnd() % w, y1 = y0 + 1 + rnd() % h, x1 = x0 + 1 + rnd() % w, dy = (int)(rnd() % 5) - 2, dx = (int)(rnd() % 5) - 2;
            const unsigned int noise = rnd() % 12;
            for (int x = 0; x < w; ++x)
                for (int y = 0; y < h; ++y) {
                    g[(size_t)x * h + y] = (y >= y0 && y < y1 && x >= x0 && x < x1) || rnd() % 100 < noise;
                    p[(size_t)x * h + y] = (y >= y0 + dy && y < y1 + dy && x >= x0 + dx && x < x1 + dx) || rnd() % 100 < noise;
                }
            if (it % 9 == 0 && i == 0) std::fill(p.begin(), p.end(), 0);          // an empty prediction: the sentinel
            CHECK(add_mask(gp, g, h, w) == 0 && add_mask(pp, p, h, w) == 0);
            G.push_back(g); P.push_back(p);
        }
        std::vector<int> pg((size_t)n), pq((size_t)n), box((size_t)n * 4);
        std::vector<uint32_t> wfp, wfn;
        std::vector<unsigned long long> wfpo(1, 0), wfno(1, 0);
        for (int k = 0; k < n; ++k) {
            pg[k] = rnd() % nm; pq[k] = rnd() % nm;
            int* b = &box[4 * (size_t)k];
            b[0] = rnd() % (h + 3); b[1] = b[0] + rnd() % (h + 40); b[2] = rnd() % (w + 3); b[3] = b[2] + rnd() % (w + 40);
            const int r1 = std::min(b[0], h), r2 = std::min(b[1], h), c1 = std::min(b[2], w), c2 = std::min(b[3], w);
            brute(P[pq[k]], G[pg[k]], h, r1, r2, c1, c2, wfp);
            brute(G[pg[k]], P[pq[k]], h, r1, r2, c1, c2, wfn);
            wfpo.push_back(wfp.size()); wfno.push_back(wfn.size());
        }
        std::vector<uint32_t> fp(wfp.size()), fn(wfn.size());                    // exactly the need: one value more would be a heap overflow
        std::vector<unsigned long long> fpo((size_t)n + 1, 77), fno((size_t)n + 1, 77);
        std::vector<int> crop;
        amp::RunPlan runs;
        CHECK(amp::edge_distance_check(gp.pool.data(), gp.off.data(), gp.len.data(), nm, pp.pool.data(), pp.off.data(), pp.len.data(), nm, pg.data(), pq.data(),
                                       box.data(), n, h, w, fp.data(), fp.size(), fpo.data(), fn.data(), fn.size(), fno.data(), crop, runs) == AMP_OK);
        CHECK(amp::edge_distance_host(runs, nm, pg.data(), pq.data(), crop.data(),
                                      n, h, fp.data(), fp.size(), fpo.data(), fn.data(), fn.size(), fno.data()) == AMP_OK);
        CHECK(fp == wfp && fn == wfn && fpo == wfpo && fno == wfno);
        if (!wfp.empty()) {                                                      // one value short: refused, nothing written
            std::vector<uint32_t> small(wfp.size() - 1, 5u);
            std::vector<unsigned long long> o2((size_t)n + 1, 77);
            CHECK(amp::edge_distance_host(runs, nm, pg.data(), pq.data(),
                                          crop.data(), n, h, small.data(), small.size(), o2.data(), fn.data(), fn.size(), fno.data()) == AMP_ERR_NOMEM);
            CHECK(std::all_of(small.begin(), small.end(), [](uint32_t v) { return v == 5u; }) && std::all_of(o2.begin(), o2.end(), [](unsigned long long v) { return v == 77; }));
        }
        if (n > 0) {                                                             // hostile input: every one refused by the check, by name
            std::vector<int> crop2;
            amp::RunPlan runs2;
            auto check = [&](const Pools& g2, const std::vector<int>& pg2, const std::vector<int>& box2, int hh) {
                return amp::edge_distance_check(g2.pool.data(), g2.off.data(), g2.len.data(), nm, pp.pool.data(), pp.off.data(), pp.len.data(), nm, pg2.data(), pq.data(),
                                                box2.data(), n, hh, w, fp.data(), fp.size(), fpo.data(), fn.data(), fn.size(), fno.data(), crop2, runs2);
            };
            Pools bad = gp;
            bad.pool[bad.off[pg[0]]] += 1;                                       // runs that do not sum to h * w
            CHECK(check(bad, pg, box, h) == AMP_ERR_ARG);
            bad = gp;
            bad.len[pg[0]] = 0;                                                  // an empty run list
            CHECK(check(bad, pg, box, h) == AMP_ERR_ARG);
            std::vector<int> pg2 = pg;
            pg2[n - 1] = nm;                                                     // a pair index beyond the masks
            CHECK(check(gp, pg2, box, h) == AMP_ERR_ARG);
            pg2[n - 1] = -1;
            CHECK(check(gp, pg2, box, h) == AMP_ERR_ARG);
            std::vector<int> box2 = box;
            box2[0] = -1;                                                        // a negative index
            CHECK(check(gp, pg, box2, h) == AMP_ERR_ARG);
            box2 = box;
            box2[2] = box2[3] + 1;                                               // c1 > c2
            CHECK(check(gp, pg, box2, h) == AMP_ERR_ARG);
            CHECK(check(gp, pg, box, 32769) == AMP_ERR_ARG && check(gp, pg, box, 0) == AMP_ERR_ARG);
        }
    }
    printf("EDGE DISTANCE SANITIZE OK\n");
    return 0;
}
