// Host-only AddressSanitizer / UBSan run of amp_rle_overlap_groups' argument checks, plan and host evaluation (ampis_amd/csrc/mask_analysis_host.hip:
// amp::overlap_groups_check / amp::overlap_groups_host, what the call runs with a NULL context): random groups of random masks, every count
// compared with a per-pixel evaluation, output buffers of exactly the needed size, and hostile input.  Built and run by
// tests/test_rle_overlap_sanitize.py like the region-property run beside it.  The device kernel indexes only what these checks let through.
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

static int add_mask(Pool& p, int h, int w) {
    std::vector<uint8_t> m((size_t)h * w, 0);
    const int kind = rnd() % 6, y0 = rnd() % h, x0 = rnd() % w, y1 = y0 + 1 + rnd() % h, x1 = x0 + 1 + rnd() % w;
    const unsigned int noise = rnd() % 10, holes = rnd() % 30;
    for (int x = 0; x < w; ++x)
        for (int y = 0; y < h; ++y) {
            const bool in = y >= y0 && y < y1 && x >= x0 && x < x1;
            m[(size_t)x * h + y] = kind == 0 ? 0 : kind == 1 ? 1 : (in && rnd() % 100 >= holes) || rnd() % 100 < noise;
        }
    std::vector<uint32_t> c((size_t)h * w + 2);
    int k = 0;
    if (amp_rle_encode(m.data(), h, w, c.data(), (int)c.size(), &k) != AMP_OK) return 1;
    p.off.push_back(p.pool.size()); p.len.push_back(k);
    p.pool.insert(p.pool.end(), c.begin(), c.begin() + k);
    p.bits.push_back(m);
    return 0;
}

int main() {
    for (int it = 0; it < 120; ++it) {
        const int ng = 1 + rnd() % 3;
        Pool A, B;
        std::vector<int> af(1, 0), bf(1, 0), gh, gw;
        std::vector<uint32_t> want;
        std::vector<unsigned long long> want_a, want_b;
        for (int g = 0; g < ng; ++g) {
            const int h = 1 + rnd() % (it % 3 ? 40 : 130), w = 1 + rnd() % 40, na = rnd() % 5, nb = it % 7 == 0 ? 60 + rnd() % 10 : rnd() % 5;
            gh.push_back(h); gw.push_back(w);
            for (int i = 0; i < na; ++i) CHECK(add_mask(A, h, w) == 0);
            for (int j = 0; j < nb; ++j) CHECK(add_mask(B, h, w) == 0);
            for (int i = af.back(); i < af.back() + na; ++i)
                for (int j = bf.back(); j < bf.back() + nb; ++j) {
                    uint32_t s = 0;
                    for (size_t q = 0; q < (size_t)h * w; ++q) s += A.bits[i][q] & B.bits[j][q];
                    want.push_back(s);
                }
            af.push_back(af.back() + na); bf.push_back(bf.back() + nb);
        }
        for (auto& m : A.bits) { unsigned long long s = 0; for (uint8_t v : m) s += v; want_a.push_back(s); }
        for (auto& m : B.bits) { unsigned long long s = 0; for (uint8_t v : m) s += v; want_b.push_back(s); }
        std::vector<uint32_t> inter(want.size(), 99u);                            // exactly the need
        std::vector<unsigned long long> area_a(want_a.size(), 99ull), area_b(want_b.size(), 99ull);
        // the public entry point is device code; the NULL-context path is these two calls
        {
            amp::RunPlan a, b;
            CHECK(amp::overlap_groups_check(A.pool.data(), A.off.data(), A.len.data(), B.pool.data(), B.off.data(), B.len.data(), af.data(), bf.data(),
                                            gh.data(), gw.data(), ng, inter.data(), inter.size(), area_a.data(), area_b.data(), a, b) == AMP_OK);
            CHECK(amp::overlap_groups_host(a, b, af.data(), bf.data(), ng, inter.data()) == AMP_OK);
            CHECK(inter == want);
            CHECK(a.m.size() == want_a.size() && b.m.size() == want_b.size());
            for (size_t p = 0; p < a.m.size(); ++p) CHECK(a.m[p].area == want_a[p]);
            for (size_t p = 0; p < b.m.size(); ++p) CHECK(b.m[p].area == want_b[p]);
        }
        // hostile input: every one refused by the check
        amp::RunPlan a, b;
#define REFUSED(AP, AL, AF, BF, GH, GW, NG, CAP)                                                                                                  \
        CHECK(amp::overlap_groups_check(AP, A.off.data(), AL, B.pool.data(), B.off.data(), B.len.data(), AF, BF, GH, GW, NG, inter.data(), CAP, \
                                        area_a.data(), area_b.data(), a, b) == AMP_ERR_ARG)
        if (!A.pool.empty()) {
            std::vector<uint32_t> bad = A.pool;
            bad[A.off.back()] += 1;                                               // runs that do not sum to h * w
            REFUSED(bad.data(), A.len.data(), af.data(), bf.data(), gh.data(), gw.data(), ng, inter.size());
            bad = A.pool;
            bad[A.off[0]] = 0xffffffffu;                                          // a run far beyond the image
            REFUSED(bad.data(), A.len.data(), af.data(), bf.data(), gh.data(), gw.data(), ng, inter.size());
            std::vector<int> len2 = A.len;
            len2[0] = 0;                                                          // an empty run list
            REFUSED(A.pool.data(), len2.data(), af.data(), bf.data(), gh.data(), gw.data(), ng, inter.size());
            REFUSED(nullptr, A.len.data(), af.data(), bf.data(), gh.data(), gw.data(), ng, inter.size());
        }
        std::vector<int> bad_h = gh, bad_w = gw, bad_f = bf;
        bad_h[ng - 1] = 32769; bad_w[0] = 0; bad_f[ng] = bad_f[ng - 1] - 1;
        REFUSED(A.pool.data(), A.len.data(), af.data(), bf.data(), bad_h.data(), gw.data(), ng, inter.size());
        REFUSED(A.pool.data(), A.len.data(), af.data(), bf.data(), gh.data(), bad_w.data(), ng, inter.size());
        REFUSED(A.pool.data(), A.len.data(), af.data(), bad_f.data(), gh.data(), gw.data(), ng, inter.size());
        REFUSED(A.pool.data(), A.len.data(), af.data(), bf.data(), gh.data(), gw.data(), -1, inter.size());
        REFUSED(A.pool.data(), A.len.data(), af.data(), bf.data(), gh.data(), nullptr, ng, inter.size());
        if (!want.empty()) REFUSED(A.pool.data(), A.len.data(), af.data(), bf.data(), gh.data(), gw.data(), ng, inter.size() - 1);
    }
    printf("RLE OVERLAP SANITIZE OK\n");
    return 0;
}
