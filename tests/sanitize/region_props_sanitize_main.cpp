// Host-only AddressSanitizer / UBSan run of the region-property argument checks and host evaluation (ampis_amd/csrc/mask_analysis_host.hip:
// amp::region_props_check / amp::region_props_host, what amp_mask_region_props runs with a NULL context, and through them the word arithmetic
// of region_props.h that the kernels share), on random masks up to three 64-row words tall -- every integer compared with a per-pixel
// evaluation -- and on hostile input.  Built and run by tests/test_region_props_sanitize.py like the edge-distance run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

typedef std::pair<long long, long long> Pt;
static long long cross(const Pt& o, const Pt& a, const Pt& b) { return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first); }

// the 13 integers and the box of a column-major byte mask, pixel by pixel
static void brute(const std::vector<uint8_t>& m, int h, int w, int* box, unsigned long long* v) {
    auto at = [&](int r, int c) { return r >= 0 && r < h && c >= 0 && c < w && m[(size_t)c * h + r]; };
    std::fill(v, v + 13, 0ull);
    int r0 = h, r1 = -1, c0 = w, c1 = -1;
    std::vector<uint8_t> border((size_t)h * w, 0);
    std::vector<Pt> pts;
    for (int c = 0; c < w; ++c)
        for (int r = 0; r < h; ++r) {
            if (!at(r, c)) continue;
            r0 = std::min(r0, r); r1 = std::max(r1, r); c0 = std::min(c0, c); c1 = std::max(c1, c);
            v[0] += 1; v[1] += r; v[2] += c; v[3] += (unsigned long long)r * r; v[4] += (unsigned long long)r * c; v[5] += (unsigned long long)c * c;
            border[(size_t)c * h + r] = !(at(r - 1, c) && at(r + 1, c) && at(r, c - 1) && at(r, c + 1));
            pts.push_back(Pt(2 * c, 2 * r - 1)); pts.push_back(Pt(2 * c, 2 * r + 1)); pts.push_back(Pt(2 * c - 1, 2 * r)); pts.push_back(Pt(2 * c + 1, 2 * r));
        }
    box[0] = box[1] = box[2] = box[3] = 0;
    if (r1 < 0) return;
    box[0] = r0; box[1] = c0; box[2] = r1 + 1; box[3] = c1 + 1;
    auto bd = [&](int r, int c) { return r >= 0 && r < h && c >= 0 && c < w && border[(size_t)c * h + r]; };
    for (int c = 0; c < w; ++c)
        for (int r = 0; r < h; ++r) {
            if (!bd(r, c)) continue;
            const int n4 = bd(r - 1, c) + bd(r + 1, c) + bd(r, c - 1) + bd(r, c + 1), nd = bd(r - 1, c - 1) + bd(r - 1, c + 1) + bd(r + 1, c - 1) + bd(r + 1, c + 1);
            const int code = 1 + 2 * n4 + 10 * nd;
            if (code == 5 || code == 7 || code == 15 || code == 17 || code == 25 || code == 27) v[6] += 1;
            if (code == 21 || code == 33) v[7] += 1;
            if (code == 13 || code == 23) v[8] += 1;
        }
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    std::vector<Pt> hull;
    for (int pass = 0; pass < 2; ++pass) {
        const size_t start = hull.size();
        for (size_t i = 0; i < pts.size(); ++i) {
            const Pt& p = pass ? pts[pts.size() - 1 - i] : pts[i];
            while (hull.size() >= start + 2 && cross(hull[hull.size() - 2], hull.back(), p) <= 0) hull.pop_back();
            hull.push_back(p);
        }
        hull.pop_back();
    }
    for (int c = c0; c <= c1; ++c)
        for (int r = r0; r <= r1; ++r) {
            bool in = true;
            for (size_t k = 0; k < hull.size() && in; ++k) in = cross(hull[k], hull[(k + 1) % hull.size()], Pt(2 * c, 2 * r)) >= 0;
            v[9] += in;
        }
}

int main() {
    for (int it = 0; it < 150; ++it) {
        const int h = 1 + rnd() % (it % 3 ? 70 : 200), w = 1 + rnd() % 60, n = 1 + rnd() % 4;
        std::vector<uint32_t> pool;
        std::vector<unsigned long long> off;
        std::vector<int> len, wbox((size_t)n * 4);
        std::vector<unsigned long long> want((size_t)n * 13);
        for (int i = 0; i < n; ++i) {
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
            CHECK(amp_rle_encode(m.data(), h, w, c.data(), (int)c.size(), &k) == AMP_OK);
            off.push_back(pool.size()); len.push_back(k);
            pool.insert(pool.end(), c.begin(), c.begin() + k);
            brute(m, h, w, &wbox[4 * (size_t)i], &want[13 * (size_t)i]);
        }
        std::vector<long long> bbox((size_t)n * 4);                               // exactly the need
        std::vector<unsigned long long> vals((size_t)n * 13, 99);
        amp::RunPlan plan;
        CHECK(amp::region_props_check(pool.data(), off.data(), len.data(), n, h, w, bbox.data(), vals.data(), plan) == AMP_OK);
        CHECK(amp::region_props_host(plan, h, vals.data()) == AMP_OK);
        std::vector<int> box;                                                     // the tight boxes are the plan's
        for (const amp::RunMask& mk : plan.m) box.insert(box.end(), {mk.r0, mk.c0, mk.r1, mk.c1});
        CHECK(box == wbox && vals == want);
        // hostile input: every one refused by the check
        std::vector<uint32_t> bad = pool;
        bad[off[n - 1]] += 1;                                                     // runs that do not sum to h * w
        CHECK(amp::region_props_check(bad.data(), off.data(), len.data(), n, h, w, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
        bad = pool;
        bad[off[0]] = 0xffffffffu;                                                // a run far beyond the image
        CHECK(amp::region_props_check(bad.data(), off.data(), len.data(), n, h, w, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
        std::vector<int> len2 = len;
        len2[0] = 0;                                                              // an empty run list
        CHECK(amp::region_props_check(pool.data(), off.data(), len2.data(), n, h, w, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
        CHECK(amp::region_props_check(pool.data(), off.data(), len.data(), n, 32769, w, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
        CHECK(amp::region_props_check(pool.data(), off.data(), len.data(), n, h, 0, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
        CHECK(amp::region_props_check(pool.data(), off.data(), len.data(), -1, h, w, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
        CHECK(amp::region_props_check(nullptr, off.data(), len.data(), n, h, w, bbox.data(), vals.data(), plan) == AMP_ERR_ARG);
    }
    printf("REGION PROPS SANITIZE OK\n");
    return 0;
}
