// Host-only AddressSanitizer / UBSan run of amp_polygons_to_rle's argument check and host evaluation (ampis_amd/csrc/polygon_runs_host.hip:
// amp::polygons_check / amp::polygons_host, what the call runs with a NULL context, on the routines of ampis_amd/csrc/rle_host.hip): random
// star polygons in and around images of many sizes, one to five polygons an instance, against the composition of the two public entry points
// amp_rle_from_polygon and amp_rle_merge2 written here, every output buffer of exactly the capacity asked for, the closed-form edge walk of
// mask_analysis.h against the crossings the routine collects, and the refusals.  Built and run by tests/test_polygons_sanitize.py.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() % 1000003u) / 1000003.0; }

// the run list of one instance from the public entry points
static int composed(const std::vector<std::vector<double>>& polys, int h, int w, std::vector<uint32_t>* out) {
    std::vector<uint32_t> cur, one((size_t)h * w + 2), tmp;
    for (size_t p = 0; p < polys.size(); ++p) {
        int m = 0;
        CHECK(amp_rle_from_polygon(polys[p].data(), (int)(polys[p].size() / 2), h, w, one.data(), (int)one.size(), &m) == AMP_OK);
        if (p == 0) { cur.assign(one.begin(), one.begin() + m); continue; }
        tmp.resize(cur.size() + (size_t)m);
        int k = 0;
        CHECK(amp_rle_merge2(cur.data(), (int)cur.size(), one.data(), m, 0, tmp.data(), (int)tmp.size(), &k) == AMP_OK);
        cur.assign(tmp.begin(), tmp.begin() + k);
    }
    *out = cur;
    return 0;
}

// the closed-form walk of mask_analysis.h gives the crossings of the routine: same multiset of positions
static int walk_matches(const std::vector<double>& xy, int h, int w) {
    const int k = (int)(xy.size() / 2);
    std::vector<unsigned long long> mine;
    for (int j = 0; j < k; ++j) {
        const int jn = j + 1 == k ? 0 : j + 1;
        const amp::PolygonEdge e = amp::polygon_edge(amp::polygon_grid(xy[2 * j]), amp::polygon_grid(xy[2 * j + 1]), amp::polygon_grid(xy[2 * jn]),
                                                     amp::polygon_grid(xy[2 * jn + 1]));
        for (int d = 1; d <= e.len; ++d) {
            unsigned int pos;
            if (amp::polygon_crossing(e, d, h, w, &pos)) mine.push_back(pos);
        }
    }
    mine.push_back((unsigned long long)h * w);
    std::sort(mine.begin(), mine.end());
    amp::PolygonScratch sc;
    amp::rle_from_polygon_runs(xy.data(), k, h, w, sc);
    // sc.a holds the differences of the sorted crossings
    CHECK(sc.a.size() == mine.size());
    unsigned long long at = 0;
    for (size_t i = 0; i < mine.size(); ++i) { at += sc.a[i]; CHECK(at == mine[i]); }
    return 0;
}

static int one_case(const std::vector<std::vector<std::vector<double>>>& insts, int h, int w) {
    const int n = (int)insts.size();
    std::vector<double> xy;
    std::vector<unsigned long long> poff(1, 0);
    std::vector<int> first(1, 0);
    std::vector<uint32_t> want;
    std::vector<size_t> want_off;
    for (const auto& inst : insts) {
        for (const auto& p : inst) { xy.insert(xy.end(), p.begin(), p.end()); poff.push_back(xy.size()); CHECK(walk_matches(p, h, w) == 0); }
        first.push_back((int)poff.size() - 1);
        std::vector<uint32_t> c;
        CHECK(composed(inst, h, w, &c) == 0);
        want_off.push_back(want.size());
        want.insert(want.end(), c.begin(), c.end());
    }
    want_off.push_back(want.size());
    unsigned long long need = 77, probe_l = 5;
    uint32_t probe_c = 5;
    unsigned int probe_u = 5;
    int probe_i[4] = {5, 5, 5, 5};
    CHECK(amp::polygons_check(xy.data(), poff.data(), first.data(), n, h, w, &probe_c, &probe_l, probe_i, probe_i, &probe_u, &need) == AMP_OK);
    CHECK(amp::polygons_host(xy.data(), poff.data(), first.data(), n, h, w, &probe_c, 0, &probe_l, probe_i, probe_i, &probe_u, &need) == AMP_ERR_NOMEM);
    CHECK(need == want.size() && probe_c == 5 && probe_l == 5 && probe_u == 5 && probe_i[0] == 5);
    // exactly the need: heap arrays of that size, so one element more is an AddressSanitizer report
    const size_t total = (size_t)need;
    uint32_t* counts = new uint32_t[total];
    unsigned long long* off = new unsigned long long[(size_t)n];
    int *len = new int[(size_t)n], *boxes = new int[4 * (size_t)n];
    unsigned int* areas = new unsigned int[(size_t)n];
    int rc = 1;
    do {
        if (amp::polygons_host(xy.data(), poff.data(), first.data(), n, h, w, counts, total, off, len, boxes, areas, &need) != AMP_OK || need != total) break;
        bool ok = true;
        for (size_t t = 0; t < total; ++t) ok &= counts[t] == want[t];
        for (int i = 0; i < n && ok; ++i) {
            ok &= off[i] == want_off[(size_t)i] && (size_t)len[i] == want_off[(size_t)i + 1] - want_off[(size_t)i];
            int r0 = h, r1 = 0, c0 = w, c1 = 0;
            unsigned int px = 0;
            size_t pos = 0;
            for (int j = 0; j < len[i]; ++j)
                for (uint32_t t = 0; t < counts[off[i] + j]; ++t, ++pos)
                    if (j & 1) { const int c = (int)(pos / h), r = (int)(pos % h); r0 = std::min(r0, r); r1 = std::max(r1, r + 1); c0 = std::min(c0, c); c1 = std::max(c1, c + 1); ++px; }
            ok &= pos == (size_t)h * w && px == areas[i];
            if (px) ok &= boxes[4 * i] == r0 && boxes[4 * i + 1] == c0 && boxes[4 * i + 2] == r1 && boxes[4 * i + 3] == c1;
            else ok &= !boxes[4 * i] && !boxes[4 * i + 1] && !boxes[4 * i + 2] && !boxes[4 * i + 3];
        }
        if (!ok) break;
        if (total && amp::polygons_host(xy.data(), poff.data(), first.data(), n, h, w, counts, total - 1, off, len, boxes, areas, &need) != AMP_ERR_NOMEM) break;
        rc = 0;
    } while (0);
    delete[] counts; delete[] off; delete[] len; delete[] boxes; delete[] areas;
    if (rc) fprintf(stderr, "case %d x %d with %d instances failed (%s)\n", h, w, n, amp::g_err);
    return rc;
}

static int refusals() {
    double xy[16] = {1, 1, 8, 1, 8, 8, 1, 8, 1, 1, 8, 1, 8, 8, 1, 8};
    unsigned long long poff[3] = {0, 8, 16}, l4[4], need = 5;
    int first[3] = {0, 1, 2}, i4[16];
    uint32_t c4[64];
    unsigned int u4[4];
#define REFUSED(XY, POFF, FIRST, N, H, W, NEED) CHECK(amp::polygons_check(XY, POFF, FIRST, N, H, W, c4, l4, i4, i4, u4, NEED) == AMP_ERR_ARG)
    REFUSED(xy, poff, first, -1, 10, 10, &need);
    REFUSED(xy, poff, first, 2, 0, 10, &need);
    REFUSED(xy, poff, first, 2, 10, -3, &need);
    REFUSED(xy, poff, first, 2, 32768, 32769, &need);
    REFUSED(xy, poff, first, 2, 2147483647, 2147483647, &need);
    REFUSED(nullptr, poff, first, 2, 10, 10, &need);
    REFUSED(xy, nullptr, first, 2, 10, 10, &need);
    REFUSED(xy, poff, nullptr, 2, 10, 10, &need);
    REFUSED(xy, poff, first, 2, 10, 10, nullptr);
    { unsigned long long bad[3] = {0, 8, 4}; REFUSED(xy, bad, first, 2, 10, 10, &need); }
    { unsigned long long bad[3] = {0, 8, 15}; REFUSED(xy, bad, first, 2, 10, 10, &need); }
    { unsigned long long bad[3] = {0, 0, 8}; REFUSED(xy, bad, first, 2, 10, 10, &need); }
    { int bad[3] = {0, 2, 2}; REFUSED(xy, poff, bad, 2, 10, 10, &need); }
    { int bad[3] = {-1, 1, 2}; REFUSED(xy, poff, bad, 2, 10, 10, &need); }
    const double bads[4] = {NAN, INFINITY, -INFINITY, 1000000.5};
    for (double b : bads) { double x2[16]; std::copy(xy, xy + 16, x2); x2[11] = b; REFUSED(x2, poff, first, 2, 10, 10, &need); }
    CHECK(need == 5);
    CHECK(amp::polygons_check(xy, poff, first, 2, 10, 10, c4, l4, i4, i4, u4, &need) == AMP_OK);
    CHECK(amp::polygons_check(nullptr, nullptr, nullptr, 0, 10, 10, nullptr, nullptr, nullptr, nullptr, nullptr, &need) == AMP_OK);
    return 0;
}

int main() {
    CHECK(refusals() == 0);
    const int sizes[][2] = {{1, 1}, {1, 40}, {40, 1}, {10, 10}, {37, 53}, {64, 64}, {65, 129}, {130, 70}};
    for (int it = 0; it < 400; ++it) {
        const int h = sizes[it % 8][0], w = sizes[it % 8][1], n = 1 + (int)(rnd() % 4);
        std::vector<std::vector<std::vector<double>>> insts((size_t)n);
        for (auto& inst : insts) {
            inst.resize(1 + rnd() % 5);
            for (auto& p : inst) {
                const int k = 1 + (int)(rnd() % 12);
                const double cx = uni(-0.2, 1.2) * w, cy = uni(-0.2, 1.2) * h, step = (it % 5 == 0) ? 0.0 : (it % 5 == 1 ? 1.0 : it % 5 == 2 ? 0.5 : it % 5 == 3 ? 0.25 : 0.1);
                std::vector<double> ang((size_t)k);
                for (auto& a : ang) a = uni(0, 6.283185307179586);
                if (rnd() % 10 >= 3) std::sort(ang.begin(), ang.end());
                for (int j = 0; j < k; ++j) {
                    const double r = uni(0, 0.6 * std::max(h, w));
                    double x = cx + r * cos(ang[(size_t)j]), y = cy + r * sin(ang[(size_t)j]);
                    if (step > 0) { x = floor(x / step + 0.5) * step; y = floor(y / step + 0.5) * step; }
                    p.push_back(x); p.push_back(y);
                }
            }
        }
        if (it == 7) insts[0][0] = {-1.0e6, -1.0e6, 1.0e6, -1.0e6, 1.0e6, 1.0e6, -1.0e6, 1.0e6};        // the largest coordinates the check lets through
        CHECK(one_case(insts, h, w) == 0);
    }
    printf("POLYGONS SANITIZE OK\n");
    return 0;
}
