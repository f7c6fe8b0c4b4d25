// Host-only AddressSanitizer / UBSan run of amp_label_runs' argument check and host evaluation (ampis_amd/csrc/label_runs_host.hip:
// amp::label_runs_check / amp::label_runs_host, what the call runs with a NULL context): the hand shapes of tests/label_runs_cases.py restated (one
// pixel, one row, one column, 63 / 64 / 65 / 129 rows, empty, full, checkerboard, serpentine, comb) and random images of both kinds and both
// connectivities, every instance compared with a per-pixel flood fill written here, every buffer of exactly the capacity asked for, and the
// refusals.  Built and run by tests/test_label_runs_sanitize.py like the class-map run beside it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../ampis_amd/csrc/mask_analysis.h"
#include "../../include/ampis_hip.h"
#include "sanitize_common.h"

// the instance number (1 ..) of every pixel by definition: flood fill in row-major order of the first pixel (BINARY), rank of the id (LABEL)
static std::vector<int> reference_labels(const std::vector<int>& img, int h, int w, int kind, int conn, int zero_bg, std::vector<int>* ids) {
    std::vector<int> lab((size_t)h * w, 0);
    ids->clear();
    if (kind == AMP_LABEL_IDS) {
        std::map<int, int> rank;
        for (int v : img) if (v != 0 || !zero_bg) rank[v] = 0;
        int n = 0;
        for (auto& kv : rank) { kv.second = ++n; ids->push_back(kv.first); }
        for (size_t i = 0; i < img.size(); ++i) if (img[i] != 0 || !zero_bg) lab[i] = rank[img[i]];
        return lab;
    }
    int n = 0;
    std::vector<int> stack;
    for (int i = 0; i < h * w; ++i) {
        if (!img[i] || lab[i]) continue;
        lab[i] = ++n;
        ids->push_back(n);
        stack.assign(1, i);
        while (!stack.empty()) {
            const int p = stack.back(), r = p / w, c = p % w;
            stack.pop_back();
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    if ((!dr && !dc) || (conn == 1 && dr && dc)) continue;
                    const int y = r + dr, x = c + dc;
                    if (y < 0 || y >= h || x < 0 || x >= w || !img[y * w + x] || lab[y * w + x]) continue;
                    lab[y * w + x] = n;
                    stack.push_back(y * w + x);
                }
        }
    }
    return lab;
}

static int one_case(const std::vector<int>& img, int h, int w, int kind, int conn, int zero_bg) {
    std::vector<uint8_t> bytes(img.begin(), img.end());              // BINARY: any nonzero byte is foreground
    if (kind == AMP_LABEL_BINARY) for (size_t i = 0; i < img.size(); ++i) bytes[i] = img[i] ? (uint8_t)(1 + i % 255) : 0;
    const void* image = kind == AMP_LABEL_BINARY ? (const void*)bytes.data() : (const void*)img.data();
    std::vector<int> want_ids;
    const std::vector<int> want = reference_labels(img, h, w, kind, conn, zero_bg, &want_ids);
    unsigned long long need[2] = {77, 77};
    int probe_i[4] = {0, 0, 0, 0};
    unsigned int probe_u = 0;
    unsigned long long probe_l = 0;
    CHECK(amp::label_runs_check(image, h, w, kind, conn, probe_i, probe_i, &probe_u, &probe_u, &probe_l, probe_i, 0, need) == AMP_OK);
    int st = amp::label_runs_host(image, h, w, kind, conn, zero_bg, probe_i, probe_i, &probe_u, &probe_u, &probe_l, probe_i, 0, 0, nullptr, need);
    const size_t n = (size_t)need[0], total = (size_t)need[1];
    CHECK(n == want_ids.size());
    CHECK(st == (n ? AMP_ERR_NOMEM : AMP_OK) && probe_i[0] == 0 && probe_u == 0 && probe_l == 0);
    // exactly the need: heap arrays of that size, so one element more is an AddressSanitizer report
    int *ids = new int[n], *boxes = new int[4 * n], *len = new int[n], *labels = new int[(size_t)h * w];
    unsigned int *areas = new unsigned int[n], *counts = new unsigned int[total];
    unsigned long long* off = new unsigned long long[n];
    st = amp::label_runs_host(image, h, w, kind, conn, zero_bg, ids, boxes, areas, counts, off, len, (int)n, total, labels, need);
    int rc = 1;
    do {
        if (st != AMP_OK || need[0] != n || need[1] != total) break;
        bool ok = true;
        for (size_t i = 0; i < (size_t)h * w; ++i) ok &= labels[i] == want[i];
        size_t at = 0;
        for (size_t k = 0; k < n && ok; ++k) {
            ok &= ids[k] == want_ids[k] && off[k] == at && len[k] >= 2;
            int r0 = h, r1 = 0, c0 = w, c1 = 0;
            unsigned int px = 0;
            size_t pos = 0;
            for (int j = 0; j < len[k] && ok; ++j) {
                ok &= j == 0 || counts[at + j] > 0;                  // only the first count may be 0
                for (unsigned int t = 0; t < counts[at + j] && ok; ++t, ++pos) {
                    ok &= pos < (size_t)h * w;
                    if (!ok) break;
                    const int c = (int)(pos / h), r = (int)(pos % h), in = want[(size_t)r * w + c] == (int)k + 1;
                    ok &= in == (j & 1);
                    if (in) { r0 = std::min(r0, r); r1 = std::max(r1, r + 1); c0 = std::min(c0, c); c1 = std::max(c1, c + 1); ++px; }
                }
            }
            ok &= pos == (size_t)h * w && px == areas[k] && px > 0;
            ok &= boxes[4 * k] == r0 && boxes[4 * k + 1] == c0 && boxes[4 * k + 2] == r1 && boxes[4 * k + 3] == c1;
            at += len[k];
        }
        if (!ok || at != total) break;
        if (n) {                                                     // one less of either capacity: refused
            if (amp::label_runs_host(image, h, w, kind, conn, zero_bg, ids, boxes, areas, counts, off, len, (int)n - 1, total, labels, need) != AMP_ERR_NOMEM) break;
            if (amp::label_runs_host(image, h, w, kind, conn, zero_bg, ids, boxes, areas, counts, off, len, (int)n, total - 1, labels, need) != AMP_ERR_NOMEM) break;
        }
        rc = 0;
    } while (0);
    delete[] ids; delete[] boxes; delete[] len; delete[] labels; delete[] areas; delete[] counts; delete[] off;
    if (rc) fprintf(stderr, "case %d x %d kind %d connectivity %d failed (%s)\n", h, w, kind, conn, amp::g_err);
    return rc;
}

static int shapes() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {63, 5}, {64, 5}, {65, 5}, {129, 3}, {16, 16}, {65, 65}, {21, 30}};
    for (const auto& s : sizes) {
        const int h = s[0], w = s[1];
        for (int pattern = 0; pattern < 6; ++pattern) {
            std::vector<int> img((size_t)h * w, 0);
            for (int r = 0; r < h; ++r)
                for (int c = 0; c < w; ++c) {
                    int v = 0;
                    if (pattern == 1) v = 1;                                                                 // full
                    if (pattern == 2) v = (r + c) % 2 == 0;                                                 // checkerboard
                    if (pattern == 3) v = c % 2 == 0 || r == ((c / 2) % 2 ? 0 : h - 1);                     // serpentine
                    if (pattern == 4) v = r % 2 == 0 || c == w - 1;                                         // comb: the arms meet in the last column
                    if (pattern == 5) v = (r >= 1 && r < h - 1 && c == w / 2) || (r == h - 1 && c + 1 < w) || (r == 0 && c > 0);      // word edges, column ends
                    img[(size_t)r * w + c] = v;
                }
            for (int conn = 1; conn <= 2; ++conn) CHECK(one_case(img, h, w, AMP_LABEL_BINARY, conn, 1) == 0);
            for (size_t i = 0; i < img.size(); ++i) img[i] = img[i] ? (int)(i % 3 ? 0x7fffffff - (int)(i % 5) : -0x7fffffff - 1 + (int)(i % 2)) : 0;
            CHECK(one_case(img, h, w, AMP_LABEL_IDS, 2, 1) == 0);
            CHECK(one_case(img, h, w, AMP_LABEL_IDS, 1, 0) == 0);
        }
    }
    return 0;
}

static int refusals() {
    uint8_t img[6] = {1, 0, 1, 1, 0, 1};
    int i4[16];
    unsigned int u4[16];
    unsigned long long l4[4], need[2] = {5, 5};
#define REFUSED(IMG, H, W, KIND, CONN, IDS, CAP, NEED) CHECK(amp::label_runs_check(IMG, H, W, KIND, CONN, IDS, i4, u4, u4, l4, i4, CAP, NEED) == AMP_ERR_ARG)
    REFUSED(img, 0, 3, 0, 2, i4, 4, need);
    REFUSED(img, 2, -1, 0, 2, i4, 4, need);
    REFUSED(img, 32768, 32769, 0, 2, i4, 4, need);
    REFUSED(img, 2147483647, 2147483647, 1, 2, i4, 4, need);
    REFUSED(img, 2, 3, 2, 2, i4, 4, need);
    REFUSED(img, 2, 3, 0, 0, i4, 4, need);
    REFUSED(img, 2, 3, 0, 3, i4, 4, need);
    REFUSED(img, 2, 3, 0, 2, i4, -1, need);
    REFUSED(nullptr, 2, 3, 0, 2, i4, 4, need);
    REFUSED(img, 2, 3, 0, 2, nullptr, 4, need);
    REFUSED(img, 2, 3, 0, 2, i4, 4, nullptr);
    CHECK(need[0] == 5 && need[1] == 5);
    CHECK(amp::label_runs_check(img, 2, 3, 0, 2, i4, i4, u4, u4, l4, i4, 4, need) == AMP_OK);
    return 0;
}

int main() {
    CHECK(shapes() == 0);
    CHECK(refusals() == 0);
    for (int it = 0; it < 300; ++it) {
        const int h = 1 + rnd() % (it % 3 ? 40 : 96), w = 1 + rnd() % (it % 5 ? 40 : 96), kind = it % 2;
        const unsigned int density = 5 + rnd() % 91, nid = 1 + rnd() % 9;
        std::vector<int> img((size_t)h * w);
        for (auto& v : img) v = rnd() % 100 < density ? (kind ? (int)(rnd() % nid) - (it % 4 == 3 ? 2 : 0) : 1) : 0;
        CHECK(one_case(img, h, w, kind, 1 + (it / 2) % 2, it % 4 != 3) == 0);
    }
    printf("LABEL RUNS SANITIZE OK\n");
    return 0;
}
