// Host-only AddressSanitizer / UBSan run of amp_render_instances' argument checks, plan and host drawing (ampis_amd/csrc/mask_analysis_host.hip:
// amp::render_check / amp::render_host, what the call runs with a NULL context): the shapes of tests/render_cases.py restated (heights and widths
// 1, 2, 63, 64, 65, 130; empty and full masks, masks owning the corners, noise; boxes on the border, inverted and thinner than the line) against
// a per-pixel evaluation written here, the image and output buffers of exactly h * w * 3 bytes, and hostile input.  Built and run by
// tests/test_render_sanitize.py like the runs beside it.  The device kernel indexes only what these checks let through.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
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

// kind 0 empty, 1 full, 2 the corners and the border rows, 3 full columns, otherwise a noisy box
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

static int one_case(int h, int w, int n, int it) {
    const bool with_masks = it % 5 != 1, with_boxes = it % 5 != 0, with_edge = it % 3 != 2;
    const int lw = 1 + it % 4;
    Pool P;
    for (int i = 0; with_masks && i < n; ++i) CHECK(add_mask(P, h, w, (it + i) % 7) == 0);
    const size_t bytes = (size_t)h * w * 3;
    std::vector<uint8_t> img(bytes), tab((size_t)n * 768 + 1), rgb((size_t)n * 6 + 1);
    for (auto& v : img) v = (uint8_t)rnd();
    for (auto& v : tab) v = (uint8_t)rnd();
    for (auto& v : rgb) v = (uint8_t)rnd();
    const uint8_t *edge = rgb.data(), *brgb = rgb.data() + 3 * (size_t)n;
    std::vector<int> boxes((size_t)n * 4 + 1);
    for (int i = 0; i < n; ++i) {                                                 // any corner order: inverted boxes are valid
        boxes[4 * i] = rnd() % w; boxes[4 * i + 1] = rnd() % h; boxes[4 * i + 2] = rnd() % w; boxes[4 * i + 3] = rnd() % h;
        if (i == 0) { boxes[0] = boxes[1] = 0; boxes[2] = w - 1; boxes[3] = h - 1; }
    }
    // the per-pixel evaluation: instance by instance on a copy
    std::vector<uint8_t> want = img;
    auto in = [&](const std::vector<uint8_t>& m, int y, int x) { return y >= 0 && y < h && x >= 0 && x < w && m[(size_t)x * h + y]; };
    for (int i = 0; i < n; ++i) {
        if (with_masks) {
            const std::vector<uint8_t>& m = P.bits[i];
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    if (!m[(size_t)x * h + y]) continue;
                    const bool inner = in(m, y - 1, x) && in(m, y + 1, x) && in(m, y, x - 1) && in(m, y, x + 1) && y > 0 && y < h - 1 && x > 0 && x < w - 1;
                    uint8_t* px = &want[((size_t)y * w + x) * 3];
                    for (int c = 0; c < 3; ++c) px[c] = with_edge && !inner ? edge[3 * i + c] : tab[768 * (size_t)i + 3 * px[c] + c];
                }
        }
        if (with_boxes) {
            const int x0 = boxes[4 * i], y0 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], y1 = boxes[4 * i + 3];
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const bool cols = x >= x0 && x <= x1, rows = y >= y0 && y <= y1;
                    const bool hit = (cols && y >= y0 && y < std::min(y0 + lw, h)) || (cols && y >= std::max(y1 - lw + 1, 0) && y <= y1) ||
                                     (rows && x >= x0 && x < std::min(x0 + lw, w)) || (rows && x >= std::max(x1 - lw + 1, 0) && x <= x1);
                    if (hit) memcpy(&want[((size_t)y * w + x) * 3], brgb + 3 * i, 3);
                }
        }
    }
    const uint32_t* pool = with_masks ? P.pool.data() : nullptr;
    const int* bx = with_boxes ? boxes.data() : nullptr;
    amp::RunPlan runs;
    std::vector<int> rects;
    std::vector<uint8_t> out = img;                                               // exactly h * w * 3 bytes
    CHECK(amp::render_check(img.data(), h, w, pool, P.off.data(), P.len.data(), n, tab.data(), with_edge ? edge : nullptr, bx, brgb, lw, out.data(),
                            runs, rects) == AMP_OK);
    CHECK(amp::render_host(runs, tab.data(), with_edge ? edge : nullptr, rects, brgb, n, h, w, out.data()) == AMP_OK);
    CHECK(out == want);
    // hostile input: every one refused by the check
#define REFUSED(IMG, HH, WW, POOL, LEN, N, TAB, BX, BRGB, LW)                                                                       \
    CHECK(amp::render_check(IMG, HH, WW, POOL, P.off.data(), LEN, N, TAB, edge, BX, BRGB, LW, out.data(), runs, rects) == AMP_ERR_ARG)
    REFUSED(nullptr, h, w, pool, P.len.data(), n, tab.data(), bx, brgb, lw);
    REFUSED(img.data(), h, w, pool, P.len.data(), -1, tab.data(), bx, brgb, lw);
    REFUSED(img.data(), h, w, pool, P.len.data(), n, tab.data(), bx, brgb, 0);
    REFUSED(img.data(), 0, w, pool, P.len.data(), n, tab.data(), bx, brgb, lw);
    REFUSED(img.data(), 32769, 32769, pool, P.len.data(), n, tab.data(), bx, brgb, lw);
    if (with_masks && n > 0) {
        std::vector<uint32_t> bad = P.pool;
        bad[P.off[n - 1]] += 1;                                                   // runs that do not sum to h * w
        REFUSED(img.data(), h, w, bad.data(), P.len.data(), n, tab.data(), bx, brgb, lw);
        bad = P.pool;
        bad[P.off[0]] = 0xffffffffu;                                              // a run far beyond the image
        REFUSED(img.data(), h, w, bad.data(), P.len.data(), n, tab.data(), bx, brgb, lw);
        std::vector<int> len2 = P.len;
        len2[n / 2] = 0;                                                          // an empty run list
        REFUSED(img.data(), h, w, pool, len2.data(), n, tab.data(), bx, brgb, lw);
        REFUSED(img.data(), h, w, pool, nullptr, n, tab.data(), bx, brgb, lw);
        REFUSED(img.data(), h, w, pool, P.len.data(), n, nullptr, bx, brgb, lw);
        REFUSED(img.data(), h + 1, w, pool, P.len.data(), n, tab.data(), nullptr, brgb, lw);
    }
    if (with_boxes && n > 0) {
        REFUSED(img.data(), h, w, pool, P.len.data(), n, tab.data(), bx, nullptr, lw);
        std::vector<int> far = boxes;
        far[4 * (n - 1) + 2] = w;                                                 // a corner outside the image
        REFUSED(img.data(), h, w, pool, P.len.data(), n, tab.data(), far.data(), brgb, lw);
        far = boxes;
        far[1] = -1;
        REFUSED(img.data(), h, w, pool, P.len.data(), n, tab.data(), far.data(), brgb, lw);
        far = boxes;
        far[4 * (n - 1) + 3] = 0x7fffffff;
        REFUSED(img.data(), h, w, pool, P.len.data(), n, tab.data(), far.data(), brgb, 0x7fffffff);
    }
    // a line width beyond any int sum: valid, the frame fills the box
    CHECK(amp::render_check(img.data(), h, w, nullptr, nullptr, nullptr, n, nullptr, nullptr, boxes.data(), brgb, 0x7fffffff, out.data(), runs, rects) == AMP_OK);
    CHECK(amp::render_host(runs, nullptr, nullptr, rects, brgb, n, h, w, out.data()) == AMP_OK);
    return 0;
}

int main() {
    const int sizes[] = {1, 2, 63, 64, 65, 130};
    int it = 0;
    for (int h : sizes)
        for (int w : sizes) { CHECK(one_case(h, w, 1 + it % 5, it) == 0); ++it; }
    for (int n : {0, 1, 12}) CHECK(one_case(70, 75, n, it++) == 0);
    for (; it < 160; ++it) {
        const int h = 1 + rnd() % (it % 3 ? 40 : 140), w = 1 + rnd() % (it % 4 ? 40 : 140);
        CHECK(one_case(h, w, rnd() % 13, it) == 0);
    }
    printf("RENDER SANITIZE OK\n");
    return 0;
}
