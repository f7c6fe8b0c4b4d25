// What the host-only sanitizer programs of this directory share: the amp::set_error the library code under test calls (its last message is
// kept for the reports), the xorshift generator, the CHECK that ends a program with the line and that message, and the dense-mask encoder
// of the programs that build their inputs from pixel arrays.  Included after <stdint.h> / <vector> users' own headers; a program that wants
// another sequence defines SANITIZE_SEED first.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace amp {
static char g_err[1024];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace amp

#ifndef SANITIZE_SEED
#define SANITIZE_SEED 0x9E3779B97F4A7C15ull
#endif
static unsigned long long rng_state = SANITIZE_SEED;
static inline unsigned int rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned int)(rng_state >> 11); }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "CHECK failed line %d: %s (%s)\n", __LINE__, #cond, amp::g_err); return 1; } } while (0)

// a dense row-major mask as COCO counts (column-major, zeros first); loose: zero-length runs are put in here and there
static inline std::vector<uint32_t> encode(const std::vector<int>& m, int h, int w, bool loose) {
    std::vector<uint32_t> c;
    int cur = 0;
    uint32_t run = 0;
    for (int x = 0; x < w; ++x)
        for (int y = 0; y < h; ++y) {
            const int v = m[(size_t)y * w + x];
            if (v != cur) { c.push_back(run); run = 0; cur = v; }
            if (loose && run == 2) { c.push_back(2); c.push_back(0); run = 0; }          // the same colour goes on behind an empty run of the other
            ++run;
        }
    c.push_back(run);
    return c;
}
