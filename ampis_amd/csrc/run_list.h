// What the mask analyses on COCO run lists share (edge distance, region properties, group overlap, segmentation class map; host evaluations in
// mask_analysis_host.hip, kernels in the four .hip files): the one walk over a list of run lengths that validates it and adds it to a plan,
// the plan itself, and the painter of pixels [s, e) into a column-major bit plane of 64 rows a word.  The host and the device path of an
// analysis use the same functions here, so they cannot drift apart.  Plain C++ (the host-only sanitizer builds compile it with g++), integers
// throughout; the helpers that need a wavefront or LDS are at the end, for hipcc only.
#pragma once
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define AMP_HD __host__ __device__ __forceinline__
#else
#define AMP_HD inline
#endif

namespace amp {

typedef unsigned long long u64;                   // one word of a bit plane: bit b = row 64 wv + b of a column

AMP_HD int popc(u64 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}
AMP_HD int ctz(u64 x) {               // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((long long)x) - 1;
#else
    return __builtin_ctzll(x);
#endif
}
AMP_HD int clz(u64 x) {               // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// bits [lo, hi) of a word, 0 <= lo < hi <= 64
AMP_HD u64 word_span(int lo, int hi) { return (hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull); }

// how a painter ORs a word: kernels pass OrAtomic (the runs of one column share words), the host OrPlain
struct OrPlain {
    AMP_HD void operator()(u64* p, u64 m) const { *p |= m; }
};
#ifdef __HIPCC__
struct OrAtomic {
    __device__ __forceinline__ void operator()(u64* p, u64 m) const { atomicOr(p, m); }
};
#endif

// Pixels [s, e) of the column-major image of height h (s < e <= h * w <= 2^30) into a column-major plane with origin (r0, c0), extent H x W
// and pitch = ceil(H / 64) words a column.  CLIP: the part outside the plane is dropped; without it the caller promises there is none (a
// mask's tight box, the full image: r0 = c0 = 0, H = h).
template <bool CLIP, class Or>
AMP_HD void paint_run(unsigned int s, unsigned int e, int h, u64* plane, int r0, int c0, int H, int W, int pitch, Or or_word) {
    int c_first = (int)(s / (unsigned)h), c_last = (int)((e - 1) / (unsigned)h);
    if (CLIP) {
        c_first = c_first > c0 ? c_first : c0;
        c_last = c_last < c0 + W - 1 ? c_last : c0 + W - 1;
    }
    for (int c = c_first; c <= c_last; ++c) {
        const unsigned int cb = (unsigned)c * (unsigned)h;
        int ya = (int)((s > cb ? s : cb) - cb) - r0, yb = (int)((e < cb + (unsigned)h ? e : cb + (unsigned)h) - cb) - r0;       // rows [ya, yb) of the plane
        if (CLIP) {
            ya = ya > 0 ? ya : 0;
            yb = yb < H ? yb : H;
            if (yb <= ya) continue;
        }
        u64* col = plane + (size_t)(c - c0) * pitch;
        for (int wv = ya >> 6; wv <= (yb - 1) >> 6; ++wv) {
            const int lo = ya - (wv << 6), hi = yb - (wv << 6);
            or_word(&col[wv], word_span(lo > 0 ? lo : 0, hi < 64 ? hi : 64));
        }
    }
}

// The plan of a pool of masks.  Per planned mask its non-empty runs of ones k = 0 .. n - 1 as pixel positions [S[ro + k], E[ro + k]) of the
// column-major image and one closing entry S = E = 0xffffffff, so that "the first run that ends beyond x" needs no special case at the end of
// the list.  P (only when asked for): P[ro + k] = the pixels of the runs before k, P[ro + n] = the area.
struct RunMask {
    unsigned int ro;              // where the mask's entries start in S / E / P
    int n;                        // runs of ones (0: an empty mask, its box is all zeros and meets nothing; -1: not planned, never read)
    int r0, c0, r1, c1;           // the tight box, ends exclusive
    unsigned int area;
};
struct RunPlan {
    std::vector<uint32_t> S, E, P;
    std::vector<RunMask> m;
    // n masks, none planned yet
    void reset(size_t n) { S.clear(); E.clear(); P.clear(); m.assign(n, RunMask{0, -1, 0, 0, 0, 0, 0}); }
};

enum RunListFault {
    RUNS_OK = 0,
    RUNS_EMPTY,                   // no run at all
    RUNS_OVER,                    // the runs cover more than h * w pixels
    RUNS_SHORT,                   // they cover *covered < h * w pixels
    RUNS_TOO_MANY                 // the plan would pass 2^31 entries
};

// One walk over the run lengths c[0 .. len) of a mask of an h x w image (h * w <= 2^30; zeros first, COCO order): refuses what is not a run
// list of the image, skips zero-length runs, appends the runs of ones to the plan and fills m[idx] with their number, the area and the tight
// box.  A run that crosses a column end covers the last and the first row.  Nothing is read when len <= 0, nothing beyond c[len - 1] ever.
inline RunListFault plan_add_mask(RunPlan& pl, size_t idx, const uint32_t* c, int len, int h, int w, bool prefix, u64* covered) {
    *covered = 0;
    if (len <= 0) return RUNS_EMPTY;
    const u64 image = (u64)h * (u64)w;
    RunMask e{(unsigned int)pl.S.size(), 0, 0, 0, 0, 0, 0};
    u64 pos = 0, ones = 0;
    int r0 = h, r1 = -1, c0 = w, c1 = -1;
    for (int j = 0; j < len; ++j) {
        const u64 s = pos, t = pos + c[j];
        pos = t;
        if (t > image) return RUNS_OVER;
        if (!(j & 1) || t == s) continue;
        pl.S.push_back((uint32_t)s); pl.E.push_back((uint32_t)t);
        if (prefix) pl.P.push_back((uint32_t)ones);
        ones += t - s;
        const int cf = (int)(s / (unsigned)h), cl = (int)((t - 1) / (unsigned)h);
        c0 = cf < c0 ? cf : c0; c1 = cl > c1 ? cl : c1;
        if (cf != cl) { r0 = 0; r1 = h - 1; continue; }
        const int ra = (int)(s % (unsigned)h), rb = (int)((t - 1) % (unsigned)h);
        r0 = ra < r0 ? ra : r0; r1 = rb > r1 ? rb : r1;
    }
    *covered = pos;
    if (pos != image) return RUNS_SHORT;
    e.n = (int)(pl.S.size() - e.ro);
    e.area = (unsigned int)ones;
    if (e.n) { e.r0 = r0; e.c0 = c0; e.r1 = r1 + 1; e.c1 = c1 + 1; }
    pl.S.push_back(0xffffffffu); pl.E.push_back(0xffffffffu);
    if (prefix) pl.P.push_back((uint32_t)ones);
    if (pl.S.size() >= (1ull << 31)) return RUNS_TOO_MANY;
    pl.m[idx] = e;
    return RUNS_OK;
}

#ifdef __HIPCC__
// sum over the 64 lanes, valid in lane 0
__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the owner of item x among n ranges: off[i] <= x < off[i + 1] (ascending offsets; an empty range is never found), x < off[n]
__device__ __forceinline__ int owner_of(const u64* __restrict__ off, int n, u64 x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// the first of n runs that ends beyond position x (E: the run ends, ascending); n when there is none: the closing entry
__device__ __forceinline__ int first_run_ending_after(const unsigned int* __restrict__ E, int n, unsigned int x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (E[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the 64 rows [a, a + 64) of the column-major image of one mask as a word, a and b pixel positions with b <= a + 64 the end of the word or of
// its column.  S, E: the run starts and ends, ascending; S[n] = 0xffffffff closes the list
__device__ __forceinline__ u64 mask_word(const unsigned int* __restrict__ S, const unsigned int* __restrict__ E, int n, unsigned int a,
                                         unsigned int b) {
    u64 word = 0;
    for (int k = first_run_ending_after(E, n, a); S[k] < b; ++k)                               // k <= n: the closing entry stops the walk
        word |= word_span((int)(max(S[k], a) - a), (int)(min(E[k], b) - a));                   // bits [from, to), 0 <= from < to <= 64
    return word;
}

// mask_word with the pixels above and below it: positions [a, b) of one column [cb, ce) as the word, *up = the mask at a - 1 (0 when a is
// the column's first row), *down = the mask at b (0 when b is the column's end).  One search, then the runs in order.
__device__ __forceinline__ u64 mask_word_halo(const unsigned int* __restrict__ S, const unsigned int* __restrict__ E, int n, unsigned int cb,
                                              unsigned int ce, unsigned int a, unsigned int b, u64* up, u64* down) {
    const unsigned int a1 = a > cb ? a - 1 : a, b1 = b < ce ? b + 1 : b;
    u64 word = 0;
    *up = 0; *down = 0;
    for (int k = first_run_ending_after(E, n, a1); S[k] < b1; ++k) {
        unsigned int s = max(S[k], a1), e = min(E[k], b1);
        if (s < a) { *up = 1; s = a; }
        if (e > b) { *down = 1; e = b; }
        if (s < e) word |= word_span((int)(s - a), (int)(e - a));
    }
    return word;
}

// Inclusive scan of one value per thread over a workgroup of 1024, in the LDS array s[1024]; every thread calls it.  A fixed tree and no
// atomics: the order is fixed and the bytes repeat.  s[1023] is the total once it returns.
__device__ __forceinline__ u64 block_scan_1024(u64* s, u64 v) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const u64 b = tid >= o ? s[tid - o] : 0ull;
        __syncthreads();
        s[tid] += b;
        __syncthreads();
    }
    return s[tid];
}
#endif  // __HIPCC__

}  // namespace amp
