// amp_seg_class_map: the word arithmetic that the host evaluation (rle_host.hip) and the device kernels (seg_class_map.hip) share, so the two
// paths cannot drift apart.  A word is 64 rows of one column of the three image planes TP / FN / FP (bit b = row 64 wv + b); from the three
// words of a place come the pixels of a code, the pixels of a class of the mode and the run boundaries the word contributes to the class's
// column-major run list.  Plain C++ (the host-only sanitizer builds compile it with g++), integers throughout.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define AMP_SC_HD __host__ __device__ __forceinline__
#else
#define AMP_SC_HD inline
#endif

namespace amp {

typedef unsigned long long sc_u64;

AMP_SC_HD int sc_classes(int mode) { return mode ? 7 : 4; }

// the rows of word wv that exist in a column of h rows: the padding rows of a column's last word never count
AMP_SC_HD sc_u64 sc_valid(int h, int wv) {
    const int left = h - (wv << 6);
    return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}

// pixels whose code TP + 2 FN + 4 FP is `code` (padding rows included for code 0: AND with sc_valid)
AMP_SC_HD sc_u64 sc_code_word(sc_u64 tp, sc_u64 fn, sc_u64 fp, int code) {
    return ((code & 1) ? tp : ~tp) & ((code & 2) ? fn : ~fn) & ((code & 4) ? fp : ~fp);
}

// pixels of class k.  mode 1 ('all'): code k + 1.  mode 0 ('reduced'): TP only, FN only, FP only, more than one of them
AMP_SC_HD sc_u64 sc_class_word(sc_u64 tp, sc_u64 fn, sc_u64 fp, int mode, int k) {
    if (mode) return sc_code_word(tp, fn, fp, k + 1);
    if (k < 3) return sc_code_word(tp, fn, fp, 1 << k);
    return (tp & fn) | (tp & fp) | (fn & fp);
}

// the bit of the plane word in front of word u = col * pitch + wv in column-major order that holds the pixel before the word's first one:
// row 63 of the word above, or the last row of the previous column (u > 0)
AMP_SC_HD int sc_prev_bit(int h, int wv) { return wv > 0 ? 63 : ((h - 1) & 63); }

// bit b set: the class changes between the pixel before row b of the word and row b.  x: the class word, already ANDed with `valid`;
// prev: the class at the pixel before the word's first (0 in front of the image's first pixel)
AMP_SC_HD sc_u64 sc_transitions(sc_u64 x, sc_u64 prev, sc_u64 valid) { return (x ^ ((x << 1) | (prev & 1ull))) & valid; }

AMP_SC_HD int sc_popc(sc_u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
AMP_SC_HD int sc_ctz(sc_u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}

}  // namespace amp
