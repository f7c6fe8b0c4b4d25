// amp_seg_class_map: the word arithmetic that the host evaluation (mask_analysis_host.hip) and the device kernels (seg_class_map.hip) share, so the two
// paths cannot drift apart.  A word is 64 rows of one column of the three image planes TP / FN / FP (bit b = row 64 wv + b); from the three
// words of a place come the pixels of a code, the pixels of a class of the mode and the run boundaries the word contributes to the class's
// column-major run list.  Plain C++ (the host-only sanitizer builds compile it with g++), integers throughout.
#pragma once
#include "run_list.h"

namespace amp {

AMP_HD int sc_classes(int mode) { return mode ? 7 : 4; }

// the rows of word wv that exist in a column of h rows: the padding rows of a column's last word never count
AMP_HD u64 sc_valid(int h, int wv) {
    const int left = h - (wv << 6);
    return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}

// pixels whose code TP + 2 FN + 4 FP is `code` (padding rows included for code 0: AND with sc_valid)
AMP_HD u64 sc_code_word(u64 tp, u64 fn, u64 fp, int code) {
    return ((code & 1) ? tp : ~tp) & ((code & 2) ? fn : ~fn) & ((code & 4) ? fp : ~fp);
}

// pixels of class k.  mode 1 ('all'): code k + 1.  mode 0 ('reduced'): TP only, FN only, FP only, more than one of them
AMP_HD u64 sc_class_word(u64 tp, u64 fn, u64 fp, int mode, int k) {
    if (mode) return sc_code_word(tp, fn, fp, k + 1);
    if (k < 3) return sc_code_word(tp, fn, fp, 1 << k);
    return (tp & fn) | (tp & fp) | (fn & fp);
}

// the bit of the plane word in front of word u = col * pitch + wv in column-major order that holds the pixel before the word's first one:
// row 63 of the word above, or the last row of the previous column (u > 0)
AMP_HD int sc_prev_bit(int h, int wv) { return wv > 0 ? 63 : ((h - 1) & 63); }

// bit b set: the class changes between the pixel before row b of the word and row b.  x: the class word, already ANDed with `valid`;
// prev: the class at the pixel before the word's first (0 in front of the image's first pixel)
AMP_HD u64 sc_transitions(u64 x, u64 prev, u64 valid) { return (x ^ ((x << 1) | (prev & 1ull))) & valid; }

}  // namespace amp
