// amp_mask_intensity: the grey-level statistics of the micrograph under every mask of a pool, from the run lists.  What the device path
// (mask_intensity.hip) and the host path (mask_intensity_host.hip) share: the sums of one (mask, channel) and how a pixel enters them, the
// size of a work item, and the declarations of the check, the host evaluation and the writer of the outputs.  A COCO run list is a list of
// spans over the column-major flattening of the image; position p is pixel (row p mod h, column p div h).  All arithmetic is integer, so
// the two paths give the same bytes.  Plain C++: the host-only sanitizer build of tests/sanitize includes this header.
//
// The bounds (h, w <= 32768, h * w <= 2^30, v < 2^16): sum v < 2^46, sum v^2 < 2^30 * 2^32 = 2^62, sum r v and sum c v < 2^30 * 2^15 * 2^16
// = 2^61: every sum fits 64 bits.
#pragma once
#include "mask_analysis.h"

namespace amp {

constexpr int MI_PER_LANE = 8;                    // pixel ranks a lane of the reduce kernel reads
constexpr int MI_CHUNK = 256 * MI_PER_LANE;       // pixel ranks of one work item (a workgroup of 256): tests/mask_intensity_cases.py cuts masks here
constexpr int MI_MAX_BINS = 4096;                 // bins of a histogram: one LDS table of 16 KiB per workgroup and channel
constexpr int MI_RAW = AMP_INTENSITY_NVALS;       // words of one (mask, channel) as both paths leave them for mask_intensity_write

// the sums of one (mask, channel); slots 1 .. 6 of its eight words
struct MiSums {
    u64 sv, svv, srv, scv;
    uint32_t mn, mx;
};
AMP_HD MiSums mi_none() { return MiSums{0, 0, 0, 0, 0xffffffffu, 0}; }
// pixel (r, c) of value v
AMP_HD void mi_add(MiSums& a, uint32_t v, uint32_t r, uint32_t c) {
    a.sv += v;
    a.svv += (u64)v * (u64)v;
    a.srv += (u64)r * (u64)v;
    a.scv += (u64)c * (u64)v;
    a.mn = v < a.mn ? v : a.mn;
    a.mx = v > a.mx ? v : a.mx;
}

// The argument check: everything but the capacity.  plan: every mask; nbins: 0 without a histogram.
int mask_intensity_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const void* image, int channels,
                         int depth, int hist_shift, const unsigned long long* vals, const uint32_t* hist, const unsigned long long* need,
                         RunPlan& plan, u64& nbins);
// need[0] = n * channels * nbins; AMP_ERR_NOMEM when hist_cap is below it
int mask_intensity_capacity(int n, int channels, u64 nbins, unsigned long long hist_cap, unsigned long long* need);
// The evaluation with a NULL context.  raw [n][channels][MI_RAW]: slots 1 .. 4 the sums, 5 the minimum (all ones where the mask has no
// pixel), 6 the maximum -- the words the kernel's atomics leave; hist (nbins != 0) [n][channels][nbins], every word written.
void mask_intensity_host(const RunPlan& plan, int h, int w, const void* image, int channels, int depth, int hist_shift, u64 nbins,
                         std::vector<u64>& raw, uint32_t* hist);
// vals from raw and the plan's areas: {N, sum v, sum v^2, sum r v, sum c v, min, max, 0}, eight zeros for an empty mask
void mask_intensity_write(const RunPlan& plan, int channels, const std::vector<u64>& raw, unsigned long long* vals);

}  // namespace amp
