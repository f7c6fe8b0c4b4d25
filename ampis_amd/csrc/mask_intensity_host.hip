// Host side of amp_mask_intensity (mask_intensity.h): the argument check, whose plan both paths evaluate, the capacity report, the evaluation
// with a NULL context -- every run of ones cut at the column ends, the row-major image read at stride w * channels --, and the outputs from
// the per-(mask, channel) words of either path.  Plain C++ throughout, integers only: the host-only sanitizer build of tests/sanitize compiles
// this file with g++.  mask_intensity.hip computes the same bytes on the device.
#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "mask_intensity.h"

namespace amp {

int mask_intensity_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const void* image, int channels,
                         int depth, int hist_shift, const unsigned long long* vals, const uint32_t* hist, const unsigned long long* need,
                         RunPlan& plan, u64& nbins) {
    nbins = 0;
    AMP_REQUIRE(n >= 0, "amp_mask_intensity: n = %d", n);
    AMP_TRY_STATUS(require_image_size("amp_mask_intensity", h, w));
    AMP_REQUIRE(channels >= 1 && channels <= 4, "amp_mask_intensity: channels = %d (1 .. 4)", channels);
    AMP_REQUIRE(depth == 8 || depth == 16, "amp_mask_intensity: depth = %d (8 or 16)", depth);
    AMP_REQUIRE(hist_shift >= -1 && hist_shift <= depth, "amp_mask_intensity: hist_shift = %d (-1: no histogram, or 0 .. %d)", hist_shift, depth);
    AMP_REQUIRE(hist_shift < 0 || depth - hist_shift <= 12, "amp_mask_intensity: hist_shift = %d at depth %d asks for %d bins (at most %d)",
                hist_shift, depth, 1 << (depth - hist_shift), MI_MAX_BINS);
    AMP_REQUIRE(hist_shift < 0 || (hist && need), "amp_mask_intensity: null argument %s with hist_shift = %d", !hist ? "hist" : "need", hist_shift);
    AMP_REQUIRE(n == 0 || (pool && off && len && image && vals), "amp_mask_intensity: null argument %s",
                !pool ? "pool" : !off ? "off" : !len ? "len" : !image ? "image" : "vals");
    AMP_TRY_STATUS(plan_pool("amp_mask_intensity", pool, off, len, n, h, w, plan));
    if (hist_shift >= 0) nbins = 1ull << (depth - hist_shift);
    return AMP_OK;
}

int mask_intensity_capacity(int n, int channels, u64 nbins, unsigned long long hist_cap, unsigned long long* need) {
    return counts_capacity("amp_mask_intensity", "hist_cap", (u64)n * (u64)channels * nbins, hist_cap, need);
}

namespace {

template <typename T>
void mi_host(const RunPlan& plan, int h, int w, const T* img, int C, int hist_shift, u64 nbins, std::vector<u64>& raw, uint32_t* hist) {
    const size_t n = plan.m.size();
    for (size_t i = 0; i < n; ++i) {
        const RunMask& mk = plan.m[i];
        MiSums acc[4] = {mi_none(), mi_none(), mi_none(), mi_none()};
        uint32_t* hi = nbins ? hist + i * (size_t)C * nbins : nullptr;
        for (int k = 0; k < mk.n; ++k) {
            const uint32_t e = plan.E[mk.ro + (size_t)k];
            for (uint32_t pos = plan.S[mk.ro + (size_t)k]; pos < e;) {                     // ends: every turn moves pos to the column's end or to e
                const uint32_t c = pos / (uint32_t)h, stop = std::min(e, (c + 1) * (uint32_t)h);
                for (uint32_t r = pos - c * (uint32_t)h; pos < stop; ++pos, ++r) {
                    const T* px = img + ((size_t)r * (size_t)w + c) * (size_t)C;
                    for (int ch = 0; ch < C; ++ch) {
                        const uint32_t v = px[ch];
                        mi_add(acc[ch], v, r, c);
                        if (hi) ++hi[(size_t)ch * nbins + (v >> hist_shift)];
                    }
                }
            }
        }
        for (int ch = 0; ch < C; ++ch) {
            u64* o = raw.data() + (i * (size_t)C + (size_t)ch) * MI_RAW;
            o[1] = acc[ch].sv; o[2] = acc[ch].svv; o[3] = acc[ch].srv; o[4] = acc[ch].scv;
            o[5] = acc[ch].mn == 0xffffffffu ? ~0ull : acc[ch].mn; o[6] = acc[ch].mx;
        }
    }
}

}  // namespace

void mask_intensity_host(const RunPlan& plan, int h, int w, const void* image, int channels, int depth, int hist_shift, u64 nbins,
                         std::vector<u64>& raw, uint32_t* hist) {
    const size_t n = plan.m.size();
    raw.assign(n * (size_t)channels * MI_RAW, 0);
    if (nbins) std::fill(hist, hist + n * (size_t)channels * nbins, 0u);
    if (depth == 8) mi_host(plan, h, w, static_cast<const uint8_t*>(image), channels, hist_shift, nbins, raw, hist);
    else mi_host(plan, h, w, static_cast<const uint16_t*>(image), channels, hist_shift, nbins, raw, hist);
}

void mask_intensity_write(const RunPlan& plan, int channels, const std::vector<u64>& raw, unsigned long long* vals) {
    const size_t n = plan.m.size();
    for (size_t i = 0; i < n; ++i)
        for (int ch = 0; ch < channels; ++ch) {
            const size_t at = (i * (size_t)channels + (size_t)ch) * MI_RAW;
            const bool any = plan.m[i].area != 0;
            vals[at] = plan.m[i].area;
            for (int k = 1; k < 7; ++k) vals[at + (size_t)k] = any ? raw[at + (size_t)k] : 0;
            vals[at + 7] = 0;
        }
}

}  // namespace amp
