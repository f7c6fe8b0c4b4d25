// Host side of the mask analyses on COCO run lists -- mask_edge_distance, region properties, group overlap, segmentation class map, overlays
// (mask_analysis.h): the argument checks, which build the plan (run_list.h: plan_add_mask, the one walk over a run list) that the device path
// and the host path both evaluate, and the host evaluations, what each call runs with a NULL context.  Plain C++ throughout: the host-only
// sanitizer builds of tests/sanitize compile this file with g++.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"
#include "region_props.h"
#include "seg_class_map.h"

// ---- mask_edge_distance (ampis/analyze.py:416-499): the argument checks and the host evaluation ------------------
// For each (ground truth, prediction) pair and its crop [r1:r2, c1:c2]: the squared distance from every false-positive pixel (pred & ~gt) to the
// nearest gt pixel of the crop, and from every false-negative pixel (gt & ~pred) to the nearest pred pixel, queries in row-major order.
// The reference forms a dense [queries x targets x 2] double tensor per pair; here a column pass stores each pixel's distance to the nearest
// target of its own column, and a query walks the columns outward until the column offset alone is no better than what it has: exact
// (integers throughout), memory linear in the crop.
namespace amp {

int edge_distance_check(const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                        const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, const int* box, int n,
                        int h, int w, const uint32_t* fp_d2, unsigned long long fp_cap, const unsigned long long* fp_off, const uint32_t* fn_d2,
                        unsigned long long fn_cap, const unsigned long long* fn_off, std::vector<int>& crop, RunPlan& runs) {
    AMP_REQUIRE(n >= 0 && ng >= 0 && np >= 0 && fp_off && fn_off && (fp_d2 || fp_cap == 0) && (fn_d2 || fn_cap == 0),
                "amp_mask_edge_distance: bad argument");
    AMP_REQUIRE(n == 0 || (gpool && goff && glen && ppool && poff && plen && pair_g && pair_p && box), "amp_mask_edge_distance: null argument");
    AMP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768,
                "amp_mask_edge_distance: image size %d x %d (1 .. 32768 a side: squared distances are 32-bit)", h, w);
    const unsigned long long area = (unsigned long long)h * w;
    runs.reset((size_t)ng + (size_t)np);                                         // a run list named by many pairs is walked once
    crop.assign((size_t)n * 4, 0);
    for (int p = 0; p < n; ++p) {
        const int g = pair_g[p], q = pair_p[p];
        AMP_REQUIRE(g >= 0 && g < ng && q >= 0 && q < np, "amp_mask_edge_distance: pair %d = (%d, %d) outside %d x %d masks", p, g, q, ng, np);
        for (int side = 0; side < 2; ++side) {
            const size_t idx = side ? (size_t)ng + q : (size_t)g;
            if (runs.m[idx].n >= 0) continue;
            const char* which = side ? "prediction" : "ground-truth";
            u64 covered = 0;
            const RunListFault f = side ? plan_add_mask(runs, idx, ppool + poff[q], plen[q], h, w, false, &covered)
                                        : plan_add_mask(runs, idx, gpool + goff[g], glen[g], h, w, false, &covered);
            AMP_REQUIRE(f != RUNS_EMPTY, "amp_mask_edge_distance: pair %d names an empty %s run list", p, which);
            AMP_REQUIRE(f != RUNS_OVER, "amp_mask_edge_distance: the %s runs of pair %d cover more than the image's %llu pixels", which, p, area);
            AMP_REQUIRE(f != RUNS_SHORT, "amp_mask_edge_distance: the %s runs of pair %d cover %llu pixels, the image has %llu", which, p, covered, area);
            AMP_REQUIRE(f == RUNS_OK, "amp_mask_edge_distance: the masks of the pairs have more than 2^31 runs");
        }
        const int* b = box + 4 * (size_t)p;
        AMP_REQUIRE(b[0] >= 0 && b[2] >= 0 && b[0] <= b[1] && b[2] <= b[3], "amp_mask_edge_distance: box [%d, %d, %d, %d] of pair %d", b[0], b[1], b[2], b[3], p);
        int* c = &crop[4 * (size_t)p];                                            // numpy's slice: an end beyond the image is the image's end
        c[0] = std::min(b[0], h); c[1] = std::min(b[1], h); c[2] = std::min(b[2], w); c[3] = std::min(b[3], w);
    }
    return AMP_OK;
}

// bytes of the crop, row-major, of a planned mask
static void edge_decode_crop(const RunPlan& runs, const RunMask& mk, int h, const int* cr, std::vector<unsigned char>& out) {
    const int H = cr[1] - cr[0], W = cr[3] - cr[2];
    out.assign((size_t)H * W, 0);
    if (H == 0 || W == 0) return;
    const unsigned long long stop = (unsigned long long)cr[3] * h;               // nothing of the crop lies behind its last column
    for (int k = 0; k < mk.n && runs.S[mk.ro + k] < stop; ++k) {
        const unsigned long long s = runs.S[mk.ro + k], e = runs.E[mk.ro + k];
        const long long first = (long long)(s / (unsigned)h), last = (long long)((e - 1) / (unsigned)h);
        for (long long col = std::max<long long>(first, cr[2]); col <= std::min<long long>(last, cr[3] - 1); ++col) {
            const unsigned long long cb = (unsigned long long)col * h;
            const int ya = std::max((int)(std::max(s, cb) - cb), cr[0]), yb = std::min((int)(std::min(e, cb + h) - cb), cr[1]);
            for (int y = ya; y < yb; ++y) out[(size_t)(y - cr[0]) * W + (size_t)(col - cr[2])] = 1;
        }
    }
}

// squared distance of every pixel of q & ~t to the nearest pixel of t, appended in row-major order
static void edge_nearest(const std::vector<unsigned char>& q, const std::vector<unsigned char>& t, int H, int W, std::vector<int>& colv,
                         std::vector<uint32_t>& out) {
    const int NONE = 1 << 20;
    bool any = false;
    for (size_t i = 0; i < q.size() && !any; ++i) any = q[i] && !t[i];
    if (!any) return;
    colv.assign((size_t)H * W, NONE);                                            // distance to the nearest target of the pixel's own column
    for (int c = 0; c < W; ++c) {
        int d = NONE;
        for (int r = 0; r < H; ++r) { d = t[(size_t)r * W + c] ? 0 : std::min(d + 1, NONE); colv[(size_t)r * W + c] = d; }
        d = NONE;
        for (int r = H - 1; r >= 0; --r) { d = t[(size_t)r * W + c] ? 0 : std::min(d + 1, NONE); int& v = colv[(size_t)r * W + c]; v = std::min(v, d); }
    }
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            if (!q[(size_t)r * W + c] || t[(size_t)r * W + c]) continue;
            uint32_t best = 0xffffffffu;
            const int* row = &colv[(size_t)r * W];
            for (int dc = 0; (uint32_t)dc * (uint32_t)dc < best && (c - dc >= 0 || c + dc < W); ++dc) {
                const uint32_t d2c = (uint32_t)dc * (uint32_t)dc;
                if (c - dc >= 0 && row[c - dc] != NONE) best = std::min(best, (uint32_t)row[c - dc] * (uint32_t)row[c - dc] + d2c);
                if (c + dc < W && row[c + dc] != NONE) best = std::min(best, (uint32_t)row[c + dc] * (uint32_t)row[c + dc] + d2c);
            }
            out.push_back(best);
        }
}

int edge_distance_host(const RunPlan& runs, int ng, const int* pair_g, const int* pair_p, const int* crop, int n, int h, uint32_t* fp_d2,
                       unsigned long long fp_cap, unsigned long long* fp_off, uint32_t* fn_d2, unsigned long long fn_cap, unsigned long long* fn_off) {
    std::vector<uint32_t> fp, fn;                                                // results are handed over whole or not at all
    std::vector<unsigned long long> fpo((size_t)n + 1, 0), fno((size_t)n + 1, 0);
    std::vector<unsigned char> gm, pm;
    std::vector<int> colv;
    for (int p = 0; p < n; ++p) {
        const int* cr = crop + 4 * (size_t)p;
        const int H = cr[1] - cr[0], W = cr[3] - cr[2];
        if (H > 0 && W > 0) {
            edge_decode_crop(runs, runs.m[(size_t)pair_g[p]], h, cr, gm);
            edge_decode_crop(runs, runs.m[(size_t)ng + pair_p[p]], h, cr, pm);
            edge_nearest(pm, gm, H, W, colv, fp);
            edge_nearest(gm, pm, H, W, colv, fn);
        }
        fpo[(size_t)p + 1] = fp.size();
        fno[(size_t)p + 1] = fn.size();
    }
    if (fp.size() > fp_cap || fn.size() > fn_cap) {
        set_error("amp_mask_edge_distance: %zu false-positive and %zu false-negative pixels, capacities %llu and %llu", fp.size(), fn.size(), fp_cap, fn_cap);
        return AMP_ERR_NOMEM;
    }
    std::copy(fp.begin(), fp.end(), fp_d2);
    std::copy(fn.begin(), fn.end(), fn_d2);
    std::copy(fpo.begin(), fpo.end(), fp_off);
    std::copy(fno.begin(), fno.end(), fn_off);
    return AMP_OK;
}

}  // namespace amp

// ---- region properties (ampis/structures.py:474-514, skimage.measure.regionprops restated): the argument checks, whose plan
// holds the tight boxes, and the host evaluation.  Per mask 13 exact integers {N, sum r, sum c, sum r^2, sum r c, sum c^2, P1, P2, P3, convex area, 0, 0, 0}:
// the moments in closed form from the runs, the perimeter classes and the hull on a column-major bit plane of the tight box (region_props.h:
// the same word arithmetic as the kernels of region_props.hip).
namespace amp {

int region_props_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const long long* bbox,
                       const unsigned long long* vals, RunPlan& runs) {
    AMP_REQUIRE(n >= 0, "amp_mask_region_props: n = %d", n);
    AMP_REQUIRE(n == 0 || (pool && off && len && bbox && vals), "amp_mask_region_props: null argument");
    AMP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && (unsigned long long)h * w <= (1ull << 30),
                "amp_mask_region_props: image size %d x %d (1 .. 32768 a side, at most 2^30 pixels: the moment sums are 64-bit)", h, w);
    AMP_TRY_STATUS(plan_pool("amp_mask_region_props", pool, off, len, n, h, w, runs));
    return AMP_OK;
}

int region_props_host(const RunPlan& runs, int h, unsigned long long* vals) {
    std::vector<u64> mask, border;
    std::vector<int> pts;
    for (size_t p = 0; p < runs.m.size(); ++p) {
        unsigned long long* v = vals + 13 * p;
        std::fill(v, v + 13, 0ull);
        const RunMask& mk = runs.m[p];
        const int H = mk.r1 - mk.r0, W = mk.c1 - mk.c0, pitch = (H + 63) >> 6;
        if (H == 0) continue;
        mask.assign((size_t)W * pitch, 0ull);
        border.assign((size_t)W * pitch, 0ull);
        for (int k = 0; k < mk.n; ++k) {                                          // inside the tight box by construction
            const unsigned int s = runs.S[mk.ro + k], e = runs.E[mk.ro + k];
            rp_run_sums(s, e, (u64)h, v);
            paint_run<false>(s, e, h, mask.data(), mk.r0, mk.c0, H, W, pitch, OrPlain());
        }
        for (int q = 0; q < W; ++q)
            for (int wv = 0; wv < pitch; ++wv) border[(size_t)q * pitch + wv] = rp_border_at(mask.data(), W, pitch, q, wv);
        for (int q = 0; q < W; ++q)
            for (int wv = 0; wv < pitch; ++wv) {
                if (!border[(size_t)q * pitch + wv]) continue;
                u64 cls[3];
                rp_classify_at(border.data(), W, pitch, q, wv, cls);
                for (int k = 0; k < 3; ++k) v[6 + k] += (unsigned)popc(cls[k]);
            }
        const int np = 2 * W + 1;
        pts.assign((size_t)4 * np, 0);
        int *lo = pts.data(), *hi = lo + np, *sl = hi + np, *su = sl + np;
        for (int i = 0; i < np; ++i) rp_point(i, W, mask.data(), pitch, &lo[i], &hi[i]);
        const int kl = rp_chain(lo, np, +1, sl), ku = rp_chain(hi, np, -1, su);
        long long fill = W;                                                      // sum over the columns of floor(upper / 2) - ceil(lower / 2) + 1
        for (int k = 0; k + 1 < ku; ++k) fill += rp_edge_sum(su[k], hi[su[k]], su[k + 1], hi[su[k + 1]], true);
        for (int k = 0; k + 1 < kl; ++k) fill -= rp_edge_sum(sl[k], lo[sl[k]], sl[k + 1], lo[sl[k + 1]], false);
        v[9] = (unsigned long long)fill;
    }
    return AMP_OK;
}

}  // namespace amp

// ---- all-pairs mask intersection inside groups (ampis/applications/powder.py:80-83, RLE.merge(intersect=True) + RLE.area for every satellite
// against every particle of an image): argument checks that also build the plan (run_list.h), shared with the device path, and the host
// evaluation: the box test, then one walk over both lists of runs for the pairs it leaves.
namespace amp {

static int overlap_plan_pool(const char* which, const uint32_t* pool, const unsigned long long* off, const int* len, const int* first,
                             const int* gh, const int* gw, int ngroups, RunPlan& pl) {
    pl.reset((size_t)first[ngroups]);
    for (int g = 0; g < ngroups; ++g) {
        const unsigned long long area = (unsigned long long)gh[g] * gw[g];
        for (int p = first[g]; p < first[g + 1]; ++p) {
            u64 covered = 0;
            const RunListFault f = plan_add_mask(pl, (size_t)p, pool + off[p], len[p], gh[g], gw[g], true, &covered);
            AMP_REQUIRE(f != RUNS_EMPTY, "amp_rle_overlap_groups: mask %d of pool %s (group %d) has an empty run list", p, which, g);
            AMP_REQUIRE(f != RUNS_OVER, "amp_rle_overlap_groups: the runs of mask %d of pool %s (group %d) cover more than the image's %llu pixels",
                        p, which, g, area);
            AMP_REQUIRE(f != RUNS_SHORT, "amp_rle_overlap_groups: the runs of mask %d of pool %s (group %d) cover %llu pixels, the image has %llu",
                        p, which, g, covered, area);
            AMP_REQUIRE(f == RUNS_OK, "amp_rle_overlap_groups: the masks of pool %s have more than 2^31 runs", which);
        }
    }
    return AMP_OK;
}

int overlap_groups_check(const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                         const unsigned long long* boff, const int* blen, const int* a_first, const int* b_first, const int* gh, const int* gw,
                         int ngroups, const uint32_t* inter, size_t inter_cap, const unsigned long long* area_a, const unsigned long long* area_b,
                         RunPlan& a, RunPlan& b) {
    AMP_REQUIRE(ngroups >= 0, "amp_rle_overlap_groups: ngroups = %d", ngroups);
    if (ngroups == 0) return AMP_OK;
    AMP_REQUIRE(a_first && b_first && gh && gw, "amp_rle_overlap_groups: null argument");
    AMP_REQUIRE(a_first[0] == 0 && b_first[0] == 0, "amp_rle_overlap_groups: a_first[0] = %d, b_first[0] = %d (group 0 starts at mask 0)",
                a_first[0], b_first[0]);
    unsigned long long total = 0;
    for (int g = 0; g < ngroups; ++g) {
        AMP_REQUIRE(a_first[g + 1] >= a_first[g], "amp_rle_overlap_groups: a_first[%d] = %d is below a_first[%d] = %d", g + 1, a_first[g + 1], g,
                    a_first[g]);
        AMP_REQUIRE(b_first[g + 1] >= b_first[g], "amp_rle_overlap_groups: b_first[%d] = %d is below b_first[%d] = %d", g + 1, b_first[g + 1], g,
                    b_first[g]);
        AMP_REQUIRE(gh[g] >= 1 && gw[g] >= 1 && gh[g] <= 32768 && gw[g] <= 32768 && (unsigned long long)gh[g] * gw[g] <= (1ull << 30),
                    "amp_rle_overlap_groups: image size %d x %d of group %d (1 .. 32768 a side, at most 2^30 pixels)", gh[g], gw[g], g);
        total += (unsigned long long)(a_first[g + 1] - a_first[g]) * (unsigned long long)(b_first[g + 1] - b_first[g]);
    }
    const int na = a_first[ngroups], nb = b_first[ngroups];
    AMP_REQUIRE((na == 0 || (apool && aoff && alen && area_a)) && (nb == 0 || (bpool && boff && blen && area_b)) && (total == 0 || inter),
                "amp_rle_overlap_groups: null argument");
    AMP_REQUIRE(total <= inter_cap, "amp_rle_overlap_groups: inter_cap = %zu, the groups have %llu pairs", inter_cap, total);
    AMP_TRY_STATUS(overlap_plan_pool("A", apool, aoff, alen, a_first, gh, gw, ngroups, a));
    AMP_TRY_STATUS(overlap_plan_pool("B", bpool, boff, blen, b_first, gh, gw, ngroups, b));
    return AMP_OK;
}

int overlap_groups_host(const RunPlan& a, const RunPlan& b, const int* a_first, const int* b_first, int ngroups, uint32_t* inter) {
    size_t out = 0;
    for (int g = 0; g < ngroups; ++g)
        for (int i = a_first[g]; i < a_first[g + 1]; ++i) {
            const RunMask& A = a.m[(size_t)i];
            for (int j = b_first[g]; j < b_first[g + 1]; ++j, ++out) {
                const RunMask& B = b.m[(size_t)j];
                uint32_t sum = 0;
                if (A.n && B.n && A.r0 < B.r1 && B.r0 < A.r1 && A.c0 < B.c1 && B.c0 < A.c1) {
                    const uint32_t *as = &a.S[A.ro], *ae = &a.E[A.ro], *bs = &b.S[B.ro], *be = &b.E[B.ro];
                    for (int p = 0, q = 0; p < A.n && q < B.n;) {
                        const uint32_t lo = std::max(as[p], bs[q]), hi = std::min(ae[p], be[q]);
                        if (hi > lo) sum += hi - lo;
                        if (ae[p] <= be[q]) ++p; else ++q;
                    }
                }
                inter[out] = sum;
            }
        }
    return AMP_OK;
}

}  // namespace amp

// ---- segmentation class map (ampis/analyze.py:589-699, seg_perf_iset): argument checks that also build the plan (run_list.h, entries for
// the masks the pairs name), shared with the device path, and the host evaluation.  TP = OR over the pairs of g & q, FN of g & ~q, FP of
// ~g & q as three column-major bit planes of the image (64 rows a word), painted from the runs of every pair by one walk over both lists; the
// classes of the mode and their run lists then come from the plane words (seg_class_map.h: the same word arithmetic as the kernels of
// seg_class_map.hip).  Memory: three planes of h * w bits and the result, whatever the number of pairs.
namespace amp {

static int seg_plan_mask(const char* which, int pair, int idx, const uint32_t* c, int len, int h, int w, RunPlan& pl, unsigned long long& bounds) {
    const unsigned long long area = (unsigned long long)h * w;
    u64 covered = 0;
    const RunListFault f = plan_add_mask(pl, (size_t)idx, c, len, h, w, false, &covered);
    AMP_REQUIRE(f != RUNS_EMPTY, "amp_seg_class_map: pair %d names %s mask %d, which has an empty run list", pair, which, idx);
    AMP_REQUIRE(f != RUNS_OVER, "amp_seg_class_map: the runs of %s mask %d (pair %d) cover more than the image's %llu pixels", which, idx, pair, area);
    AMP_REQUIRE(f != RUNS_SHORT, "amp_seg_class_map: the runs of %s mask %d (pair %d) cover %llu pixels, the image has %llu", which, idx, pair, covered, area);
    AMP_REQUIRE(f == RUNS_OK, "amp_seg_class_map: the %s masks of the pairs have more than 2^31 runs", which);
    bounds += (unsigned long long)(len - 1);
    return AMP_OK;
}

int seg_class_map_check(const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                        const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, int n, int h, int w,
                        int mode, const uint32_t* counts, unsigned long long counts_cap, const unsigned long long* counts_off,
                        const unsigned long long* pixels, RunPlan& g, RunPlan& p, unsigned long long* need) {
    AMP_REQUIRE(n >= 0 && ng >= 0 && np >= 0, "amp_seg_class_map: n = %d, ng = %d, np = %d", n, ng, np);
    AMP_REQUIRE(mode == 0 || mode == 1, "amp_seg_class_map: mode = %d (0 reduced, 1 all)", mode);
    AMP_REQUIRE(counts && counts_off && pixels, "amp_seg_class_map: null argument");
    AMP_REQUIRE(n == 0 || (gpool && goff && glen && ppool && poff && plen && pair_g && pair_p), "amp_seg_class_map: null argument");
    AMP_TRY_STATUS(require_image_size("amp_seg_class_map", h, w));
    g.reset((size_t)ng);
    p.reset((size_t)np);
    unsigned long long bounds = 0;                                               // every boundary of a class is a boundary of a named run list
    for (int i = 0; i < n; ++i) {
        const int a = pair_g[i], b = pair_p[i];
        AMP_REQUIRE(a >= 0 && a < ng && b >= 0 && b < np, "amp_seg_class_map: pair %d = (%d, %d) outside %d x %d masks", i, a, b, ng, np);
        if (g.m[(size_t)a].n < 0) AMP_TRY_STATUS(seg_plan_mask("ground-truth", i, a, gpool + goff[a], glen[a], h, w, g, bounds));
        if (p.m[(size_t)b].n < 0) AMP_TRY_STATUS(seg_plan_mask("predicted", i, b, ppool + poff[b], plen[b], h, w, p, bounds));
    }
    *need = (unsigned long long)sc_classes(mode) * (bounds + 1);
    if (counts_cap < *need) {
        set_error("amp_seg_class_map: counts_cap = %llu, %llu are needed (classes x (1 + the run boundaries of the masks the pairs name))",
                  counts_cap, *need);
        return AMP_ERR_NOMEM;
    }
    return AMP_OK;
}

// every run of A cut by the runs of B: the parts inside B into `in` (or nowhere), the parts outside into `out`
static void sc_split(const RunPlan& pa, const RunMask& A, const RunPlan& pb, const RunMask& B, u64* in, u64* out, int h, int pitch) {
    const uint32_t *as = &pa.S[A.ro], *ae = &pa.E[A.ro], *bs = &pb.S[B.ro], *be = &pb.E[B.ro];
    auto paint = [&](u64* plane, unsigned int s, unsigned int e) { paint_run<false>(s, e, h, plane, 0, 0, h, 0, pitch, OrPlain()); };      // the full image; no clip, W is not read
    int k = 0;
    for (int i = 0; i < A.n; ++i) {
        unsigned int pos = as[i];
        const unsigned int e = ae[i];
        while (k < B.n && be[k] <= pos) ++k;
        while (pos < e) {
            if (k < B.n && bs[k] < e) {
                const unsigned int lo = std::max(bs[k], pos), hi = std::min(be[k], e);
                if (lo > pos) paint(out, pos, lo);
                if (in) paint(in, lo, hi);
                pos = hi;
                if (be[k] <= e) ++k;
            } else {
                paint(out, pos, e);
                pos = e;
            }
        }
    }
}

int seg_class_map_host(const RunPlan& g, const RunPlan& p, const int* pair_g, const int* pair_p, int n, int h, int w, int mode, uint32_t* counts,
                       unsigned long long* counts_off, unsigned long long* pixels) {
    const int pitch = (h + 63) >> 6, K = sc_classes(mode);
    const size_t units = (size_t)w * pitch;
    std::vector<u64> planes(3 * units, 0ull);
    u64 *TP = planes.data(), *FN = TP + units, *FP = FN + units;
    for (int i = 0; i < n; ++i) {
        const RunMask& G = g.m[(size_t)pair_g[i]];
        const RunMask& Q = p.m[(size_t)pair_p[i]];
        sc_split(g, G, p, Q, TP, FN, h, pitch);
        sc_split(p, Q, g, G, nullptr, FP, h, pitch);
    }
    std::vector<uint32_t> bnd[7];
    unsigned long long px[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int col = 0; col < w; ++col)
        for (int wv = 0; wv < pitch; ++wv) {
            const size_t u = (size_t)col * pitch + wv;
            const u64 valid = sc_valid(h, wv), tp = TP[u], fn = FN[u], fp = FP[u];
            for (int c = 0; c < 8; ++c) px[c] += (unsigned)popc(sc_code_word(tp, fn, fp, c) & valid);
            const int pb = sc_prev_bit(h, wv);
            const u64 qt = u ? TP[u - 1] >> pb : 0ull, qf = u ? FN[u - 1] >> pb : 0ull, qp = u ? FP[u - 1] >> pb : 0ull;
            const uint32_t base = (uint32_t)col * (uint32_t)h + ((uint32_t)wv << 6);
            for (int k = 0; k < K; ++k) {
                u64 t = sc_transitions(sc_class_word(tp, fn, fp, mode, k) & valid, sc_class_word(qt & 1ull, qf & 1ull, qp & 1ull, mode, k), valid);
                for (; t; t &= t - 1) bnd[k].push_back(base + (uint32_t)ctz(t));
            }
        }
    unsigned long long o = 0;
    const uint32_t area = (uint32_t)((unsigned long long)h * w);
    for (int k = 0; k < K; ++k) {
        counts_off[k] = o;
        uint32_t prev = 0;
        for (uint32_t b : bnd[k]) { counts[o++] = b - prev; prev = b; }
        counts[o++] = area - prev;
    }
    counts_off[K] = o;
    std::copy(px, px + 8, pixels);
    return AMP_OK;
}

}  // namespace amp


// ---- instance overlays (ampis_amd/utils/visualizer.py: draw_binary_mask + draw_box per instance, in draw order): the argument checks, which
// build the plan and the outline rectangles, and the host drawing: per instance one walk over its runs into a bit plane of its tight box, the
// edge rule on the plane's words (render_inner, shared with render.hip), then the table lookups and the four rectangles on the pixels.
namespace amp {

int render_check(const uint8_t* image, int h, int w, const uint32_t* pool, const unsigned long long* off, const int* len, int n,
                 const uint8_t* fill_tab, const uint8_t* edge_rgb, const int* boxes, const uint8_t* box_rgb, int lw, const uint8_t* out,
                 RunPlan& runs, std::vector<int>& rects) {
    (void)edge_rgb;
    AMP_REQUIRE(image && out, "amp_render_instances: null image");
    AMP_REQUIRE(n >= 0, "amp_render_instances: n = %d", n);
    AMP_REQUIRE(lw >= 1, "amp_render_instances: lw = %d (at least 1)", lw);
    AMP_REQUIRE(h >= 1 && w >= 1 && (unsigned long long)h * w <= (1ull << 30), "amp_render_instances: image size %d x %d (at most 2^30 pixels)", h, w);
    AMP_REQUIRE(n == 0 || !pool || (off && len && fill_tab), "amp_render_instances: null argument (off, len and fill_tab go with pool)");
    AMP_REQUIRE(n == 0 || !boxes || box_rgb, "amp_render_instances: null argument (box_rgb goes with boxes)");
    AMP_TRY_STATUS(plan_pool("amp_render_instances", pool, off, len, n, h, w, runs));
    rects.assign(boxes ? (size_t)n * 16 : 0, 0);
    for (int p = 0; boxes && p < n; ++p) {
        const int x0 = boxes[4 * (size_t)p], y0 = boxes[4 * (size_t)p + 1], x1 = boxes[4 * (size_t)p + 2], y1 = boxes[4 * (size_t)p + 3];
        AMP_REQUIRE(x0 >= 0 && x0 < w && x1 >= 0 && x1 < w && y0 >= 0 && y0 < h && y1 >= 0 && y1 < h,
                    "amp_render_instances: box %d = (%d, %d, %d, %d) outside the %d x %d image", p, x0, y0, x1, y1, h, w);
        const int ya = (int)std::min<long long>((long long)y0 + lw, h), yb = (int)std::max<long long>((long long)y1 - lw + 1, 0);
        const int xa = (int)std::min<long long>((long long)x0 + lw, w), xb = (int)std::max<long long>((long long)x1 - lw + 1, 0);
        const int r[16] = {y0, ya, x0, x1 + 1, yb, y1 + 1, x0, x1 + 1, y0, y1 + 1, x0, xa, y0, y1 + 1, xb, x1 + 1};
        std::copy(r, r + 16, &rects[16 * (size_t)p]);
    }
    return AMP_OK;
}

int render_host(const RunPlan& runs, const uint8_t* fill_tab, const uint8_t* edge_rgb, const std::vector<int>& rects, const uint8_t* box_rgb,
                int n, int h, int w, uint8_t* img) {
    std::vector<u64> mask;
    for (int i = 0; i < n; ++i) {
        if (!runs.m.empty() && runs.m[(size_t)i].n > 0) {
            const RunMask& mk = runs.m[(size_t)i];
            const int H = mk.r1 - mk.r0, W = mk.c1 - mk.c0, pitch = (H + 63) >> 6;
            mask.assign((size_t)W * pitch, 0ull);
            for (int k = 0; k < mk.n; ++k)                                        // inside the tight box by construction
                paint_run<false>(runs.S[mk.ro + k], runs.E[mk.ro + k], h, mask.data(), mk.r0, mk.c0, H, W, pitch, OrPlain());
            const uint8_t* tab = fill_tab + 768 * (size_t)i;
            for (int q = 0; q < W; ++q)
                for (int wv = 0; wv < pitch; ++wv) {
                    const u64* at = &mask[(size_t)q * pitch + wv];
                    const u64 m = *at;
                    if (!m) continue;
                    const int row0 = mk.r0 + (wv << 6), col = mk.c0 + q;
                    u64 edge = 0;
                    if (edge_rgb) {                                               // beyond the tight box the mask is empty
                        const u64 up = (m << 1) | (wv > 0 ? at[-1] >> 63 : 0ull), down = (m >> 1) | (wv + 1 < pitch ? at[1] << 63 : 0ull);
                        edge = m & ~render_inner(m, up, down, q > 0 ? at[-pitch] : 0ull, q + 1 < W ? at[pitch] : 0ull, row0, col, h, w);
                    }
                    for (u64 x = m; x; x &= x - 1) {
                        const int b = ctz(x);
                        uint8_t* px = img + ((size_t)(row0 + b) * w + col) * 3;
                        for (int c = 0; c < 3; ++c) px[c] = (edge >> b) & 1 ? edge_rgb[3 * (size_t)i + c] : tab[3 * px[c] + c];
                    }
                }
        }
        for (int q = 0; q < 4 && !rects.empty(); ++q) {
            const int* r = &rects[16 * (size_t)i + 4 * q];
            for (int y = r[0]; y < r[1]; ++y)
                for (int x = r[2]; x < r[3]; ++x) memcpy(img + ((size_t)y * w + x) * 3, box_rgb + 3 * (size_t)i, 3);
        }
    }
    return AMP_OK;
}

}  // namespace amp
