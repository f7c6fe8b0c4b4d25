// Host side of amp_polygons_to_rle (mask_analysis.h): the argument check, the capacity report that both paths share, and the evaluation with a
// NULL context -- the definition of the call: every polygon of an instance through the routine of amp_rle_from_polygon (pycocotools rleFrPoly),
// united in order by the walk of amp_rle_merge2, what rle.merge(rle.frPyObjects(polygons, h, w)) encodes (ampis/structures.py:677,
// detectron2's polygons_to_bitmask).  One set of buffers serves every polygon of the call.  Box and area come from run_list.h's walk over the
// finished list, so they are the ones a RunMask of that list holds.  Plain C++: polygon_runs.hip computes the same bytes on the device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "mask_analysis.h"

namespace amp {

int polygons_check(const double* xy, const unsigned long long* poly_off, const int* inst_first, int n, int h, int w, const uint32_t* counts,
                   const unsigned long long* counts_off, const int* counts_len, const int* boxes, const unsigned int* areas,
                   const unsigned long long* need) {
    AMP_REQUIRE(n >= 0, "amp_polygons_to_rle: n = %d", n);
    AMP_REQUIRE(h >= 1 && w >= 1 && (unsigned long long)h * (unsigned long long)w <= (1ull << 30),
                "amp_polygons_to_rle: image size %d x %d (at least 1 a side, at most 2^30 pixels)", h, w);
    AMP_REQUIRE(need, "amp_polygons_to_rle: null argument need");
    if (n == 0) return AMP_OK;
    AMP_REQUIRE(xy && poly_off && inst_first && counts && counts_off && counts_len && boxes && areas, "amp_polygons_to_rle: null argument %s",
                !xy ? "xy" : !poly_off ? "poly_off" : !inst_first ? "inst_first" : !counts ? "counts" : !counts_off ? "counts_off" :
                !counts_len ? "counts_len" : !boxes ? "boxes" : "areas");
    AMP_REQUIRE(inst_first[0] >= 0, "amp_polygons_to_rle: inst_first[0] = %d", inst_first[0]);
    for (int i = 0; i < n; ++i)
        AMP_REQUIRE(inst_first[i + 1] > inst_first[i], "amp_polygons_to_rle: instance %d has no polygon (inst_first[%d] = %d, inst_first[%d] = %d)", i,
                    i, inst_first[i], i + 1, inst_first[i + 1]);
    unsigned long long vertices = 0;
    for (int p = inst_first[0]; p < inst_first[n]; ++p) {
        AMP_REQUIRE(poly_off[p + 1] >= poly_off[p], "amp_polygons_to_rle: poly_off[%d] = %llu is below poly_off[%d] = %llu", p + 1, poly_off[p + 1], p,
                    poly_off[p]);
        const unsigned long long len = poly_off[p + 1] - poly_off[p];
        AMP_REQUIRE(len >= 2 && len % 2 == 0 && len <= (1ull << 31), "amp_polygons_to_rle: polygon %d has %llu coordinates (x, y pairs, at least one)", p,
                    len);
        vertices += len / 2;
        AMP_REQUIRE(vertices <= (1ull << 30), "amp_polygons_to_rle: more than 2^30 vertices");
    }
    for (unsigned long long j = poly_off[inst_first[0]]; j < poly_off[inst_first[n]]; ++j)
        AMP_REQUIRE(std::isfinite(xy[j]) && std::fabs(xy[j]) <= AMP_POLYGON_COORD_MAX,
                    "amp_polygons_to_rle: coordinate xy[%llu] = %g (finite and at most 10^6 in magnitude)", j, xy[j]);
    return AMP_OK;
}

int polygons_capacity(unsigned long long counts, unsigned long long counts_cap, unsigned long long* need) {
    return counts_capacity("amp_polygons_to_rle", "counts_cap", counts, counts_cap, need);
}

int polygons_host(const double* xy, const unsigned long long* poly_off, const int* inst_first, int n, int h, int w, uint32_t* counts,
                  unsigned long long counts_cap, unsigned long long* counts_off, int* counts_len, int* boxes, unsigned int* areas,
                  unsigned long long* need) {
    PolygonScratch sc;
    std::vector<uint32_t> cur, one, tmp, out;     // the union so far, the next polygon, their union; the counts of all instances back to back
    std::vector<unsigned long long> off((size_t)n);
    for (int i = 0; i < n; ++i) {
        for (int p = inst_first[i]; p < inst_first[i + 1]; ++p) {
            rle_from_polygon_runs(xy + poly_off[p], (int)((poly_off[p + 1] - poly_off[p]) / 2), h, w, sc);
            std::vector<uint32_t>& dst = p == inst_first[i] ? cur : one;
            dst.resize(sc.b.size());
            for (size_t j = 0; j < sc.b.size(); ++j) dst[j] = (uint32_t)sc.b[j];
            if (p == inst_first[i]) continue;
            tmp.resize(cur.size() + one.size());
            const unsigned long long m = rle_merge2_runs(cur.data(), (int)cur.size(), one.data(), (int)one.size(), 0, tmp.data(), tmp.size());
            if (m > tmp.size()) {                 // cannot happen: a union has no more boundaries than its two lists together
                set_error("amp_polygons_to_rle: a union of %zu and %zu runs has %llu", cur.size(), one.size(), m);
                return AMP_ERR_ARG;
            }
            tmp.resize((size_t)m);
            cur.swap(tmp);
        }
        AMP_REQUIRE(cur.size() < (1ull << 31), "amp_polygons_to_rle: instance %d has %zu runs", i, cur.size());
        off[(size_t)i] = out.size();
        out.insert(out.end(), cur.begin(), cur.end());
    }
    AMP_TRY_STATUS(polygons_capacity(out.size(), counts_cap, need));
    RunPlan pl;
    for (int i = 0; i < n; ++i) {
        const unsigned long long end = (size_t)i + 1 < (size_t)n ? off[(size_t)i + 1] : (unsigned long long)out.size();
        counts_off[i] = off[(size_t)i];
        counts_len[i] = (int)(end - off[(size_t)i]);
        pl.reset(1);
        u64 covered = 0;
        const RunListFault f = plan_add_mask(pl, 0, out.data() + off[(size_t)i], counts_len[i], h, w, false, &covered);
        if (f != RUNS_OK) {                       // cannot happen: the routines above close every list at h * w
            set_error("amp_polygons_to_rle: the runs of instance %d cover %llu of %d x %d pixels", i, covered, h, w);
            return AMP_ERR_ARG;
        }
        const RunMask& m = pl.m[0];
        boxes[4 * i] = m.r0; boxes[4 * i + 1] = m.c0; boxes[4 * i + 2] = m.r1; boxes[4 * i + 3] = m.c1;
        areas[i] = m.area;
    }
    std::copy(out.begin(), out.end(), counts);
    return AMP_OK;
}

}  // namespace amp
