// The mask analyses on run lists: what their entry points (edge_distance.hip, region_props.hip, rle_overlap.hip, seg_class_map.hip, render.hip) share
// with mask_analysis_host.hip.  Each *_check validates the arguments and builds the plan (run_list.h) that both paths evaluate; each *_host is
// the evaluation with a NULL context, byte for byte what the kernels give.  amp_label_runs, the producer of run lists from an annotation image
// (label_runs.hip, label_runs_host.hip), and amp_polygons_to_rle, the producer from polygons (polygon_runs.hip, polygon_runs_host.hip), are declared
// at the end; amp_mask_parts, the components of every mask and their repair (mask_parts.hip, mask_parts_host.hip), has its shared arithmetic and
// its declarations in mask_parts.h, included below.  Plain C++: the host-only sanitizer builds include this header.
#pragma once
#include "../../include/ampis_hip.h"
#include "run_list.h"

namespace amp {

void set_error(const char* fmt, ...);            // context.hip; the sanitizer programs bring their own

// What the argument checks of the entry points share.  api is the entry point's name, the first word of every message.
// Every mask of a pool planned (nothing when pool is NULL: the plan stays empty), or the first malformed run list refused.
inline int plan_pool(const char* api, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, RunPlan& runs) {
    const unsigned long long area = (unsigned long long)h * w;
    runs.reset(pool && n > 0 ? (size_t)n : 0);
    for (int p = 0; pool && p < n; ++p) {
        u64 covered = 0;
        const RunListFault f = plan_add_mask(runs, (size_t)p, pool + off[p], len[p], h, w, false, &covered);
        if (f == RUNS_OK) continue;
        if (f == RUNS_EMPTY) set_error("%s: mask %d has an empty run list", api, p);
        else if (f == RUNS_OVER) set_error("%s: the runs of mask %d cover more than the image's %llu pixels", api, p, area);
        else if (f == RUNS_SHORT) set_error("%s: the runs of mask %d cover %llu pixels, the image has %llu", api, p, covered, area);
        else set_error("%s: the masks of one call have more than 2^31 runs", api);
        return AMP_ERR_ARG;
    }
    return AMP_OK;
}

// the image size of the analyses that index pixels and sides in 32 bits
inline int require_image_size(const char* api, int h, int w) {
    if (h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && (unsigned long long)h * w <= (1ull << 30)) return AMP_OK;
    set_error("%s: image size %d x %d (1 .. 32768 a side, at most 2^30 pixels)", api, h, w);
    return AMP_ERR_ARG;
}

// the capacity report of a call whose need is one number: need[0] = counts, refused when the capacity cap_name = cap is smaller
inline int counts_capacity(const char* api, const char* cap_name, unsigned long long counts, unsigned long long cap, unsigned long long* need) {
    need[0] = counts;
    if (counts > cap) {
        set_error("%s: %s = %llu; %llu counts are needed", api, cap_name, cap, counts);
        return AMP_ERR_NOMEM;
    }
    return AMP_OK;
}

// amp_mask_edge_distance.  One plan for both pools: mask g of the ground truths is runs.m[g], mask q of the predictions runs.m[ng + q];
// planned are the masks the pairs name.  crop = the boxes clamped to the image, [n][4] {r1, r2, c1, c2}.
int edge_distance_check(const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                        const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, const int* box, int n,
                        int h, int w, const uint32_t* fp_d2, unsigned long long fp_cap, const unsigned long long* fp_off, const uint32_t* fn_d2,
                        unsigned long long fn_cap, const unsigned long long* fn_off, std::vector<int>& crop, RunPlan& runs);
int edge_distance_host(const RunPlan& runs, int ng, const int* pair_g, const int* pair_p, const int* crop, int n, int h, uint32_t* fp_d2,
                       unsigned long long fp_cap, unsigned long long* fp_off, uint32_t* fn_d2, unsigned long long fn_cap, unsigned long long* fn_off);

// amp_mask_region_props.  Every mask is planned; its tight box {r0, c0, r1, c1} (zeros for an empty mask) is the bbox the call returns.
int region_props_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const long long* bbox,
                       const unsigned long long* vals, RunPlan& runs);
int region_props_host(const RunPlan& runs, int h, unsigned long long* vals);

// amp_rle_overlap_groups.  A plan per pool, every mask planned, with the prefix P.
int overlap_groups_check(const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                         const unsigned long long* boff, const int* blen, const int* a_first, const int* b_first, const int* gh, const int* gw,
                         int ngroups, const uint32_t* inter, size_t inter_cap, const unsigned long long* area_a, const unsigned long long* area_b,
                         RunPlan& a, RunPlan& b);
int overlap_groups_host(const RunPlan& a, const RunPlan& b, const int* a_first, const int* b_first, int ngroups, uint32_t* inter);

// amp_seg_class_map.  A plan per pool, planned are the masks the pairs name; need = the sufficient counts capacity.
int seg_class_map_check(const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                        const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, int n, int h, int w,
                        int mode, const uint32_t* counts, unsigned long long counts_cap, const unsigned long long* counts_off,
                        const unsigned long long* pixels, RunPlan& g, RunPlan& p, unsigned long long* need);
int seg_class_map_host(const RunPlan& g, const RunPlan& p, const int* pair_g, const int* pair_p, int n, int h, int w, int mode, uint32_t* counts,
                       unsigned long long* counts_off, unsigned long long* pixels);

// amp_render_instances.  Every mask is planned (none when pool is NULL: the plan stays empty); rects = per instance the four rectangles
// {row0, row1, col0, col1} of its box outline, ends exclusive and inside the image, [n][4][4], empty without boxes.  render_host draws on img
// in place.
int render_check(const uint8_t* image, int h, int w, const uint32_t* pool, const unsigned long long* off, const int* len, int n,
                 const uint8_t* fill_tab, const uint8_t* edge_rgb, const int* boxes, const uint8_t* box_rgb, int lw, const uint8_t* out,
                 RunPlan& runs, std::vector<int>& rects);
int render_host(const RunPlan& runs, const uint8_t* fill_tab, const uint8_t* edge_rgb, const std::vector<int>& rects, const uint8_t* box_rgb,
                int n, int h, int w, uint8_t* img);

// The pixels of the word m of column col, bit 0 = image row row0, whose four neighbours are all in the mask and that lie in no border row or
// column of the h x w image (draw_binary_mask's `inner`); up / down / left / right: the mask one row above / below, one column left / right
AMP_HD u64 render_inner(u64 m, u64 up, u64 down, u64 left, u64 right, int row0, int col, int h, int w) {
    u64 inner = m & up & down & left & right;
    if (col == 0 || col == w - 1) inner = 0;
    if (row0 == 0) inner &= ~1ull;
    const long long last = (long long)h - 1 - row0;
    if (last >= 0 && last < 64) inner &= ~(1ull << last);
    return inner;
}

// amp_label_runs (label_runs_host.hip, label_runs.hip).  The check looks at the arguments only; both paths report their needs through
// label_runs_capacity before they write anything else.
int label_runs_check(const void* image, int h, int w, int kind, int connectivity, const int* ids, const int* boxes, const unsigned int* areas,
                     const uint32_t* counts, const unsigned long long* counts_off, const int* counts_len, int inst_cap,
                     const unsigned long long* need);
int label_runs_capacity(unsigned long long instances, unsigned long long counts, int inst_cap, unsigned long long counts_cap,
                        unsigned long long* need);
int label_runs_host(const void* image, int h, int w, int kind, int connectivity, int zero_is_background, int* ids, int* boxes,
                    unsigned int* areas, uint32_t* counts, unsigned long long* counts_off, int* counts_len, int inst_cap,
                    unsigned long long counts_cap, int* labels, unsigned long long* need);

// amp_polygons_to_rle (polygon_runs_host.hip, polygon_runs.hip).  The check looks at every argument and every coordinate before either path
// does anything; both paths report the counts they need through polygons_capacity before they write anything else.  The host path is the
// definition: rle_from_polygon_runs per polygon, united in order with rle_merge2_runs (rle_host.hip: the routines behind amp_rle_from_polygon and
// amp_rle_merge2, on buffers that are kept from polygon to polygon).
struct PolygonScratch {
    std::vector<int> x, y;                        // the vertices on the 5x grid, the first repeated at the end
    std::vector<unsigned long long> a, b;         // the crossings, then the run lengths
};
void rle_from_polygon_runs(const double* xy, int k, int h, int w, PolygonScratch& sc);
unsigned long long rle_merge2_runs(const uint32_t* A, int ka, const uint32_t* B, int kb, int intersect, uint32_t* out, unsigned long long cap);
int polygons_check(const double* xy, const unsigned long long* poly_off, const int* inst_first, int n, int h, int w, const uint32_t* counts,
                   const unsigned long long* counts_off, const int* counts_len, const int* boxes, const unsigned int* areas,
                   const unsigned long long* need);
int polygons_capacity(unsigned long long counts, unsigned long long counts_cap, unsigned long long* need);
int polygons_host(const double* xy, const unsigned long long* poly_off, const int* inst_first, int n, int h, int w, uint32_t* counts,
                  unsigned long long counts_cap, unsigned long long* counts_off, int* counts_len, int* boxes, unsigned int* areas,
                  unsigned long long* need);
#define AMP_POLYGON_COORD_MAX 1.0e6               // beyond it the (int) casts of the edge walk are not defined

// One edge of a polygon as the walk of rle_from_polygon_runs sees it, and step d of the walk (1 <= d <= len) in closed form: u, v of the step
// and pu, pv of the step before are functions of (edge, d) alone.  The device path evaluates exactly these expressions, in the order the host
// routine does (the build has -ffp-contract=off, divisions are IEEE).
struct PolygonEdge {
    int xs, ys, dx, dy, len;                      // the start after the swap, the extents, the number of steps
    bool flip;
    double s;                                     // the slope along the longer extent
};
AMP_HD int polygon_grid(double v) { return (int)(5.0 * v + 0.5); }
AMP_HD PolygonEdge polygon_edge(int xs, int ys, int xe, int ye) {
    PolygonEdge e;
    e.dx = xe > xs ? xe - xs : xs - xe;
    e.dy = ys > ye ? ys - ye : ye - ys;
    e.flip = (e.dx >= e.dy && xs > xe) || (e.dx < e.dy && ys > ye);
    if (e.flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    e.xs = xs; e.ys = ys;
    e.len = e.dx >= e.dy ? e.dx : e.dy;
    e.s = e.dx >= e.dy ? (e.dx ? (double)(ye - ys) / e.dx : 0.0) : (double)(xe - xs) / e.dy;
    return e;
}
AMP_HD void polygon_step(const PolygonEdge& e, int d, int* u, int* v) {
    const int t = e.flip ? e.len - d : d;
    if (e.dx >= e.dy) { *u = t + e.xs; *v = (int)(e.ys + e.s * t + 0.5); } else { *v = t + e.ys; *u = (int)(e.xs + e.s * t + 0.5); }
}
// does step d toggle the mask, and at which position x * h + y of the column-major image (at most h * w)
AMP_HD bool polygon_crossing(const PolygonEdge& e, int d, int h, int w, unsigned int* pos) {
    int u, v, pu, pv;
    polygon_step(e, d, &u, &v);
    polygon_step(e, d - 1, &pu, &pv);
    if (u == pu) return false;
    double xd = (double)(u < pu ? u : u - 1);
    xd = (xd + 0.5) / 5.0 - 0.5;
    if (!(__builtin_floor(xd) == xd && xd >= 0 && xd <= w - 1)) return false;
    double yd = (double)(v < pv ? v : pv);
    yd = (yd + 0.5) / 5.0 - 0.5;
    if (yd < 0) yd = 0; else if (yd > h) yd = h;
    yd = __builtin_ceil(yd);
    *pos = (unsigned int)((unsigned long long)xd * (unsigned long long)h + (unsigned long long)yd);
    return true;
}

// the pixel of an annotation image as both paths read it: foreground is 1 in a BINARY image, the id in a LABEL image; a pixel belongs to an
// instance unless it is 0 and 0 is background
AMP_HD int label_pixel(const void* image, int kind, size_t i) {
    return kind == 0 ? (static_cast<const uint8_t*>(image)[i] != 0 ? 1 : 0) : static_cast<const int*>(image)[i];
}
AMP_HD bool label_is_instance(int v, int kind, int zero_is_background) { return v != 0 || (kind != 0 && !zero_is_background); }

}  // namespace amp

// amp_mask_parts: mask_parts_check / mask_parts_capacity / mask_parts_host and the items both paths evaluate
#include "mask_parts.h"
