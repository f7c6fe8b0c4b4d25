// The four mask analyses on run lists: what their entry points (edge_distance.hip, region_props.hip, rle_overlap.hip, seg_class_map.hip) share
// with mask_analysis_host.hip.  Each *_check validates the arguments and builds the plan (run_list.h) that both paths evaluate; each *_host is
// the evaluation with a NULL context, byte for byte what the kernels give.  Plain C++: the host-only sanitizer builds include this header.
#pragma once
#include "run_list.h"

namespace amp {

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

}  // namespace amp
