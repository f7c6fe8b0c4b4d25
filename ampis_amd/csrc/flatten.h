// amp_flatten_instances: what the host evaluation (flatten_host.hip) and the device kernels (flatten.hip) share.  Plain C++ that also compiles
// under g++ (the host-only sanitizer build), integers throughout.
//
// The OWNER of a pixel is, among the instances whose mask covers it, the one with the smallest (rank, index); a pixel nothing covers has no
// owner.  The argument check builds the plan of run_list.h for every mask and the PRIORITY ORDER: order[p] = the instance at place p when the
// instances are sorted by (rank, index), so "the first instance in order that covers the pixel" is the owner on both paths.
#pragma once
#include <algorithm>

#include "run_list.h"

namespace amp {

// order[p] for p = 0 .. n - 1; rank == NULL: index order
inline void flatten_order(const uint32_t* rank, int n, std::vector<int>& order) {
    order.resize((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    if (rank) std::stable_sort(order.begin(), order.end(), [rank](int a, int b) { return rank[a] < rank[b]; });
}

// flatten_host.hip: the check builds the plan and the order; both paths report the counts they need through flatten_capacity before they
// write anything else
int flatten_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const uint32_t* rank,
                  const uint32_t* counts, unsigned long long counts_cap, const unsigned long long* counts_off, const int* counts_len,
                  const unsigned long long* stats, const int* boxes, const unsigned long long* pixels, const unsigned long long* need,
                  RunPlan& runs, std::vector<int>& order);
int flatten_capacity(unsigned long long counts, unsigned long long counts_cap, unsigned long long* need);
int flatten_host(const RunPlan& runs, const std::vector<int>& order, int h, int w, int* labels, uint32_t* counts, unsigned long long counts_cap,
                 unsigned long long* counts_off, int* counts_len, unsigned long long* stats, int* boxes, unsigned long long* pixels,
                 unsigned long long* need);

}  // namespace amp
