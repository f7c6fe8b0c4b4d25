// The lock-free union-find over the indices of an array of runs that label_runs.hip (the components of an annotation image) and mask_parts.hip
// (the parts and holes of every mask of a pool) share.  parent[i] = i at the start; the only write is the compare-and-swap that hooks the
// larger of two roots under the smaller, so parent[y] <= y always, a root is the smallest index of its set, and the partition -- with it
// every root -- does not depend on the order of the unions.  Device code only.
#pragma once

namespace amp {

// the root of x as far as this lane can see.  Ends: parent[y] <= y always, and the walk goes on only while parent[y] < y.  COHERENT: while
// other lanes still unite (loads that pass the CU's L1); without it for a launch that writes no parent.
template <bool COHERENT>
__device__ __forceinline__ unsigned int uf_find(unsigned int* parent, unsigned int x) {
    for (;;) {
        const unsigned int p = COHERENT ? __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : parent[x];
        if (p == x) return x;
        x = p;
    }
}

// Unites the sets of runs a and b.  A parent only ever changes from itself to a smaller index (the compare-and-swap below is the only write),
// so a stale read is an ancestor the set once had and the swap on a node that is no longer a root fails.  Ends: a failed swap returns the
// node's parent, smaller than the node, so a + b falls with every round; no round waits for another lane.
__device__ __forceinline__ void uf_unite(unsigned int* parent, unsigned int a, unsigned int b) {
    for (;;) {
        a = uf_find<true>(parent, a);
        b = uf_find<true>(parent, b);
        if (a == b) return;
        if (a < b) { const unsigned int t = a; a = b; b = t; }
        const unsigned int old = atomicCAS(&parent[a], a, b);
        if (old == a) return;
        a = old;
    }
}

}  // namespace amp
