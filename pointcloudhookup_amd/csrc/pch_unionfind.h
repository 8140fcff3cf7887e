// Lock-free union-find on an int32 parent array in device memory, shared by stage C's cell union (pch_dbscan.hip)
// and the cluster merge (pch_merge.hip).
#pragma once
#include "pch_common.h"

namespace pch {
#ifdef __HIPCC__

// ---- union-find (hook larger root under smaller; lock free) ------------------------------
// Invariant: parent[x] <= x, only roots (parent[x] == x) are ever hooked, and only by a CAS, so
// every value ever stored in parent[x] is an ancestor of x.  Loads bypass the (incoherent) L1;
// path compression is a PLAIN store of an ancestor - racing writers all write ancestors, and a
// stale read merely costs an extra hop or a failed CAS, whose return value is the truth.
// When all unions are done the root of a set is its smallest member.
__device__ __forceinline__ int uf_load(int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int* __restrict__ parent, int x) {
    int p = uf_load(&parent[x]);
    while (p != x) {
        const int gp = uf_load(&parent[p]);
        if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}
// a, b: any members (ideally already roots) of the two sets
__device__ __forceinline__ void uf_union(int* __restrict__ parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }   // a > b: hook a under b
        const int old = atomicCAS(&parent[a], a, b);
        if (old == a) return;
        a = old;                                          // somebody hooked a first: follow it
    }
}

#endif  // __HIPCC__
}  // namespace pch
