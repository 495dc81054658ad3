// kpx_unionfind.h -- lock-free union-find over int32 parents in device memory (parent[i] = i to start): the connected components of
// DBSCAN's core points (kpx_cluster.hip) and of a mesh's triangles (kpx_mesh.hip).  The larger root is hooked under the smaller, so
// the root of a set is its smallest member whatever the order in which the atomics land.
#pragma once
#include "kpx_common.h"

namespace kpx {

constexpr int kUniteBound = 1 << 20;       // failed hooks of one pair before the pass gives up (each failure is another thread's progress)

__device__ __forceinline__ int32_t parent_load(const int32_t *p, int32_t x)
{
    // another CU may have rewritten the word since this CU's L1 saw it: read it from L2 (a stale value is still an ancestor)
    return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x with path halving.  Every parent value is smaller than its index and stays inside x's set (hooks and halving only
// point a node at an ancestor), so the walk strictly descends and ends.
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x)
{
    int32_t p = parent_load(parent, x);
    while (p != x) {
        const int32_t gp = parent_load(parent, p);
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
        p = parent_load(parent, x);
    }
    return x;
}

// ECL-CC style hooking: CAS the larger root under the smaller one.  ra: an ancestor of the querying point (its root as last seen;
// refreshed here), so that its walk starts next to the root.  Returns false after kUniteBound failed CAS.
__device__ __forceinline__ bool uf_unite(int32_t *parent, int32_t &ra_seen, int32_t b)
{
    for (int it = 0; it < kUniteBound; ++it) {
        const int32_t ra = uf_find(parent, ra_seen), rb = uf_find(parent, b);
        ra_seen = ra;
        if (ra == rb) return true;
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        if (atomicCAS(parent + hi, hi, lo) == hi) { ra_seen = lo; return true; }
    }
    return false;
}

}  // namespace kpx
