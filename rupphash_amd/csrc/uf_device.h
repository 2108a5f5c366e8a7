// uf_device.h -- the device functions the union-find kernels share (components.hip, merge_tree.hip).
//
// parent[] is a forest in which every pointer goes to a smaller index (parent[x] <= x, a root points at itself).  Every access to it
// is a relaxed agent-scope atomic (loads that go past the CU's L1, vector atomics for the writes); the only property a walk relies on
// is that a value read from parent[x], however old, is x itself or an ancestor of x -- once an ancestor, always an ancestor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UF_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ uint32_t uf_parent(const uint32_t *parent, uint32_t x) { return __hip_atomic_load(parent + x, UF_RELAXED); }

// The root of x, halving the path on the way.  The walk goes to strictly smaller indices, so it ends after at most x steps whatever
// other lanes do.  fetch_min, not a store: two lanes that shorten the same pointer leave the smaller ancestor, so a pointer never rises.
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = uf_parent(parent, x);
    while (p != x) {
        const uint32_t gp = uf_parent(parent, p);
        if (gp != p) __hip_atomic_fetch_min(parent + x, gp, UF_RELAXED);
        x = p;
        p = gp;
    }
    return x;
}
