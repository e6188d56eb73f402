// unionfind.hip.h -- a lock-free union-find over a uint32_t array, for the device (isccsearch_join_components: the LINK form of the
// join kernels' emit paths, flatten_kernel) and, the SAME text, for a host program (tests/unionfind_host.cpp runs it under threads).
//
// parent[x] <= x ALWAYS: a root (parent[r] == r) is hooked only under a SMALLER label, by a compare-exchange that expects
// parent[r] == r, and compression replaces a parent by one of its ancestors.  So there is no cycle, every value an entry ever holds is
// <= its index and only decreases, and the root of a component is its smallest label.  No locks, and nothing waits for another
// lane: every loop below ends because labels strictly decrease along a path, and a failed exchange means that another lane's
// exchange on the same entry succeeded -- the entry went down, which it can do at most `index` times.
//
// The two atomics (relaxed: the array carries no other data, and the calls that read the result come after the kernels):
//   uf_load(p)          the entry
//   uf_cas(p, e, d)     *p == e ? (*p = d, e) : *p       -- the value found
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UF_FN __host__ __device__ inline
#else
#define UF_FN inline
#endif

namespace isk {

constexpr uint32_t UF_NONE = 0xFFFFFFFFu;     // a row without a label: compared, never linked, never counted

UF_FN uint32_t uf_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
UF_FN uint32_t uf_cas(uint32_t* p, uint32_t expected, uint32_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
    return expected;
}

// The root of x.  Path halving: an entry whose parent is no root is pointed at its grandparent -- an ancestor, and the entry is
// no root (its parent differs from it), so a root is never written.  Without it a dense cluster hooked in label order is a chain
// that every later find walks.  x strictly decreases per trip.
UF_FN uint32_t uf_find(uint32_t* parent, uint32_t x) {
    uint32_t p = uf_load(parent + x);
    while (p != x) {
        const uint32_t g = uf_load(parent + p);
        if (g != p) uf_cas(parent + x, p, g);      // (lost to another lane: that lane pointed x at an ancestor too)
        x = p;
        p = g;
    }
    return x;
}

// One link: afterwards a and b have one root.  The larger root is hooked under the smaller label; a failed exchange (the root was
// hooked or compressed by another lane meanwhile) goes on from the value it found, an ancestor of that root.
UF_FN void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t seen = uf_cas(parent + a, a, b);
        if (seen == a) return;
        a = seen;
    }
}

// The flatten step for one label, run for every label once no union is in flight: parent[i] = the root of i.  The roots are final
// then, and an entry never goes below its root, so the exchange loop (other lanes' finds still compress) ends at the root.
UF_FN void uf_flatten(uint32_t* parent, uint32_t i) {
    const uint32_t r = uf_find(parent, i);
    uint32_t p = uf_load(parent + i);
    while (p > r) {
        const uint32_t seen = uf_cas(parent + i, p, r);
        if (seen == p) return;
        p = seen;
    }
}

}  // namespace isk
