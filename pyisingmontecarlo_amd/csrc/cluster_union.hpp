// Union-find on a label array that other threads link concurrently (LDS: workgroup scope, global: agent scope), shared by
// cluster_kernels.hip (S8-S10) and, through packed_label.hpp, packed_cluster_kernels.hip (S11), packed_icm_kernels.hip (S12)
// and packed_between_kernels.hip (S13).  Every union links a root to a SMALLER label with an integer atomicMin, so the final
// root of a component is its smallest member whatever the order of execution, and every loop walks strictly decreasing labels:
// it ends without waiting for any other thread.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace isingmc {

template <int SCOPE>
__device__ __forceinline__ uint32_t cl_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// labels live at lab[STRIDE * a] (STRIDE > 1: several label arrays interleaved)
template <int SCOPE, uint32_t STRIDE = 1>
__device__ __forceinline__ uint32_t cl_find(const uint32_t *lab, uint32_t a)
{
    for (uint32_t p = cl_load<SCOPE>(lab + size_t(STRIDE) * a); p != a; p = cl_load<SCOPE>(lab + size_t(STRIDE) * a)) a = p; // p < a: strictly decreasing
    return a;
}

template <int SCOPE, uint32_t STRIDE = 1>
__device__ __forceinline__ void cl_unite(uint32_t *lab, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cl_find<SCOPE, STRIDE>(lab, a);
        b = cl_find<SCOPE, STRIDE>(lab, b);
        if (a == b) return;
        if (a < b) { const uint32_t x = a; a = b; b = x; }
        // a > b: hang root a below b.  If a has stopped being a root meanwhile, its label is now min(old, b) -- still a member
        // of the same component -- and the union goes on between old (< a) and b.
        const uint32_t old = __hip_atomic_fetch_min(lab + size_t(STRIDE) * a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

} // namespace isingmc
