// A 128-bit integer sum as two 64-bit words, shared by the cluster-size moments (cluster_moments.hpp: sum s^4) and the overlap
// numerators of the population-annealing step chooser (pa_kernels.hip).  Integer additions only: a sum does not depend on the
// order in which it is taken.
#pragma once
#include <hip/hip_runtime.h>

namespace isingmc {

struct Sum128 {
    unsigned long long lo = 0, hi = 0;

    __device__ __forceinline__ void add(unsigned long long a_lo, unsigned long long a_hi)
    {
        lo += a_lo;
        hi += a_hi + (lo < a_lo ? 1ull : 0ull);
    }
    // this lane's sum + that of lane (lane ^ mask)
    __device__ __forceinline__ void add_lane_xor(int mask)
    {
        const unsigned long long olo = __shfl_xor(lo, mask), ohi = __shfl_xor(hi, mask);
        add(olo, ohi);
    }
    // onto the pair of words (*dst_lo, *dst_hi) that other workgroups add to as well: one 64-bit atomic per word; the add that
    // makes the low word wrap carries one into the high word
    __device__ __forceinline__ void atomic_add_to(unsigned long long *dst_lo, unsigned long long *dst_hi) const
    {
        const unsigned long long old = atomicAdd(dst_lo, lo);
        const unsigned long long h = hi + (old + lo < old ? 1ull : 0ull);
        if (h) atomicAdd(dst_hi, h);
    }
};

} // namespace isingmc
