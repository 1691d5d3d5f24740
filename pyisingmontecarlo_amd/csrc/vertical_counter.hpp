// Bit-sliced vertical counter: K words hold 32 independent K-bit counters, counter b in bit b of every plane,
// plane 0 least significant.  Adding a word costs one AND and one XOR per plane the carry reaches; the 32 integers are only
// formed when the counter is read.  A counter holds up to 2^K - 1: the caller reads and clears it before it adds more.
// Host and device: tests/vertical_counter_host.cpp checks it against per-bit counts without a GPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VC_HD __host__ __device__ __forceinline__
#define VC_UNROLL _Pragma("unroll")
#else
#define VC_HD inline
#define VC_UNROLL
#endif

namespace isingmc {

// every counter b += bit b of `word` (ripple carry-save; the carry out of the top plane is dropped: the caller's bound)
template <int K>
VC_HD void vc_add(uint32_t (&planes)[K], uint32_t word)
{
    VC_UNROLL
    for (int j = 0; j < K; j++) {
        const uint32_t t = planes[j] & word;
        planes[j] ^= word;
        word = t;
    }
}

// the same on k planes that lie `stride` words apart in memory (the time planes of the per-replica sums); stops where the carry ends
VC_HD void vc_add_strided(uint32_t *planes, uint64_t stride, int k, uint32_t word)
{
    for (int j = 0; j < k && word; j++) {
        const uint32_t p = planes[j * stride], t = p & word;
        planes[j * stride] = p ^ word;
        word = t;
    }
}

// the value of counter `bit`
template <int K>
VC_HD uint32_t vc_value(const uint32_t (&planes)[K], int bit)
{
    uint32_t v = 0;
    VC_UNROLL
    for (int j = 0; j < K; j++) v |= ((planes[j] >> bit) & 1u) << j;
    return v;
}

// all 32 values
template <int K>
VC_HD void vc_expand(const uint32_t (&planes)[K], uint32_t (&out)[32])
{
    VC_UNROLL
    for (int b = 0; b < 32; b++) out[b] = vc_value(planes, b);
}

} // namespace isingmc
