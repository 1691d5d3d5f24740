// Each replica's lowest-energy configuration: the decision and the two conditional copies.
//   best_decide_kernel<PACKED>   one thread per counter slot: e < best_e => new record; a flag per replica, or one ballot-formed
//                                32-bit mask per replica group (a wave64 covers two groups); one 64-bit atomic per wave with
//                                an improved replica
//   best_keep_rows_kernel        checkerboard path, one grid row per replica: the flag is a wave-uniform read (blockIdx.y) and an
//                                unflagged row exits at once; 16 bytes per thread
//   best_keep_bits_kernel        packed paths, one grid row per replica group: the mask is a wave-uniform read; no improved
//                                replica: exit; every owned replica improved: a copy; else a merge under the mask
// Nothing is written but the records, the flags / masks, the counter and the best buffer.
#include "best_kernels.hpp"

#include <algorithm>

#include "kernel_pick.hpp"

namespace isingmc {

namespace {

constexpr size_t BEST_MAX_GRID_Y = 32768;

template <bool PACKED>
__global__ __launch_bounds__(256) void best_decide_kernel(const double *__restrict__ energy, const uint32_t n, const uint32_t bit0,
                                                          const uint32_t n_slots, const unsigned long long t, double *__restrict__ best_e,
                                                          unsigned long long *__restrict__ best_t, uint32_t *__restrict__ out,
                                                          unsigned long long *__restrict__ improved)
{
    const uint32_t sl = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t r = sl - bit0; // (a slot below bit0 wraps beyond n)
    bool better = false;
    if (sl < n_slots && sl >= bit0 && r < n) {
        const double e = energy[r];
        if (e < best_e[r]) {
            best_e[r] = e;
            best_t[r] = t;
            better = true;
        }
    }
    const unsigned long long b = __ballot(better); // every lane of the wave arrives here
    if (PACKED) {
        if ((lane & 31u) == 0 && sl < n_slots) out[sl >> 5] = uint32_t(b >> lane); // lanes 0 and 32: the wave's two groups
    } else if (sl < n_slots) {
        out[sl] = better ? 1u : 0u;
    }
    if (lane == 0 && b) atomicAdd(improved, (unsigned long long)__popcll(b));
}

// grid: (ceil(nv / 256), replicas of this launch); nv = uint4 per row
__global__ __launch_bounds__(256) void best_keep_rows_kernel(const uint4 *__restrict__ state, uint4 *__restrict__ best,
                                                             const uint32_t *__restrict__ flags, const uint32_t r0, const uint32_t nv)
{
    const uint32_t r = r0 + blockIdx.y;
    if (flags[r] == 0) return;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < nv) best[size_t(r) * nv + i] = state[size_t(r) * nv + i];
}

// grid: (ceil(nv / 256), groups of this launch); nv = uint4 per group
__global__ __launch_bounds__(256) void best_keep_bits_kernel(const uint4 *__restrict__ state, uint4 *__restrict__ best,
                                                             const uint32_t *__restrict__ masks, const uint32_t n, const uint32_t bit0,
                                                             const uint32_t g0, const uint32_t nv)
{
    const uint32_t g = g0 + blockIdx.y;
    const uint32_t m = masks[g];
    if (m == 0) return;
    // the bits of this group the container owns: slots [bit0, bit0 + n) cut to the group (not empty: one of them improved)
    const uint32_t lo = max(32u * g, bit0), hi = min(32u * g + 32u, bit0 + n);
    const uint32_t own = hi - lo >= 32u ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u) << (lo & 31u);
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const size_t at = size_t(g) * nv + i;
    uint4 s = state[at];
    if (m != own) { // wave-uniform
        const uint4 b = best[at];
        s.x = (b.x & ~m) | (s.x & m);
        s.y = (b.y & ~m) | (s.y & m);
        s.z = (b.z & ~m) | (s.z & m);
        s.w = (b.w & ~m) | (s.w & m);
    }
    best[at] = s;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

} // namespace

hipError_t best_launch_decide(hipStream_t stream, bool packed, const double *energy, uint32_t n, uint32_t bit0, uint32_t n_groups, uint64_t t,
                              double *best_e, unsigned long long *best_t, uint32_t *out, unsigned long long *improved)
{
    const uint32_t n_slots = packed ? 32u * n_groups : n;
    if (n_slots == 0) return hipSuccess;
    const dim3 grid((n_slots + 255) / 256);
    pick(packed, [&](auto PACKED) { // (replica slots, not bits of a group: no first bit)
        hipLaunchKernelGGL(best_decide_kernel<PACKED.value>, grid, dim3(256), 0, stream, energy, n, PACKED.value ? bit0 : 0u, n_slots,
                           (unsigned long long)t, best_e, best_t, out, improved);
    });
    return hipGetLastError();
}

hipError_t best_launch_keep_rows(hipStream_t stream, const uint32_t *state, uint32_t *best, const uint32_t *flags, size_t R, size_t state_words)
{
    if (state_words % 4 != 0 || state_words / 4 > 0xFFFFFFFFull || !aligned16(state) || !aligned16(best)) return hipErrorInvalidValue;
    const uint32_t nv = uint32_t(state_words / 4);
    for (size_t r0 = 0; r0 < R; r0 += BEST_MAX_GRID_Y)
        hipLaunchKernelGGL(best_keep_rows_kernel, dim3((nv + 255) / 256, unsigned(std::min(BEST_MAX_GRID_Y, R - r0))), dim3(256), 0, stream,
                           reinterpret_cast<const uint4 *>(state), reinterpret_cast<uint4 *>(best), flags, uint32_t(r0), nv);
    return hipGetLastError();
}

hipError_t best_launch_keep_bits(hipStream_t stream, const uint32_t *state, uint32_t *best, const uint32_t *masks, uint32_t n, uint32_t bit0,
                                 size_t groups, uint32_t n_pos)
{
    if (n_pos % 4 != 0 || !aligned16(state) || !aligned16(best)) return hipErrorInvalidValue;
    const uint32_t nv = n_pos / 4;
    for (size_t g0 = 0; g0 < groups; g0 += BEST_MAX_GRID_Y)
        hipLaunchKernelGGL(best_keep_bits_kernel, dim3((nv + 255) / 256, unsigned(std::min(BEST_MAX_GRID_Y, groups - g0))), dim3(256), 0, stream,
                           reinterpret_cast<const uint4 *>(state), reinterpret_cast<uint4 *>(best), masks, n, bit0, uint32_t(g0), nv);
    return hipGetLastError();
}

} // namespace isingmc
