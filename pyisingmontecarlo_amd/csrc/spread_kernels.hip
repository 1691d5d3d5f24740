// Translation unit of the lane-parallel resident lattice kernel (see spread_kernels.hpp for why it is apart from isingmc.hip).
#include "spread_kernels.hpp"

#include "kernel_pick.hpp"

namespace isingmc {

// f(kernel): the instantiation for one launch shape, for its launch and its occupancy query alike
template <typename F>
static void spread_pick(bool vec, bool pmj, int lanes_per_quad, int rounds, F &&f) // rounds is 7 or 10 (the callers have checked)
{
    pick(vec, pmj, or_last<8, 4, 2>{lanes_per_quad}, or_last<7, 10>{rounds},
         [&](auto V, auto P, auto L, auto N) { f(lat_resident_spread_kernel<V.value, P.value, L.value, N.value>); });
}

hipError_t spread_launch(bool vec, bool pmj, int lanes_per_quad, unsigned blocks, unsigned threads, size_t lds_bytes, hipStream_t stream, uint32_t *state,
                         const LatGeom &g, uint64_t t0, uint32_t timesteps, const uint2 *keys, const LatThr *thr_steps, uint32_t thr_stride,
                         const LatThr *thr_replica, const uint32_t *jneg, uint32_t jneg_uniform, unsigned long long *steps_out,
                         uint32_t n_replicas, int rounds)
{
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    spread_pick(vec, pmj, lanes_per_quad, rounds, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, stream, state, g, t0, timesteps, keys, thr_steps, thr_stride,
                           thr_replica, jneg, jneg_uniform, steps_out, n_replicas);
    });
    return hipGetLastError();
}

int spread_blocks_per_cu(bool vec, bool pmj, int lanes_per_quad, unsigned threads, size_t lds_bytes, int rounds)
{
    int n = 0;
    if (!philox_rounds_served(rounds)) return 0;
    spread_pick(vec, pmj, lanes_per_quad, rounds, [&](auto kernel) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, int(threads), lds_bytes) != hipSuccess) n = 0;
    });
    (void)hipGetLastError();
    return n;
}

} // namespace isingmc
