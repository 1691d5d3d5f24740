// Translation unit of the persistent strip kernel (see strip_types.hpp for why it is apart from isingmc.hip).
#include "strip_kernels.hpp"

#include "kernel_pick.hpp"

namespace isingmc {

// f(kernel, threads): the instantiation for (pmj, nw, ladder, rounds) and its workgroup size.  The plan sizes the persistent grid by the
// occupancy of the very kernel the launch runs (its workgroups wait on their neighbours' halos): both go through here.
template <typename F>
static void strip_pick(bool pmj, int nw, bool ladder, int rounds, F &&f) // rounds is 7 or 10 (the callers have checked)
{
    pick(pmj, or_last<1, 4>{nw}, ladder, or_last<7, 10>{rounds},
         [&](auto P, auto N, auto L, auto R) { f(lat_strip_kernel<P.value, N.value, L.value, R.value>, 64 * N.value); });
}

hipError_t strip_launch(bool pmj, int nw, unsigned blocks, size_t lds_bytes, hipStream_t stream, uint32_t *state, const LatGeom &g,
                        const StripArgs &a, uint64_t t0, uint32_t timesteps, const uint2 *keys, const LatThr *thr_steps,
                        uint32_t thr_stride, const LatThr *thr_replica, const uint32_t *jneg, uint32_t jneg_uniform,
                        unsigned long long *halo, unsigned long long *steps_out, const StripFinal &fin, const StripLadder &lad,
                        uint32_t n_replicas, uint32_t *err, int rounds)
{
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    strip_pick(pmj, nw, lad.ladder != nullptr, rounds, [&](auto kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, stream, state, g, a, t0, timesteps, keys, thr_steps, thr_stride,
                           thr_replica, jneg, jneg_uniform, halo, steps_out, fin, lad, n_replicas, err);
    });
    return hipGetLastError();
}

// workgroups of this instantiation that one CU holds at once, by the runtime's own occupancy calculation (registers, the
// launch's dynamic LDS, wave slots); 0 when the query fails
int strip_blocks_per_cu(bool pmj, int nw, bool ladder, size_t lds_bytes, int rounds)
{
    int n = 0;
    if (!philox_rounds_served(rounds)) return 0;
    strip_pick(pmj, nw, ladder, rounds, [&](auto kernel, int threads) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, lds_bytes) != hipSuccess) n = 0;
    });
    (void)hipGetLastError();
    return n;
}

} // namespace isingmc
