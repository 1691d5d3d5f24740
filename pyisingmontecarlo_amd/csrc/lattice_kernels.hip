// Translation unit of the checkerboard kernels (lattice_kernels.hpp): their instantiations and launchers (lattice_types.hpp).
#include "lattice_kernels.hpp"

#include "kernel_pick.hpp"

namespace isingmc {

// Random initial configuration: word w of plane c = Philox(key, (0, w>>2, c<<8, "LATI"))[w&3].
__global__ __launch_bounds__(256) void lat_init_kernel(uint32_t *__restrict__ state, const LatGeom g,
                                                       const uint2 *__restrict__ keys,
                                                       const uint32_t first_replica)
{
    const uint32_t r = first_replica + blockIdx.y;
    const uint32_t Q = blockIdx.x * 256 + threadIdx.x;
    if (Q >= 2 * g.nquads) return;
    const uint32_t c = Q >= g.nquads, q = Q - c * g.nquads;
    const uint4 rnd = philox4x32_10(make_uint4(0, q, ctr2(0, c, 0), DOM_LAT_INIT), keys[r]);
    *reinterpret_cast<uint4 *>(state + size_t(r) * 2 * g.wpp + size_t(c) * g.wpp + 4 * size_t(q)) = rnd;
}

static dim3 lat_grid(uint32_t quads, uint32_t n_replicas) { return dim3((quads + 255) / 256, n_replicas, 1); }

// the Philox round count as a template argument; rounds is 7 or 10 (the launchers have checked)
using LatRounds = or_last<7, 10>;

// f(kernel): the instantiation of the looping kernel for (pmj, rounds), for its launch and its occupancy query alike
template <typename F>
static void lat_pick_sweep_loop(bool pmj, int rounds, F &&f)
{
    pick(pmj, LatRounds{rounds}, [&](auto P, auto N) { f(lat_sweep_loop_kernel<P.value, N.value>); });
}

hipError_t lat_launch_init(hipStream_t stream, uint32_t *state, const LatGeom &g, const uint2 *keys, uint32_t first_replica, uint32_t n_replicas)
{
    hipLaunchKernelGGL(lat_init_kernel, lat_grid(2 * g.nquads, n_replicas), dim3(256), 0, stream, state, g, keys, first_replica);
    return hipGetLastError();
}

hipError_t lat_launch_sweep(bool vec, bool pmj, uint32_t iters, uint32_t n_replicas, unsigned lds_bytes, hipStream_t stream, uint32_t *state,
                            const LatGeom &g, uint32_t colour, uint64_t t, const uint2 *keys, const LatThr &thr, const LatThr *thr_replica,
                            const uint32_t *jneg, uint32_t jneg_uniform, int rounds)
{
    const bool uni = vec && g.cols_log2 >= 0;
    if (iters > 1 && (!uni || g.nquads % (256 * iters) != 0)) return hipErrorInvalidValue;
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    if (iters > 1)
        lat_pick_sweep_loop(pmj, rounds, [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(g.nquads / (256 * iters), n_replicas, 1), dim3(256), lds_bytes, stream, state, g, colour, t, keys, thr,
                               thr_replica, jneg, jneg_uniform, iters);
        });
    else
        pick(vec, pmj, uni, LatRounds{rounds}, [&](auto V, auto P, auto U, auto N) {
            if constexpr (V.value || !U.value) // UNI, the division-free mapping, only together with VEC
                hipLaunchKernelGGL((lat_sweep_kernel<V.value, P.value, U.value, N.value>), lat_grid(g.nquads, n_replicas), dim3(256), lds_bytes, stream,
                                   state, g, colour, t, keys, thr, thr_replica, jneg, jneg_uniform);
        });
    return hipGetLastError();
}

int lat_sweep_loop_blocks_per_cu(bool pmj, unsigned lds_bytes, int rounds)
{
    int n = 0;
    if (philox_rounds_served(rounds))
        lat_pick_sweep_loop(pmj, rounds, [&](auto kernel) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, lds_bytes) != hipSuccess) n = 0;
        });
    (void)hipGetLastError();
    return n;
}

hipError_t lat_launch_sweep_measure(bool vec, bool pmj, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t,
                                    const uint2 *keys, const LatThr &thr, const LatThr *thr_replica, const uint32_t *jneg,
                                    uint32_t jneg_uniform, unsigned long long *out, size_t out_stride, int rounds)
{
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    pick(vec, pmj, vec && g.cols_log2 >= 0, LatRounds{rounds}, [&](auto V, auto P, auto U, auto N) {
        if constexpr (V.value || !U.value) // as in lat_launch_sweep
            hipLaunchKernelGGL((lat_sweep_measure_kernel<V.value, P.value, U.value, N.value>), lat_grid(g.nquads, n_replicas), dim3(256), 0, stream,
                               state, g, t, keys, thr, thr_replica, jneg, jneg_uniform, out, out_stride);
    });
    return hipGetLastError();
}

hipError_t lat_launch_measure(bool vec, bool pmj, uint32_t n_replicas, hipStream_t stream, const uint32_t *state, const LatGeom &g,
                              const uint32_t *jneg, uint32_t jneg_uniform, unsigned long long *out, size_t out_stride)
{
    const uint32_t blocks = (g.nquads + 256 * MEASURE_QUADS_PER_THREAD - 1) / (256 * MEASURE_QUADS_PER_THREAD);
    pick(vec, pmj, [&](auto V, auto P) {
        hipLaunchKernelGGL((lat_measure_kernel<V.value, P.value>), dim3(blocks, n_replicas), dim3(256), 0, stream, state, g, jneg, jneg_uniform, out,
                           out_stride);
    });
    return hipGetLastError();
}

hipError_t lat_launch_resident(bool vec, bool pmj, unsigned n_replicas, unsigned threads, size_t lds_bytes, hipStream_t stream, uint32_t *state,
                               const LatGeom &g, uint64_t t0, uint32_t timesteps, const uint2 *keys, const LatThr *thr_steps,
                               uint32_t thr_stride, const LatThr *thr_replica, const uint32_t *jneg, uint32_t jneg_uniform,
                               unsigned long long *steps_out, int rounds)
{
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    pick(vec, pmj, LatRounds{rounds}, [&](auto V, auto P, auto N) {
        hipLaunchKernelGGL((lat_resident_kernel<V.value, P.value, N.value>), dim3(n_replicas), dim3(threads), lds_bytes, stream, state, g, t0, timesteps,
                           keys, thr_steps, thr_stride, thr_replica, jneg, jneg_uniform, steps_out, uint32_t(n_replicas));
    });
    return hipGetLastError();
}

} // namespace isingmc
