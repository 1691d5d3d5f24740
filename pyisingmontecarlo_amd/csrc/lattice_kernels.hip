// Translation unit of the checkerboard kernels (lattice_kernels.hpp): their instantiations and launchers (lattice_types.hpp).
#include "lattice_kernels.hpp"

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

// f(VEC, PMJ) with the two flags as compile-time constants
template <typename F>
static void lat_pick(bool vec, bool pmj, F &&f)
{
    if (vec) { if (pmj) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
    else { if (pmj) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

// f(VEC, PMJ, ROUNDS) for the kernels that draw the sweeps' random words; rounds is 7 or 10 (the launchers have checked)
template <typename F>
static void lat_pick_rounds(bool vec, bool pmj, int rounds, F &&f)
{
    lat_pick(vec, pmj, [&](auto V, auto P) {
        if (rounds == 7) f(V, P, std::integral_constant<int, 7>{});
        else f(V, P, std::integral_constant<int, 10>{});
    });
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
    lat_pick_rounds(vec, pmj, rounds, [&](auto V, auto P, auto N) {
        constexpr bool VEC = decltype(V)::value, PMJ = decltype(P)::value;
        constexpr int R = decltype(N)::value;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, lat_grid(g.nquads, n_replicas), dim3(256), lds_bytes, stream, state, g, colour, t, keys, thr, thr_replica,
                               jneg, jneg_uniform);
        };
        if (iters > 1)
            hipLaunchKernelGGL((lat_sweep_loop_kernel<PMJ, R>), dim3(g.nquads / (256 * iters), n_replicas, 1), dim3(256), lds_bytes, stream, state, g,
                               colour, t, keys, thr, thr_replica, jneg, jneg_uniform, iters);
        else if (uni) launch(lat_sweep_kernel<VEC, PMJ, VEC, R>); // division-free mapping
        else launch(lat_sweep_kernel<VEC, PMJ, false, R>);
    });
    return hipGetLastError();
}

int lat_sweep_loop_blocks_per_cu(bool pmj, unsigned lds_bytes, int rounds)
{
    int n = 0;
    hipError_t err = hipErrorInvalidValue;
    if (rounds == 10)
        err = pmj ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lat_sweep_loop_kernel<true>, 256, lds_bytes)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lat_sweep_loop_kernel<false>, 256, lds_bytes);
    else if (rounds == 7)
        err = pmj ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lat_sweep_loop_kernel<true, 7>, 256, lds_bytes)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lat_sweep_loop_kernel<false, 7>, 256, lds_bytes);
    if (err != hipSuccess) n = 0;
    (void)hipGetLastError();
    return n;
}

hipError_t lat_launch_sweep_measure(bool vec, bool pmj, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t,
                                    const uint2 *keys, const LatThr &thr, const LatThr *thr_replica, const uint32_t *jneg,
                                    uint32_t jneg_uniform, unsigned long long *out, size_t out_stride, int rounds)
{
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    lat_pick_rounds(vec, pmj, rounds, [&](auto V, auto P, auto N) {
        constexpr bool VEC = decltype(V)::value, PMJ = decltype(P)::value;
        constexpr int R = decltype(N)::value;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, lat_grid(g.nquads, n_replicas), dim3(256), 0, stream, state, g, t, keys, thr, thr_replica, jneg,
                               jneg_uniform, out, out_stride);
        };
        if (VEC && g.cols_log2 >= 0) launch(lat_sweep_measure_kernel<VEC, PMJ, VEC, R>);
        else launch(lat_sweep_measure_kernel<VEC, PMJ, false, R>);
    });
    return hipGetLastError();
}

hipError_t lat_launch_measure(bool vec, bool pmj, uint32_t n_replicas, hipStream_t stream, const uint32_t *state, const LatGeom &g,
                              const uint32_t *jneg, uint32_t jneg_uniform, unsigned long long *out, size_t out_stride)
{
    const uint32_t blocks = (g.nquads + 256 * MEASURE_QUADS_PER_THREAD - 1) / (256 * MEASURE_QUADS_PER_THREAD);
    lat_pick(vec, pmj, [&](auto V, auto P) {
        hipLaunchKernelGGL((lat_measure_kernel<decltype(V)::value, decltype(P)::value>), dim3(blocks, n_replicas), dim3(256), 0, stream, state, g,
                           jneg, jneg_uniform, out, out_stride);
    });
    return hipGetLastError();
}

hipError_t lat_launch_resident(bool vec, bool pmj, unsigned n_replicas, unsigned threads, size_t lds_bytes, hipStream_t stream, uint32_t *state,
                               const LatGeom &g, uint64_t t0, uint32_t timesteps, const uint2 *keys, const LatThr *thr_steps,
                               uint32_t thr_stride, const LatThr *thr_replica, const uint32_t *jneg, uint32_t jneg_uniform,
                               unsigned long long *steps_out, int rounds)
{
    if (!philox_rounds_served(rounds)) return hipErrorInvalidValue;
    lat_pick_rounds(vec, pmj, rounds, [&](auto V, auto P, auto N) {
        hipLaunchKernelGGL((lat_resident_kernel<decltype(V)::value, decltype(P)::value, decltype(N)::value>), dim3(n_replicas), dim3(threads), lds_bytes, stream, state,
                           g, t0, timesteps, keys, thr_steps, thr_stride, thr_replica, jneg, jneg_uniform, steps_out, uint32_t(n_replicas));
    });
    return hipGetLastError();
}

} // namespace isingmc
