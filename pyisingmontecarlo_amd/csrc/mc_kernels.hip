// Translation unit of the multi-class checkerboard kernels (mc_types.hpp).
#include "mc_kernels.hpp"

#include "kernel_pick.hpp"

namespace isingmc {

using McMode = or_last<MC_FIELD, MC_ANISO, MC_FIELD_OPEN, MC_OPEN>;

// the sign-plane (FNEG) instantiations exist for the modes with a field alone
template <int MODE>
constexpr bool mc_takes_fneg = MODE == MC_FIELD || MODE == MC_FIELD_OPEN;

hipError_t mc_launch_sweep(int mode, bool pmj, dim3 grid, hipStream_t stream, uint32_t *state, const LatGeom &g, uint32_t colour,
                           uint64_t t, const uint2 *keys, const LatThrMC &thr_uniform, const LatThrMC *thr_replica,
                           const uint32_t *jneg, uint32_t jneg_uniform, McOpen open, const uint32_t *fneg)
{
    const bool uni = g.cols_log2 >= 0; // the 2^k mapping of the streaming kernels applies (build_lattice)
    pick(McMode{mode}, pmj, uni, fneg != nullptr, [&](auto M, auto P, auto U, auto F) {
        hipLaunchKernelGGL((lat_mc_sweep_kernel<M.value, P.value, U.value, F.value && mc_takes_fneg<M.value>>), grid, dim3(256), 0, stream, state, g,
                           colour, t, keys, thr_uniform, thr_replica, jneg, jneg_uniform, open, fneg);
    });
    return hipGetLastError();
}

hipError_t mc_launch_resident(int mode, bool pmj, unsigned n_replicas, unsigned threads, size_t lds_bytes, hipStream_t stream,
                              uint32_t *state, const LatGeom &g, uint64_t t0, uint32_t timesteps, const uint2 *keys,
                              const LatThrMC *thr_steps, uint32_t thr_stride, const LatThrMC *thr_replica, const uint32_t *jneg,
                              uint32_t jneg_uniform, McOpen open, const uint32_t *fneg, unsigned long long *steps_out,
                              uint32_t steps_replicas)
{
    // lds_bytes beyond the two planes: room for the spread variant's random words (128 bytes per quad)
    const bool spread = lds_bytes > size_t(2) * g.wpp * sizeof(uint32_t);
    pick(McMode{mode}, pmj, fneg != nullptr, spread, [&](auto M, auto P, auto F, auto S) {
        hipLaunchKernelGGL((lat_mc_resident_kernel<M.value, P.value, F.value && mc_takes_fneg<M.value>, S.value>), dim3(n_replicas), dim3(threads),
                           lds_bytes, stream, state, g, t0, timesteps, keys, thr_steps, thr_stride, thr_replica, jneg, jneg_uniform, open, fneg,
                           steps_out, steps_replicas);
    });
    return hipGetLastError();
}

hipError_t mc_launch_measure_aniso(bool pmj, dim3 grid, hipStream_t stream, const uint32_t *state, const LatGeom &g, const uint32_t *jneg,
                                   uint32_t jneg_uniform, unsigned long long *out, size_t out_stride)
{
    pick(pmj, [&](auto P) {
        hipLaunchKernelGGL(lat_mc_measure_aniso_kernel<P.value>, grid, dim3(256), 0, stream, state, g, jneg, jneg_uniform, out, out_stride);
    });
    return hipGetLastError();
}

hipError_t mc_launch_measure_open(bool pmj, dim3 grid, hipStream_t stream, const uint32_t *state, const LatGeom &g, const uint32_t *jneg,
                                  uint32_t jneg_uniform, McOpen open, const uint32_t *fneg, unsigned long long *out, size_t out_stride)
{
    pick(pmj, [&](auto P) {
        hipLaunchKernelGGL(lat_mc_measure_open_kernel<P.value>, grid, dim3(256), 0, stream, state, g, jneg, jneg_uniform, open, fneg, out, out_stride);
    });
    return hipGetLastError();
}

} // namespace isingmc
