// Translation unit of the general edge-list kernels (general_kernels.hpp): their instantiations and launchers (general_launch.hpp).
#include "general_kernels.hpp"
#include "general_launch.hpp"

namespace isingmc {

hipError_t gen_launch_init(hipStream_t stream, uint32_t *state, const GenGraphDev &G, const uint2 *keys, uint32_t first_replica, uint32_t n_replicas)
{
    hipLaunchKernelGGL(gen_init_kernel, dim3((G.n_words + 255) / 256, n_replicas), dim3(256), 0, stream, state, G, keys, first_replica);
    return hipGetLastError();
}

template <typename WT>
static hipError_t gen_launch_sweep_wt(int rb, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const GenGraphDev &G, uint32_t class_begin,
                                      uint32_t class_end, uint64_t t, const uint2 *keys, double beta, const double *beta_replica)
{
    const dim3 grid((class_end - class_begin + 255) / 256, (n_replicas + unsigned(rb) - 1) / unsigned(rb));
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, state, G, class_begin, class_end, t, keys, beta, beta_replica, n_replicas);
    };
    if (rb == 8) launch(gen_sweep_kernel<WT, 8>);
    else if (rb == 4) launch(gen_sweep_kernel<WT, 4>);
    else if (rb == 2) launch(gen_sweep_kernel<WT, 2>);
    else if (rb == 1) launch(gen_sweep_kernel<WT, 1>);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t gen_launch_sweep(bool w_is_float, int rb, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const GenGraphDev &G,
                            uint32_t class_begin, uint32_t class_end, uint64_t t, const uint2 *keys, double beta, const double *beta_replica)
{
    return w_is_float ? gen_launch_sweep_wt<float>(rb, n_replicas, stream, state, G, class_begin, class_end, t, keys, beta, beta_replica)
                      : gen_launch_sweep_wt<double>(rb, n_replicas, stream, state, G, class_begin, class_end, t, keys, beta, beta_replica);
}

hipError_t gen_launch_measure(bool w_is_float, uint32_t n_replicas, uint32_t n_partials, hipStream_t stream, const uint32_t *state,
                              const GenGraphDev &G, double *partial_e, long long *partial_m)
{
    const dim3 grid(n_partials, n_replicas);
    if (w_is_float) hipLaunchKernelGGL(gen_measure_kernel<float>, grid, dim3(256), 0, stream, state, G, partial_e, partial_m);
    else hipLaunchKernelGGL(gen_measure_kernel<double>, grid, dim3(256), 0, stream, state, G, partial_e, partial_m);
    return hipGetLastError();
}

hipError_t gen_launch_reduce(hipStream_t stream, const double *partial_e, const long long *partial_m, uint32_t n_partials, uint32_t n_replicas,
                             double *out_e, long long *out_m)
{
    hipLaunchKernelGGL(gen_reduce_kernel, dim3(n_replicas), dim3(256), 0, stream, partial_e, partial_m, n_partials, out_e, out_m);
    return hipGetLastError();
}

hipError_t gen_launch_resident(bool w_is_float, int stage, unsigned n_replicas, unsigned threads, size_t lds_bytes, hipStream_t stream,
                               uint32_t *state, const GenGraphDev &G, uint64_t t0, uint32_t timesteps, const uint2 *keys,
                               const double *beta_steps, uint32_t beta_stride, const double *beta_replica, double *energies_out,
                               double self_energy, uint32_t edges2)
{
    const auto launch = [&](auto kernel) {
        if (lds_bytes > 64 * 1024) // beyond the default limit of dynamic LDS
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
        hipLaunchKernelGGL(kernel, dim3(n_replicas), dim3(threads), lds_bytes, stream, state, G, t0, timesteps, keys, beta_steps, beta_stride,
                           beta_replica, energies_out, self_energy, edges2);
    };
    if (w_is_float) {
        if (stage == 1) launch(gen_resident_kernel<float, 1>); else if (stage == 2) launch(gen_resident_kernel<float, 2>); else launch(gen_resident_kernel<float, 0>);
    } else {
        if (stage == 1) launch(gen_resident_kernel<double, 1>); else if (stage == 2) launch(gen_resident_kernel<double, 2>); else launch(gen_resident_kernel<double, 0>);
    }
    return hipGetLastError();
}

} // namespace isingmc
