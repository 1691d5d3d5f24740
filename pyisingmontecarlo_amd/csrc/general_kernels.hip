// Translation unit of the general edge-list kernels (general_kernels.hpp): their instantiations and launchers (general_launch.hpp).
#include "general_kernels.hpp"
#include "general_launch.hpp"

#include "kernel_pick.hpp"

namespace isingmc {

hipError_t gen_launch_init(hipStream_t stream, uint32_t *state, const GenGraphDev &G, const uint2 *keys, uint32_t first_replica, uint32_t n_replicas)
{
    hipLaunchKernelGGL(gen_init_kernel, dim3((G.n_words + 255) / 256, n_replicas), dim3(256), 0, stream, state, G, keys, first_replica);
    return hipGetLastError();
}

// the weight type of the kernels from the flag's tag
template <typename IsFloat>
using GenWeight = std::conditional_t<IsFloat::value, float, double>;

hipError_t gen_launch_sweep(bool w_is_float, int rb, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const GenGraphDev &G,
                            uint32_t class_begin, uint32_t class_end, uint64_t t, const uint2 *keys, double beta, const double *beta_replica)
{
    const dim3 grid((class_end - class_begin + 255) / 256, (n_replicas + unsigned(rb) - 1) / unsigned(rb));
    const bool served = pick(w_is_float, one_of<8, 4, 2, 1>{rb}, [&](auto W, auto RB) {
        hipLaunchKernelGGL((gen_sweep_kernel<GenWeight<decltype(W)>, RB.value>), grid, dim3(256), 0, stream, state, G, class_begin, class_end, t, keys,
                           beta, beta_replica, n_replicas);
    });
    return served ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t gen_launch_measure(bool w_is_float, uint32_t n_replicas, uint32_t n_partials, hipStream_t stream, const uint32_t *state,
                              const GenGraphDev &G, double *partial_e, long long *partial_m)
{
    const dim3 grid(n_partials, n_replicas);
    pick(w_is_float, [&](auto W) {
        hipLaunchKernelGGL(gen_measure_kernel<GenWeight<decltype(W)>>, grid, dim3(256), 0, stream, state, G, partial_e, partial_m);
    });
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
    pick(w_is_float, or_last<1, 2, 0>{stage}, [&](auto W, auto STAGE) {
        const auto kernel = gen_resident_kernel<GenWeight<decltype(W)>, STAGE.value>;
        if (lds_bytes > 64 * 1024) // beyond the default limit of dynamic LDS
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
        hipLaunchKernelGGL(kernel, dim3(n_replicas), dim3(threads), lds_bytes, stream, state, G, t0, timesteps, keys, beta_steps, beta_stride,
                           beta_replica, energies_out, self_energy, edges2);
    });
    return hipGetLastError();
}

} // namespace isingmc
