// Translation unit of the bit-sliced replica-packed kernels (packed_kernels.hpp) and their launchers (packed_types.hpp).
#include "packed_kernels.hpp"

namespace isingmc {

hipError_t pk_launch_init(hipStream_t stream, uint32_t *state, const PkGraphDev &G, const uint2 *group_keys, uint32_t first_group, uint32_t n_groups)
{
    hipLaunchKernelGGL(pk_init_kernel, dim3((G.n_pos + 255) / 256, n_groups), dim3(256), 0, stream, state, G, group_keys, first_group);
    return hipGetLastError();
}

hipError_t pk_launch_init_replica(hipStream_t stream, uint32_t *state, const PkGraphDev &G, const uint2 *group_keys, uint32_t g, uint32_t bit)
{
    hipLaunchKernelGGL(pk_init_replica_kernel, dim3((G.n_pos + 255) / 256), dim3(256), 0, stream, state, G, group_keys, g, bit);
    return hipGetLastError();
}

hipError_t pk_launch_set_replica(hipStream_t stream, uint32_t *state, uint32_t n_pos, const uint32_t *bits, uint32_t g, uint32_t bit)
{
    hipLaunchKernelGGL(pk_set_replica_kernel, dim3((n_pos + 255) / 256), dim3(256), 0, stream, state, n_pos, bits, g, bit);
    return hipGetLastError();
}

hipError_t pk_launch_sweep(uint32_t n_groups, hipStream_t stream, uint32_t *state, const PkGraphDev &G, uint32_t class_begin, uint32_t class_end,
                           uint64_t t, const uint2 *group_keys, const uint32_t *tabs, uint32_t tab_stride)
{
    const uint32_t n = class_end - class_begin; // a thread decides four positions
    hipLaunchKernelGGL(pk_sweep_kernel, dim3(n / 1024 + (n % 1024 != 0), n_groups), dim3(256), 0, stream, state, G, class_begin, class_end, t,
                       group_keys, tabs, tab_stride);
    return hipGetLastError();
}

hipError_t pk_launch_measure(unsigned blocks, uint32_t n_groups, hipStream_t stream, const uint32_t *state, const PkGraphDev &G,
                             unsigned long long *out, uint32_t pos_per_thread, uint32_t sat_end, uint32_t sat_scale)
{
    hipLaunchKernelGGL(pk_measure_kernel, dim3(blocks, n_groups), dim3(256), 0, stream, state, G, out, 32 * n_groups, pos_per_thread, sat_end,
                       sat_scale);
    return hipGetLastError();
}

} // namespace isingmc
