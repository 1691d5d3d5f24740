// Kernels of the observable series.  See observable_series_kernels.hpp.
//   obs_store_kernel        counters -> energy and magnetisation entries of a row, one thread per column
//   obs_class_store_kernel  class counters -> the by-class entries of a row, one thread per (column, bin), bins fastest
//   obs_lat_class_kernel    checkerboard path: the up spins of one configuration per grid row by site class (lat_class_count.hpp,
//                           the counting of the overlap class kernels with the configuration's own words)
#include "observable_series_kernels.hpp"

#include <algorithm>

#include "energy_from_counts.hpp"
#include "lat_class_count.hpp"

namespace isingmc {

constexpr unsigned OBS_THREADS = 256;
constexpr unsigned long long OBS_MAX_BLOCKS = 4096; // a grid-stride loop covers what is left

// consecutive threads write consecutive entries of row_e and of row_m; the permutation and the counters are gathered
__global__ void __launch_bounds__(OBS_THREADS) obs_store_kernel(const ObsStore S)
{
    for (uint32_t i = blockIdx.x * OBS_THREADS + threadIdx.x; i < S.n_columns; i += gridDim.x * OBS_THREADS) {
        const size_t slot = size_t(S.first_slot) + (S.perm ? S.perm[i] : i);
        if (S.row_e) {
            const unsigned long long c0 = S.cnt_e[2 * slot];
            double e;
            if (S.family == OBS_LATTICE) e = lat_energy_of_counts(S.jabs, S.n_bonds, c0);
            else if (S.family == OBS_PACKED) e = pk_energy_of_counts(S.jabs, S.half_directed, S.self_energy, c0);
            else e = rj_energy_of_counts(S.k_energy, S.self_energy, c0, S.cnt_e[2 * slot + 1]);
            S.row_e[i] = e;
        }
        if (S.row_m) S.row_m[i] = 2ll * (long long)S.cnt_u[2 * slot + 1] - S.nvars;
    }
}

__global__ void __launch_bounds__(OBS_THREADS) obs_class_store_kernel(const ObsClassStore S)
{
    const unsigned long long total = (unsigned long long)S.n_columns * S.bins, stride = (unsigned long long)gridDim.x * OBS_THREADS;
    for (unsigned long long idx = (unsigned long long)blockIdx.x * OBS_THREADS + threadIdx.x; idx < total; idx += stride) {
        const uint32_t c = uint32_t(idx / S.bins), b = uint32_t(idx - (unsigned long long)c * S.bins), i = S.column0 + c;
        const unsigned long long slot = (unsigned long long)S.first_slot + (S.perm ? S.perm[i] : i);
        if (slot < S.slot0 || slot - S.slot0 >= S.n_slots) continue;
        S.row[(unsigned long long)i * S.bins + b] = 2ll * (long long)S.acc[(slot - S.slot0) * S.bins + b] - (long long)S.sizes[b];
    }
}

// grid: (lat_class_blocks, n); grid row r = replica r of `state`; dynamic LDS: 4 bytes per bin
__global__ __launch_bounds__(256) void obs_lat_class_kernel(const uint32_t *__restrict__ state, const LatGeom g, const LatClassDev C,
                                                            unsigned long long *__restrict__ out)
{
    const uint32_t r = blockIdx.y;
    const uint32_t *s = state + size_t(r) * 2 * g.wpp;
    lat_class_count([&](uint32_t pw) { return s[pw]; }, g, C, out + size_t(r) * C.n_tables * C.n_classes);
}

hipError_t obs_launch_store(hipStream_t stream, const ObsStore &S)
{
    if (S.n_columns == 0 || (!S.row_e && !S.row_m)) return hipSuccess;
    const unsigned blocks = unsigned(std::min<unsigned long long>((S.n_columns + OBS_THREADS - 1) / OBS_THREADS, OBS_MAX_BLOCKS));
    hipLaunchKernelGGL(obs_store_kernel, dim3(blocks), dim3(OBS_THREADS), 0, stream, S);
    return hipGetLastError();
}

hipError_t obs_launch_class_store(hipStream_t stream, const ObsClassStore &S)
{
    const unsigned long long total = (unsigned long long)S.n_columns * S.bins;
    if (total == 0 || S.n_slots == 0) return hipSuccess;
    const unsigned blocks = unsigned(std::min<unsigned long long>((total + OBS_THREADS - 1) / OBS_THREADS, OBS_MAX_BLOCKS));
    hipLaunchKernelGGL(obs_class_store_kernel, dim3(blocks), dim3(OBS_THREADS), 0, stream, S);
    return hipGetLastError();
}

hipError_t obs_launch_lat_class(hipStream_t stream, const uint32_t *state, const LatGeom &g, const LatClassDev &C, uint32_t n,
                                unsigned long long *out)
{
    if (n == 0) return hipSuccess;
    const uint32_t lds = C.n_tables * C.n_classes * uint32_t(sizeof(uint32_t));
    hipLaunchKernelGGL(obs_lat_class_kernel, dim3(lat_class_blocks(g), n), dim3(256), lds, stream, state, g, C, out);
    return hipGetLastError();
}

} // namespace isingmc
