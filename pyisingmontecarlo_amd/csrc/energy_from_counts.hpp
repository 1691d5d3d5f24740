// The f64 energy of one replica from the integer counters of its measurement, on the device: the one arithmetic that the
// energy_from_counts kernels of the tempering rounds (tempering_kernels.hip, real_kernels.hpp) and the store kernel of the observable
// series (observable_series_kernels.hip) share, so that both give the bits of the host's lattice_energy / pk_energy.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace isingmc {

// checkerboard lattice (periodic, no field): E = |J| (n_bonds - 2 sat)  (exact in f64)
__device__ __forceinline__ double lat_energy_of_counts(const double jabs, const long long n_bonds, const unsigned long long sat)
{
    return jabs * double(n_bonds - 2 * (long long)sat);
}

// bit-sliced packed family: E = |J| (undirected bonds - directed satisfied count) + self loops
__device__ __forceinline__ double pk_energy_of_counts(const double jabs, const double half_directed, const double self_energy,
                                                      const unsigned long long sat)
{
    return jabs * (half_directed - double((long long)sat)) + self_energy;
}

// real-coupling packed family: hi, lo = -2 x the exact integer sums of the two levels; E = (2^kE hi + 2^(kE - 24) lo) + self loops
__device__ __forceinline__ double rj_energy_of_counts(const int k_energy, const double self_energy, const unsigned long long c_hi,
                                                      const unsigned long long c_lo)
{
    const long long hi = (long long)c_hi, lo = (long long)c_lo;
    return (ldexp(double(-(hi / 2)), k_energy) + ldexp(double(-(lo / 2)), k_energy - 24)) + self_energy;
}

} // namespace isingmc
