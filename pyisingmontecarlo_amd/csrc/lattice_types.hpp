// Host-visible types of the checkerboard path (lattice_kernels.hpp): the geometry, the thresholds and the fixed-point format.
// Headers that only pass these on include this file, not the kernels: lattice_kernels.hpp defines kernels that are no templates,
// and every translation unit that sees them compiles them into its own code object.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace isingmc {

struct LatGeom {
    uint32_t W, H;
    uint32_t wpr;    // words per colour-row = W / 64
    uint32_t wpp;    // words per plane = H * wpr
    uint32_t nquads; // wpp / 4
    int32_t cols_log2; // log2(quads per row) when the division-free, parity-uniform thread mapping applies, else -1
};

struct LatThr {
    uint64_t T3, T4; // floor(exp(-beta dE) 2^THR_BITS) for k = 3, 4; 2^THR_BITS = always accept
};

#ifndef ISINGMC_N_PLANES
#define ISINGMC_N_PLANES 7
#endif
constexpr int N_PLANES = ISINGMC_N_PLANES;
constexpr int THR_BITS = N_PLANES + 32; // acceptance probabilities are fixed-point with this many bits

} // namespace isingmc
