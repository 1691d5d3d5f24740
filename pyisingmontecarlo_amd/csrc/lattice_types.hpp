// Host-visible side of the checkerboard path: the geometry, the thresholds, the fixed-point format, and the launchers of
// lattice_kernels.hip (the kernels are in lattice_kernels.hpp).
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

constexpr uint32_t MEASURE_SLOTS = 16;            // partial counter pairs per replica of lat_sweep_measure_kernel (the host sums them)
constexpr uint32_t MEASURE_QUADS_PER_THREAD = 16; // quads a thread of lat_measure_kernel walks
constexpr uint32_t LDS_RESIDENT_MAX_BYTES = 64 * 1024; // both planes of a replica of the LDS-resident kernels

// ---- launchers (lattice_kernels.hip).  vec / pmj: quads inside one row (wpr % 4 == 0) / couplings of both signs; grid.y or
// grid.x = n_replicas, whose planes, keys and thr_replica entries (nullptr: thr for all) begin at the pointers passed.
// rounds: of the sweeps' Philox calls, 10 or 7 (anything else is hipErrorInvalidValue) -- the launcher picks the instantiation
hipError_t lat_launch_init(hipStream_t stream, uint32_t *state, const LatGeom &g, const uint2 *keys, uint32_t first_replica, uint32_t n_replicas);
// one colour of one timestep.  iters quads per thread: 1 = lat_sweep_kernel (with the division-free mapping when vec and
// g.cols_log2 >= 0), else lat_sweep_loop_kernel -- that mapping only, iters * 256 divides g.nquads and 2 * iters divides g.H
hipError_t lat_launch_sweep(bool vec, bool pmj, uint32_t iters, uint32_t n_replicas, unsigned lds_bytes, hipStream_t stream, uint32_t *state,
                            const LatGeom &g, uint32_t colour, uint64_t t, const uint2 *keys, const LatThr &thr, const LatThr *thr_replica,
                            const uint32_t *jneg, uint32_t jneg_uniform, int rounds = 10);
// workgroups of lat_sweep_loop_kernel<pmj, rounds> one compute unit holds at once with lds_bytes of LDS each; 0 when the query fails
int lat_sweep_loop_blocks_per_cu(bool pmj, unsigned lds_bytes, int rounds = 10);
// the colour-1 half-sweep fused with the measurement: out[r * out_stride + 2 slot] += satisfied bonds, MEASURE_SLOTS slots
hipError_t lat_launch_sweep_measure(bool vec, bool pmj, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t,
                                    const uint2 *keys, const LatThr &thr, const LatThr *thr_replica, const uint32_t *jneg,
                                    uint32_t jneg_uniform, unsigned long long *out, size_t out_stride, int rounds = 10);
// out[r * out_stride] += satisfied bonds, out[r * out_stride + 1] += up spins
hipError_t lat_launch_measure(bool vec, bool pmj, uint32_t n_replicas, hipStream_t stream, const uint32_t *state, const LatGeom &g,
                              const uint32_t *jneg, uint32_t jneg_uniform, unsigned long long *out, size_t out_stride);
// `timesteps` whole timesteps out of LDS, one workgroup of `threads` per replica; lds_bytes = the two planes
hipError_t lat_launch_resident(bool vec, bool pmj, unsigned n_replicas, unsigned threads, size_t lds_bytes, hipStream_t stream, uint32_t *state,
                               const LatGeom &g, uint64_t t0, uint32_t timesteps, const uint2 *keys, const LatThr *thr_steps,
                               uint32_t thr_stride, const LatThr *thr_replica, const uint32_t *jneg, uint32_t jneg_uniform,
                               unsigned long long *steps_out, int rounds = 10);

} // namespace isingmc
