// Launchers of the general edge-list kernels (general_kernels.hip; the kernels are in general_kernels.hpp).
// w_is_float: the couplings G.w are float (else double); n_replicas replicas, whose state words, keys and beta_replica entries
// (nullptr: one beta for all) begin at the pointers passed.
#pragma once
#include <hip/hip_runtime.h>

#include "general_types.hpp"

namespace isingmc {

#ifndef ISINGMC_GEN_RB
#define ISINGMC_GEN_RB 8
#endif
constexpr int GEN_RB = ISINGMC_GEN_RB; // most replicas per thread of gen_sweep_kernel (amortises the CSR stream)
static_assert(GEN_RB == 1 || GEN_RB == 2 || GEN_RB == 4 || GEN_RB == 8, "gen_sweep_kernel is instantiated for 1, 2, 4 and 8 replicas per thread");

hipError_t gen_launch_init(hipStream_t stream, uint32_t *state, const GenGraphDev &G, const uint2 *keys, uint32_t first_replica, uint32_t n_replicas);
// one colour class [class_begin, class_end) of one timestep; rb = 1, 2, 4 or 8 replicas per thread: grid.y = ceil(n_replicas / rb)
hipError_t gen_launch_sweep(bool w_is_float, int rb, uint32_t n_replicas, hipStream_t stream, uint32_t *state, const GenGraphDev &G,
                            uint32_t class_begin, uint32_t class_end, uint64_t t, const uint2 *keys, double beta, const double *beta_replica);
// partial_e / partial_m[r][n_partials], n_partials = ceil(G.n_pos / 256): per-block sums of E and M ...
hipError_t gen_launch_measure(bool w_is_float, uint32_t n_replicas, uint32_t n_partials, hipStream_t stream, const uint32_t *state,
                              const GenGraphDev &G, double *partial_e, long long *partial_m);
// ... and their fixed-order tree sums out_e[r], out_m[r]
hipError_t gen_launch_reduce(hipStream_t stream, const double *partial_e, const long long *partial_m, uint32_t n_partials, uint32_t n_replicas,
                             double *out_e, long long *out_m);
// `timesteps` whole timesteps out of LDS, one workgroup of `threads` per replica.  stage: 0 = the state words alone in LDS,
// 1 / 2 = the graph / its topology too (gen_stage_words); lds_bytes beyond the default limit of dynamic LDS are asked for here
hipError_t gen_launch_resident(bool w_is_float, int stage, unsigned n_replicas, unsigned threads, size_t lds_bytes, hipStream_t stream,
                               uint32_t *state, const GenGraphDev &G, uint64_t t0, uint32_t timesteps, const uint2 *keys,
                               const double *beta_steps, uint32_t beta_stride, const double *beta_replica, double *energies_out,
                               double self_energy, uint32_t edges2);

} // namespace isingmc
