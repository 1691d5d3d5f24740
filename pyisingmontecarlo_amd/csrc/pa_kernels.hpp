// Population annealing: the resampling step on the device.  Launch interface of pa_kernels.hip (a translation
// unit of its own: nothing here is instantiated beside the tuned sweep kernels).
//
// One resampling = five stages behind the energy measurement on the container's stream (about ten short launches in all: the
// scan is three, the gather two, the measurement up to three), no host synchronisation:
//   weights   E[R] -> W[R] (u64, 2^32 fixed point of det_exp), the step record (sum, reference energy, mean energy, offset u)
//   scan      inclusive prefix sum of W in place (three passes: blocks of 1024, the block sums, the offsets)
//   sources   src[j] = the replica whose interval of the prefix sum holds j S + u (binary search, 128-bit compare)
//   gather    configurations (rows of a checkerboard container, bits of a replica-packed one) and the family table
// Both gathers write into a SECOND state buffer of the size of the state itself (the container keeps it from the first
// resampling on and swaps the two).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "general_types.hpp"

namespace isingmc {

constexpr uint32_t DOM_PA_RESAMPLE = 0x50415253u; // "PARS"
constexpr uint32_t PA_SCAN_BLOCK = 1024;          // elements per workgroup of the scan's first and third pass
constexpr uint64_t PA_MAX_REPLICAS = uint64_t(1) << 31;

// the record of one resampling, as the device leaves it
struct PaRecord {
    unsigned long long sum;      // S = sum of the weights
    double eref;                 // reference energy (min E for dbeta >= 0, else max E)
    unsigned long long distinct; // replicas with at least one copy
    double mean;                 // population mean energy before the resampling
    unsigned long long u;        // the offset in [0, S)
};

// The step chooser: the device record of one search.  Zero before the search (hipMemsetAsync); the accumulators
// are zero again behind every decision.
constexpr uint32_t PA_CHOOSE_CANDIDATES = 16; // per round
constexpr uint32_t PA_CHOOSE_ROUNDS = 4;
constexpr uint32_t PA_CHOOSE_GRID = 65536;    // the candidates are k / 65536 of dbeta_max, k = 1 .. 65536
struct PaChoose {
    unsigned long long sum[PA_CHOOSE_CANDIDATES];                                   // S of the round's candidates
    unsigned long long num_lo[PA_CHOOSE_CANDIDATES], num_hi[PA_CHOOSE_CANDIDATES]; // N of the round's candidates, 128 bits
    double dbeta[PA_CHOOSE_CANDIDATES];                                             // the round's candidates
    unsigned long long eref_key; // ~(the ordered key of min E): grown with atomicMax from zero
    uint32_t lo, width;          // the search: the answer is in (lo, lo + width), or lo
    uint32_t done;               // the first round held at all 16 candidates: k = 65536, the later rounds do nothing
    uint32_t k;                  // the result, behind the last decision: k, dbeta_k, S(k), N(k)
    double dbeta_k;
    unsigned long long sum_k, num_lo_k, num_hi_k;
};

constexpr size_t pa_scan_blocks(size_t R) { return (R + PA_SCAN_BLOCK - 1) / PA_SCAN_BLOCK; }

// energies[R] -> weights[R] and *rec (distinct = 0); one workgroup
hipError_t pa_launch_weights(hipStream_t stream, const double *energies, uint32_t R, double dbeta, uint64_t seed, uint64_t step,
                             unsigned long long *weights, PaRecord *rec);
// inclusive prefix sum of c[R] in place; block_sums: pa_scan_blocks(R) words of scratch
hipError_t pa_launch_scan(hipStream_t stream, unsigned long long *c, uint32_t R, unsigned long long *block_sums);
// src[j], j < R, from the prefix sums c[R] and rec->u; counts rec->distinct
hipError_t pa_launch_sources(hipStream_t stream, const unsigned long long *c, uint32_t R, PaRecord *rec, uint32_t *src);
// out[j] = in[src[j]]
hipError_t pa_launch_gather_u32(hipStream_t stream, const uint32_t *in, const uint32_t *src, uint32_t R, uint32_t *out);
// checkerboard containers: out[j][:] = in[src[j]][:], rows of state_words words
hipError_t pa_launch_row_gather(hipStream_t stream, const uint32_t *in, uint32_t *out, const uint32_t *src, size_t R, size_t state_words);
// replica-packed containers, u32[groups][n_pos]: bit s % 32 of group s / 32 of `out` = that of slot src[s] of `in` for s < R at
// the real positions; every other bit (slots >= R, padding positions: site[p] == PAD_SITE) is copied from its own place
hipError_t pa_launch_bit_gather(hipStream_t stream, const uint32_t *in, uint32_t *out, const uint32_t *src, uint32_t R, size_t groups,
                                uint32_t n_pos, const uint32_t *site);
// The whole search of the step chooser from energies[R], enqueue only: *rec is cleared, E_ref found, then four
// rounds of { sum pass, overlap pass, decision }: 15 stream-ordered launches, no workgroup waits for another one.
// unit = dbeta_max 2^-16; t32 = ceil(target 2^32) in 1 .. 2^32.  The result is in rec->k, dbeta_k, sum_k, num_lo_k, num_hi_k.
hipError_t pa_launch_choose(hipStream_t stream, const double *energies, uint32_t R, double unit, unsigned long long t32, PaChoose *rec);

} // namespace isingmc
