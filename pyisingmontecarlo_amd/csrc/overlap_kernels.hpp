// Spin and link overlaps between two replicas of one graph: exact integer counts on the configurations as they are.
// For a pair (a, b) with d_i = s_i^a xor s_i^b the kernels count
//   D = sites with d_i = 1                                  (spin overlap  = nvars   - 2 D)
//   B = bonds whose two ends have unequal d                 (link overlap  = n_edges - 2 B)
// into 64-bit accumulators out[pair][2] = {D, B}, ZERO on entry.  No coupling, bias or random number is read and no state word is
// written.  A bond is an entry of the edge list given at graph creation: zero couplings count, duplicated entries count once each;
// an entry a_e == b_e is in no adjacency (host_logic.cpp build_adjacency drops it) and never adds to B -- its term of the link
// overlap is +1 whatever the spins, which n_edges - 2 B states.
// Launch interface of overlap_kernels.hip (a translation unit of its own: nothing here is instantiated beside the tuned sweep
// kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "packed_types.hpp"

namespace isingmc {

// ---- shared with overlap_class_kernels.hip --------------------------------------------------------------------
constexpr uint32_t OVL_PK_ITER = 4; // positions per thread of the packed counting kernels (a workgroup covers 1024 positions)
constexpr int OVL_D_PLANES = 3;     // counts up to OVL_PK_ITER per thread and column

// c += x in every bit column (c: the planes of a bit-sliced counter, least significant first)
template <int N>
__device__ __forceinline__ void ovl_csa_add(uint32_t (&c)[N], uint32_t x)
{
#pragma unroll
    for (int b = 0; b < N; b++) {
        const uint32_t carry = c[b] & x;
        c[b] ^= x;
        x = carry;
    }
}

// the wave's total of bit column `bit` of a bit-sliced counter (wave-uniform)
template <int N>
__device__ __forceinline__ uint32_t ovl_column_total(const uint32_t (&c)[N], uint32_t bit)
{
    uint32_t total = 0;
#pragma unroll
    for (int b = 0; b < N; b++) total += uint32_t(__popcll(__ballot((c[b] >> bit) & 1u))) << b;
    return total;
}

// Checkerboard path (state u32[R][2 wpp]).  slots_a == nullptr: pair p = replicas (2 p, 2 p + 1) of state_a (state_b is not read);
// else pair p = replica slots_a[p] of state_a and replica slots_b[p] of state_b (device tables; the two arrays may be one).
// link = false: D alone, out[2 p + 1] stays zero.
hipError_t overlap_launch_lattice(hipStream_t stream, const uint32_t *state_a, const uint32_t *state_b, const uint32_t *slots_a,
                                  const uint32_t *slots_b, const LatGeom &g, bool link, size_t n_pairs, unsigned long long *out);

// Replica-packed paths (state u32[groups][n_pos], a replica is a bit).  nbr_rj == nullptr: the neighbours of G.nbr_ell (PK_MAX_DEG
// slots, the bit-sliced family); else nbr_rj[slot][n_pos] with rj_slots <= 31 slots (the real-coupling family).
// Default pairing: pair j of group g = bits (2 j, 2 j + 1) of every state word; out[16 g + j] for ALL 16 pairs of every group (the
// caller picks the pairs that exist).  No workspace.
hipError_t overlap_launch_packed_pairs(hipStream_t stream, const uint32_t *state, const PkGraphDev &G, const uint32_t *nbr_rj,
                                       uint32_t rj_slots, bool link, size_t groups, unsigned long long *out);

// The arbitrary-pair form takes its two containers as PkSide (packed_types.hpp; the two may be the same container).
// The gather alone (DESIGN.md S17 counts its words by class): d[n_blocks][n_pos] as below
hipError_t overlap_launch_packed_gather(hipStream_t stream, const PkSide &a, const PkSide &b, const PkGraphDev &G, uint32_t block0,
                                        uint32_t n_blocks, uint32_t n_pairs, uint32_t *d);

// Arbitrary pairs: pair blocks [block0, block0 + n_blocks) of 32 pairs each (pair 32 B + i = bit i of block B) are gathered into
// the overlap words d[n_blocks][n_pos] (bit i set where pair i differs; 0 on padding and on empty lanes) and counted into
// out[32 block0 ...].  n_blocks <= 32768.
hipError_t overlap_launch_packed_tables(hipStream_t stream, const PkSide &a, const PkSide &b, const PkGraphDev &G,
                                        const uint32_t *nbr_rj, uint32_t rj_slots, bool link, uint32_t block0, uint32_t n_blocks,
                                        uint32_t n_pairs, uint32_t *d, unsigned long long *out);

} // namespace isingmc
