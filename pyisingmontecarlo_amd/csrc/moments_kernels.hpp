// Per-site spin sums and per-bond agreement sums over the samples of a run: exact integer counts on the
// configurations as they are.  No coupling, bias or random number is read and no state word is written.  Every total counts SET
// BITS -- up spins, or bonds whose two ends agree; the host turns a count c of n samples into the sum of +-1 terms, 2 c - n.
// No kernel uses an atomic: every total has one owning thread.
// Launch interface of moments_kernels.hip (a translation unit of its own: nothing here is instantiated beside the sweep kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "packed_types.hpp"

namespace isingmc {

constexpr int MOM_REG_PLANES = 8;                             // register planes of the summed checkerboard kernel:
constexpr uint32_t MOM_REG_CHUNK = (1u << MOM_REG_PLANES) - 1; // replicas added before the planes are expanded into the totals
constexpr int MOM_MAX_TIME_PLANES = 16;                       // the option moments_planes is 1 .. 16

// ---- summed over the replicas ---------------------------------------------------------------------------------------------------
// Checkerboard path (state u32[R][2 wpp]): totals u64[kinds][32][2 wpp], totals[(kind 32 + b) 2 wpp + w] += over the replicas bit b of
//   kind 0: the state word w itself (site sums)
//   kind 1: the agreement of w's sites with their right neighbours, ~(s ^ right)      (bond sums, with_bonds)
//   kind 2: ... with the neighbours below them, ~(s ^ down)
// w = plane wpp + y wpr + k; bit b of it is the site x = 2 (32 k + b) + ((plane + y) & 1) of row y.  Periodic in both directions.
hipError_t moments_launch_lattice_sum(hipStream_t stream, const uint32_t *state, const LatGeom &g, size_t n_replicas, bool with_bonds,
                                      unsigned long long *totals);

// Replica-packed paths (state u32[groups][n_pos], replica slot s = bit s & 31 of group s >> 5): the container owns the slots
// [bit0, bit0 + n_owned).  site_totals[p] += popcount of position p's words under the owned masks, padding positions included (the
// host reads none of them); bond_totals[e] += popcount of ~(word(edges[e].x) ^ word(edges[e].y)) under the masks, edges[n_edges] =
// the two positions of every edge-list entry (an entry with both ends on one site counts every owned replica).  n_edges == 0: sites only.
hipError_t moments_launch_packed_sum(hipStream_t stream, const uint32_t *state, uint32_t n_pos, size_t groups, uint32_t bit0, uint32_t n_owned,
                                     unsigned long long *site_totals, const uint2 *edges, size_t n_edges, unsigned long long *bond_totals);

// ---- per replica, both layouts: the state's own words counted over time -----------------------------------------------------------
// one sample: planes u32[k][n_words] (a vertical counter per state bit) += state u32[n_words]; at most 2^k - 1 samples between flushes
hipError_t moments_launch_add(hipStream_t stream, const uint32_t *state, size_t n_words, int k, uint32_t *planes);
// flush: totals u32[n_rows][32][row_words] += the counters of planes u32[k][n_rows row_words], which are cleared: bit b of word w of row r
// goes to totals[(32 r + b) row_words + w].  Checkerboard: a row is a replica; packed: a row is a group, 32 r + b its replica slots.
hipError_t moments_launch_flush(hipStream_t stream, uint32_t *planes, size_t n_rows, size_t row_words, int k, uint32_t *totals);

// ---- per rung of a tempering ladder: the same planes and totals, their rows rungs instead of slots ------------------
// perm u32[n_rungs] (device): rung -> the slot that holds it, read by the kernel where the exchange rounds leave it.
// Checkerboard path: planes u32[k][n_rungs row_words], row i += state row perm[i] (state u32[n_rungs][row_words]).
hipError_t moments_launch_add_by_rung(hipStream_t stream, const uint32_t *state, const uint32_t *perm, size_t n_rungs, size_t row_words, int k,
                                      uint32_t *planes);
// Packed paths: planes u32[k][n_words] of which the first ceil(n_rungs / 32) n_pos words are used; bit b of destination word (G, p) +=
// bit q & 31 of state word (q >> 5, p), q = bit0 + perm[32 G + b]; rungs from n_rungs on add nothing.  The state must hold the groups
// up to (bit0 + n_rungs - 1) >> 5.  Padding positions are counted like any other; the host reads none of them.
hipError_t moments_launch_packed_add_by_rung(hipStream_t stream, const uint32_t *state, const uint32_t *perm, size_t n_rungs, uint32_t n_pos,
                                             uint32_t bit0, size_t n_words, int k, uint32_t *planes);

} // namespace isingmc
