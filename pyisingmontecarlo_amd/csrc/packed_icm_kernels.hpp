// Isoenergetic cluster move on the replica-packed paths: experiments (2 j, 2 j + 1) of a replica group are bits
// (2 j, 2 j + 1) of the same state word, so a group holds 16 pairs.  The move reads no coupling and no bias: one set of kernels,
// templated on the neighbour accessor, serves the bit-sliced family (PkGraphDev::nbr_ell) and the real-coupling family
// (RjGraphDev::nbr).  Launch interface of packed_icm_kernels.hip (a translation unit of its own: nothing here is instantiated
// beside the tuned sweep kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstddef>
#include <cstdint>

#include "cluster_moments.hpp"
#include "packed_types.hpp"
#include "real_types.hpp"

namespace isingmc {

constexpr uint32_t DOM_PK_ICM_FLIP = 0x504B4946u; // "PKIF"

// workspace of one batch of n replica groups (n_pos positions each)
struct PkIcmWork {
    uint32_t *labels;  // [n][n_pos][16]  (position, pair) -> a smaller position of its cluster (the root: the smallest)
    uint32_t *sizes;   // [n][n_pos][16]  d = 1 positions per root
    uint32_t *fliptab; // [n][n_pos / 2]  16 flip bits per possible root position: position r = half r & 1 of word r >> 1
};

// Words per group of {labels, sizes, fliptab}.  The members lie in this order, one behind the other, in the block of a batch: its
// size (pk_icm_words_per_group) and its carving (pk_icm_carve) both follow from this one line.
constexpr std::array<size_t, 3> pk_icm_member_words(uint64_t n_pos) { return {{size_t(16 * n_pos), size_t(16 * n_pos), size_t(n_pos / 2)}}; }
constexpr size_t pk_icm_words_per_group(uint64_t n_pos) { const std::array<size_t, 3> w = pk_icm_member_words(n_pos); return w[0] + w[1] + w[2]; }
static_assert(pk_icm_words_per_group(256) == 32 * 256 + 128, "labels 16 n_pos | sizes 16 n_pos | fliptab n_pos / 2");

// the workspace of `batch` groups in a block of batch * pk_icm_words_per_group(n_pos) words
static inline PkIcmWork pk_icm_carve(uint32_t *block, size_t batch, uint64_t n_pos)
{
    const std::array<size_t, 3> w = pk_icm_member_words(n_pos);
    uint32_t *const sizes = block + batch * w[0], *const fliptab = sizes + batch * w[1];
    return PkIcmWork{block, sizes, fliptab};
}

// One move of groups [0, n) at timestep t: state / group_keys / move_mask / stats / minus point at the first group of the batch.
// move_mask[g]: bit 2 j set when pair j of group g moves.  nbr_rj == nullptr: the neighbours of G.nbr_ell (PK_MAX_DEG slots);
// else nbr_rj[slot][n_pos] with rj_slots slots (the own position in unused slots).  `site` marks the padding (PAD_SITE).
// stats: [16 n][2] = {clusters, largest cluster}, minus: [16 n] = positions where the pair differs, per (group, pair); zero on
// entry.  n <= 32768.  moments: with a row, the last launch also adds the cluster-size moments of pair j of group g into the column
// of pair slot slot0 + 16 g + j (cluster_moments.hpp).
hipError_t pk_icm_launch_step(hipStream_t stream, uint32_t *state, const PkGraphDev &G, const uint32_t *nbr_rj, uint32_t rj_slots, uint64_t t,
                              const uint2 *group_keys, const uint32_t *move_mask, const PkIcmWork &work, uint32_t n, uint32_t *stats,
                              uint32_t *minus, const ClusterMomentsOut &moments = {});

} // namespace isingmc
