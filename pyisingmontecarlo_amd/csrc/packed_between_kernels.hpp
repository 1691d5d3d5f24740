// Isoenergetic cluster move between two replica-packed containers of one family: pair n is slot slots_a[n] of
// container a and slot slots_b[n] of container b -- arbitrary bits of arbitrary words of two state arrays.  The work is organised
// in PAIR BLOCKS of 32 pairs (pair 32 B + i = bit i of block B), which gives the [block][position][32] label layout of S11.  Like
// S12 the move reads no coupling and no bias: one set of kernels, templated on the neighbour accessor (packed_nbr.hpp), serves both
// families.  Launch interface of packed_between_kernels.hip (a translation unit of its own: nothing here is instantiated beside the
// tuned sweep kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstddef>
#include <cstdint>

#include "packed_types.hpp"

namespace isingmc {

constexpr uint32_t DOM_PK_BETWEEN_FLIP = 0x504B4246u; // "PKBF"
constexpr uint32_t PKB_NO_PAIR = 0xFFFFFFFFu;

// workspace of one batch of n pair blocks (n_pos positions each)
struct PkBetweenWork {
    uint32_t *labels;  // [n][n_pos][32]       (position, pair lane) -> a smaller position of its cluster (the root: the smallest)
    uint32_t *sizes;   // [n][n_pos][32]       d = 1 positions per root
    uint32_t *d;       // [n][n_pos]           overlap words: bit i set where the two replicas of pair lane i differ
    uint32_t *f;       // [n][n_pos]           flip words: bit i set where pair lane i swaps its two spins
    uint32_t *fliptab; // [n][32][n_pos / 32]  one flip bit per (pair lane, possible root position)
};

// Words per block of {labels, sizes, d, f, fliptab}.  The members lie in this order, one behind the other, in the block of a batch: its
// size (pk_between_words_per_block) and its carving (pk_between_carve) both follow from this one line.
constexpr std::array<size_t, 5> pk_between_member_words(uint64_t n_pos) { return {{size_t(32 * n_pos), size_t(32 * n_pos), size_t(n_pos), size_t(n_pos), size_t(n_pos)}}; }
constexpr size_t pk_between_words_per_block(uint64_t n_pos) { const std::array<size_t, 5> w = pk_between_member_words(n_pos); return w[0] + w[1] + w[2] + w[3] + w[4]; }
static_assert(pk_between_words_per_block(256) == 67 * 256, "labels 32 n_pos | sizes 32 n_pos | d n_pos | f n_pos | fliptab n_pos");

// the workspace of `batch` pair blocks in a block of batch * pk_between_words_per_block(n_pos) words
static inline PkBetweenWork pk_between_carve(uint32_t *block, size_t batch, uint64_t n_pos)
{
    const std::array<size_t, 5> w = pk_between_member_words(n_pos);
    uint32_t *const sizes = block + batch * w[0], *const d = sizes + batch * w[1], *const f = d + batch * w[2], *const fliptab = f + batch * w[3];
    return PkBetweenWork{block, sizes, d, f, fliptab};
}

// one of the two containers as the kernels see it: PkSide (packed_types.hpp) and what the move writes back through
struct PkBetweenSide : PkSide {
    uint32_t *inv;         // [groups][32] pair of every (local group, bit), PKB_NO_PAIR where none (pk_between_launch_tables)
    uint32_t groups;
};

// the bit -> pair tables of both sides, once per move
hipError_t pk_between_launch_tables(hipStream_t stream, const PkBetweenSide &a, const PkBetweenSide &b, uint32_t n_pairs);

// Pair blocks [block0, block0 + n_blocks) of a move of n_pairs pairs at timestep t.  nbr_rj == nullptr: the neighbours of
// G.nbr_ell (PK_MAX_DEG slots); else nbr_rj[slot][n_pos] with rj_slots slots.  a_keys: the group keys of a's local groups.
// stats: [n_pairs][2] = {clusters, largest cluster}, minus: [n_pairs] = positions where the pair differs; zero on entry.
// n_blocks <= 32768.
hipError_t pk_between_launch_batch(hipStream_t stream, const PkBetweenSide &a, const PkBetweenSide &b, const PkGraphDev &G, const uint32_t *nbr_rj,
                                   uint32_t rj_slots, uint64_t t, const uint2 *a_keys, const PkBetweenWork &work, uint32_t block0, uint32_t n_blocks,
                                   uint32_t n_pairs, uint32_t *stats, uint32_t *minus);

} // namespace isingmc
