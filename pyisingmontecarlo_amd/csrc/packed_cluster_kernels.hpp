// Swendsen-Wang cluster step on the replica-packed bit-sliced path: any graph the S6 path serves (one |J|, no
// fields, degree <= 6, any sign pattern).  Launch interface of packed_cluster_kernels.hip (a translation unit of its own:
// nothing here is instantiated beside the tuned sweep kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstddef>
#include <cstdint>

#include "cluster_moments.hpp"
#include "packed_types.hpp"

namespace isingmc {

constexpr uint32_t DOM_PK_CL_BOND = 0x504B4244u; // "PKBD"
constexpr uint32_t DOM_PK_CL_FLIP = 0x504B464Cu; // "PKFL"

// workspace of one batch of n replica groups (n_pos positions each)
struct PkClusterWork {
    uint32_t *labels;  // [n][n_pos][32]         (position, replica bit) -> a smaller position of its cluster (the root: the smallest)
    uint32_t *sizes;   // [n][n_pos][32]         positions per root
    uint32_t *bonds;   // [n][PK_MAX_DEG][n_pos] active bonds of the 32 replicas, by (adjacency slot, owner position); 0 where not owned
    uint32_t *fliptab; // [n][n_pos]             flip bits of the 32 replicas for every possible root
};

// Words per group of {labels, sizes, bonds, fliptab}.  The members lie in this order, one behind the other, in the block of a batch: its
// size (pk_cluster_words_per_group) and its carving (pk_cluster_carve) both follow from this one line.
constexpr std::array<size_t, 4> pk_cluster_member_words(uint64_t n_pos) { return {{size_t(32 * n_pos), size_t(32 * n_pos), size_t(PK_MAX_DEG * n_pos), size_t(n_pos)}}; }
constexpr size_t pk_cluster_words_per_group(uint64_t n_pos) { const std::array<size_t, 4> w = pk_cluster_member_words(n_pos); return w[0] + w[1] + w[2] + w[3]; }
static_assert(pk_cluster_words_per_group(256) == (64 + PK_MAX_DEG + 1) * 256, "labels 32 n_pos | sizes 32 n_pos | bonds PK_MAX_DEG n_pos | fliptab n_pos");

// the workspace of `batch` groups in a block of batch * pk_cluster_words_per_group(n_pos) words
static inline PkClusterWork pk_cluster_carve(uint32_t *block, size_t batch, uint64_t n_pos)
{
    const std::array<size_t, 4> w = pk_cluster_member_words(n_pos);
    uint32_t *const sizes = block + batch * w[0], *const bonds = sizes + batch * w[1], *const fliptab = bonds + batch * w[2];
    return PkClusterWork{block, sizes, bonds, fliptab};
}

// One cluster step of groups [0, n) at timestep t: state / group_keys / thr_per_slot / stats point at the first group of the
// batch.  thr_per_slot == nullptr: every replica uses thr; else thr_per_slot[32 g + b].  stats: [32 n][2] = {clusters, largest
// cluster} per (group, replica bit), zero on entry.  n <= 32768.  moments: with a row, the last launch also adds the cluster-size
// moments of bit b of group g into the column of counter slot slot0 + 32 g + b (cluster_moments.hpp).
hipError_t pk_cluster_launch_step(hipStream_t stream, uint32_t *state, const PkGraphDev &G, uint64_t t, const uint2 *group_keys, uint64_t thr,
                                  const uint64_t *thr_per_slot, const PkClusterWork &work, uint32_t n, uint32_t *stats,
                                  const ClusterMomentsOut &moments = {});

// The last launch of the step on its own, for any sizes[n][n_pos][32] (S13's pair blocks have this layout): stats[2 (32 g + b) + 1]
// = max over p of sizes[g][p][b]; entries whose maximum is 0 are not written.
hipError_t pk_cluster_launch_max(hipStream_t stream, uint32_t n_pos, const uint32_t *sizes, uint32_t n, uint32_t *stats);

} // namespace isingmc
