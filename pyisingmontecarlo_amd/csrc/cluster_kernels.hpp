// Swendsen-Wang cluster step for periodic, field-free checkerboard lattices with one |J| and one coupling
// sign, and the isoenergetic cluster move between replica pairs (S9, any sign pattern) on the same labelling: launch
// interface of cluster_kernels.hip (a translation unit of its own: nothing here is instantiated beside the tuned sweep
// kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstddef>
#include <cstdint>

#include "cluster_moments.hpp"
#include "lattice_types.hpp"

namespace isingmc {

constexpr uint32_t DOM_SW_BOND = 0x53574244u; // "SWBD"
constexpr uint32_t DOM_SW_FLIP = 0x5357464Cu; // "SWFL"
constexpr uint32_t DOM_ICM_FLIP = 0x4943464Cu; // "ICFL"

constexpr uint32_t CL_TILE_W = 64;    // sites: the 32 spins of one word of plane 0 interleaved with the 32 of plane 1
constexpr uint32_t CL_TILE_ROWS = 32; // rows of a tile (the last tile row of a lattice may be shorter)

// workspace of one batch of n replicas (N = W H sites, wpp = N / 64 words per plane)
struct ClusterWork {
    uint32_t *labels;  // [n][N]       site -> a smaller site of its cluster (the root: the smallest)
    uint32_t *sizes;   // [n][N]       sites per root
    uint32_t *bonds;   // [n][2][2][wpp] active bonds, [direction][plane][word] in the layout of the spins
    uint32_t *fliptab; // [n][N / 32]  flip bit of every possible root
};

// Words per replica of {labels, sizes, bonds, fliptab}.  The members lie in this order, one behind the other, in the block of a batch: its
// size (cluster_words_per_replica) and its carving (cluster_carve) both follow from this one line.
constexpr std::array<size_t, 4> cluster_member_words(uint64_t nvars) { return {{size_t(nvars), size_t(nvars), size_t(nvars / 16), size_t(nvars / 32)}}; }
constexpr size_t cluster_words_per_replica(uint64_t nvars) { const std::array<size_t, 4> w = cluster_member_words(nvars); return w[0] + w[1] + w[2] + w[3]; }
static_assert(cluster_words_per_replica(4096) == 2 * 4096 + 256 + 128, "labels N | sizes N | bonds N / 16 | fliptab N / 32");

// the workspace of `batch` replicas in a block of batch * cluster_words_per_replica(nvars) words
static inline ClusterWork cluster_carve(uint32_t *block, size_t batch, uint64_t nvars)
{
    const std::array<size_t, 4> w = cluster_member_words(nvars);
    uint32_t *const sizes = block + batch * w[0], *const bonds = sizes + batch * w[1], *const fliptab = bonds + batch * w[2];
    return ClusterWork{block, sizes, bonds, fliptab};
}

// One cluster step of replicas [0, n) at timestep t: state / keys / thr_per_replica / stats point at the first replica of the
// batch.  thr_per_replica == nullptr: every replica uses thr.  stats: [n][2] = {clusters, largest cluster}, zero on entry.
// moments: with a row, the last launch also adds the cluster-size moments of replica r into column slot0 + r (cluster_moments.hpp).
hipError_t cluster_launch_step(hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t, const uint2 *keys, uint32_t jneg_uniform,
                               uint64_t thr, const uint64_t *thr_per_replica, const ClusterWork &work, uint32_t n, uint32_t *stats,
                               const ClusterMomentsOut &moments = {});

// One isoenergetic cluster move of pairs [0, n_pairs) at timestep t: pair p = replicas 2 p and 2 p + 1 behind
// `state` / `keys` (the key of replica 2 p draws the flip bits); the workspace holds n_pairs labelling problems.
// stats: [n_pairs][2] = {q = -1 clusters, largest one} in the layout cl_max_kernel writes; minus_sites: [n_pairs] q = -1 sites;
// both zero on entry.  moments: as above, pair p into column slot0 + p.
hipError_t icm_launch_step(hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t, const uint2 *keys, const ClusterWork &work,
                           uint32_t n_pairs, uint32_t *stats, uint32_t *minus_sites, const ClusterMomentsOut &moments = {});

// The same move between two containers: pair p = replica slots_a[p] behind state_a and replica slots_b[p] behind
// state_b, both tables in DEVICE memory ([n_pairs], every slot at most once); keys_a: the keys of state_a's replicas from slot 0
// on (the key of slots_a[p] draws the flip bits).  stats / minus_sites as above.
hipError_t icm_between_launch_step(hipStream_t stream, uint32_t *state_a, uint32_t *state_b, const uint32_t *slots_a, const uint32_t *slots_b,
                                   const LatGeom &g, uint64_t t, const uint2 *keys_a, const ClusterWork &work, uint32_t n_pairs, uint32_t *stats,
                                   uint32_t *minus_sites);

} // namespace isingmc
