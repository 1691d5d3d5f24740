// Cluster-size moments of a non-local step: what the largest-cluster kernels of cluster_kernels.hip and
// packed_label.hpp share while a cluster series is live.  A row of the series holds CLS_ROW 64-bit entries per column:
//   n_clusters, largest, sites = sum s, S2 = sum s^2, S4_lo, S4_hi (S4 = sum s^4 = S4_hi 2^64 + S4_lo)
// over the cluster sizes s of the column's labelling problem.  With s <= N < 2^32: s^4 < 2^128, and since sum s <= N,
// S2 <= N^2 < 2^64 and S4 <= N^4 < 2^128: no partial sum overflows its width.  Integer additions only: the sums do not depend on
// the order of execution.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "sum128.hpp"

namespace isingmc {

constexpr uint32_t CLS_ROW = 6;
enum : uint32_t { CLS_N_CLUSTERS, CLS_LARGEST, CLS_SITES, CLS_S2, CLS_S4_LO, CLS_S4_HI };

// Where the moments of one batch go.  Column c of item g of the batch is counter slot slot0 + lanes g + c (lanes: 1 on a lattice,
// 32 / 16 on the packed layouts); the row's column 0 is counter slot first_slot, and slots outside [first_slot, first_slot +
// n_cols) -- the bits a packed shard does not own -- have no column: they add nothing.  row == nullptr: no series.
struct ClusterMomentsOut {
    unsigned long long *row = nullptr; // [n_cols][CLS_ROW], the moment entries zero before the step's first batch
    uint32_t slot0 = 0, first_slot = 0, n_cols = 0;
};

// the sums of one thread, then of one wave
struct ClusterMoments {
    unsigned long long s2 = 0;
    Sum128 s4;

    __device__ __forceinline__ void add_size(uint32_t s)
    {
        const unsigned long long q = (unsigned long long)s * s;
        s2 += q;
        s4.add(q * q, __umul64hi(q, q));
    }
    // this lane's sums + those of lane (lane ^ mask)
    __device__ __forceinline__ void add_lane_xor(int mask)
    {
        s2 += __shfl_xor(s2, mask);
        s4.add_lane_xor(mask);
    }
    // into the column at `col`: one 64-bit atomic per word (the carry of the low word of S4: Sum128::atomic_add_to)
    __device__ __forceinline__ void add_to(unsigned long long *col) const
    {
        if (!s2) return; // (no cluster among the sizes this sum saw)
        atomicAdd(col + CLS_S2, s2);
        s4.atomic_add_to(col + CLS_S4_LO, col + CLS_S4_HI);
    }
};

// Behind the last batch of a step: n_clusters, largest and sites of every column out of the step's 32-bit statistics.
// stats[slot][2] = {clusters, largest}; minus[slot] = the q = -1 sites of an isoenergetic move, or nullptr: sites = nvars.
hipError_t cluster_series_launch_store(hipStream_t stream, const uint32_t *stats, const uint32_t *minus, unsigned long long nvars,
                                       uint32_t first_slot, uint32_t n_cols, unsigned long long *row);

} // namespace isingmc
