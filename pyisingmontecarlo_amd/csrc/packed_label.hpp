// The labelling core that the replica-packed cluster kernels share (packed_cluster_kernels.hip, S12:
// packed_icm_kernels.hip, S13: packed_between_kernels.hip; the gather also serves S15's overlap_kernels.hip).  A workgroup of
// 256 threads covers 256 / LANES positions x LANES columns (replica bits, pairs or pair lanes): thread = (position-lane
// tid / LANES, column tid % LANES), and column c of position p of an item has its label and its size at [LANES p + c].  LANES
// is 32 or 16, so a wave holds 2 or 4 position-lanes.  Device code, inlined into the kernels that use it: every ballot and
// shuffle below is wave-wide and every barrier is reached by the whole workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "cluster_union.hpp"
#include "packed_cluster_kernels.hpp"

namespace isingmc {

constexpr int PKL_AGENT = __HIP_MEMORY_SCOPE_AGENT;

// per-column combination of the 256 / LANES position-lanes of a workgroup -> threads 0 .. LANES - 1 (0 in the others)
template <uint32_t LANES, typename OP>
__device__ __forceinline__ uint32_t pkl_reduce(uint32_t v, uint32_t (&red)[4][LANES], OP op)
{
#pragma unroll
    for (uint32_t sh = LANES; sh <= 32; sh *= 2) v = op(v, uint32_t(__shfl_xor(v, sh)));
    if ((threadIdx.x & 63u) < LANES) red[threadIdx.x >> 6][threadIdx.x & (LANES - 1)] = v;
    __syncthreads();
    return threadIdx.x < LANES ? op(op(red[0][threadIdx.x], red[1][threadIdx.x]), op(red[2][threadIdx.x], red[3][threadIdx.x])) : 0u;
}

// What a thread of a flip kernel counts while it visits the positions of its column one after another.  Positions per root:
// consecutive positions of one root (a large cluster) add up in a register before they go out.
template <uint32_t LANES>
struct PklCounts {
    uint32_t *sz; // this column's sizes: sz[LANES position]
    uint32_t n_roots = 0, n_members = 0, run_root = 0, run = 0;

    // position p belongs to the cluster of `root`
    __device__ __forceinline__ void account(uint32_t p, uint32_t root)
    {
        n_members++;
        n_roots += root == p;
        if (run && root != run_root) {
            atomicAdd(sz + size_t(LANES) * run_root, run);
            run = 0;
        }
        run_root = root;
        run++;
    }

    // the last run goes out; the position-lanes of a wave often end in the same root: one atomic for all of them
    __device__ __forceinline__ void flush()
    {
#pragma unroll
        for (uint32_t sh = LANES; sh <= 32; sh *= 2) {
            const uint32_t o_root = uint32_t(__shfl_xor(run_root, sh)), o_run = uint32_t(__shfl_xor(run, sh));
            if (run && o_run && o_root == run_root) run = (threadIdx.x & sh) ? 0 : run + o_run;
        }
        if (run) atomicAdd(sz + size_t(LANES) * run_root, run);
    }

    // the workgroup's roots per column -> stats[2 (LANES item + column)]
    __device__ __forceinline__ void finish(uint32_t (&red)[4][LANES], uint32_t item, uint32_t *stats) const
    {
        const uint32_t roots = pkl_reduce(n_roots, red, [](uint32_t a, uint32_t c) { return a + c; });
        if (threadIdx.x < LANES && roots) atomicAdd(stats + 2 * (LANES * size_t(item) + threadIdx.x), roots);
    }
    // ... and the accounted positions per column -> minus[LANES item + column]
    __device__ __forceinline__ void finish(uint32_t (&red)[4][LANES], uint32_t item, uint32_t *stats, uint32_t *minus) const
    {
        finish(red, item, stats);
        __syncthreads(); // red is reused
        const uint32_t total = pkl_reduce(n_members, red, [](uint32_t a, uint32_t c) { return a + c; });
        if (threadIdx.x < LANES && total) atomicAdd(minus + LANES * size_t(item) + threadIdx.x, total);
    }
};

// Every bond that position p owns (neighbour position above the own) and whose other end q passes `joins` hooks the larger root
// below the smaller.  lab: this column's labels, lab[LANES position].
template <uint32_t LANES, typename NBR, typename JOINS>
__device__ __forceinline__ void pkl_unite_owned(uint32_t *lab, const NBR &nbr, uint32_t p, JOINS joins)
{
    const uint32_t n_slots = nbr.slots();
    for (uint32_t k = 0; k < n_slots; k++) {
        const uint32_t q = nbr(k, p);
        if (q <= p) continue; // the end with the smaller position owns the bond
        if (joins(q)) cl_unite<PKL_AGENT, LANES>(lab, p, q);
    }
}

// Largest cluster: stats[2 (LANES g + column) + 1] = max over p of sizes[g][p][column]; entries whose maximum is 0 are not written.
// grid: (min(n_pos LANES / 256, 1024), n)
template <uint32_t LANES>
__global__ __launch_bounds__(256) void pkl_max_kernel(const uint32_t n_pos, const uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t red[4][LANES];
    const uint32_t g = blockIdx.y, c = threadIdx.x & (LANES - 1), pl = threadIdx.x / LANES;
    const uint32_t *sz = sizes + size_t(g) * n_pos * LANES + c;
    uint32_t m = 0;
    for (uint32_t p = blockIdx.x * (256 / LANES) + pl; p < n_pos; p += gridDim.x * (256 / LANES)) m = max(m, sz[size_t(LANES) * p]);
    const uint32_t total = pkl_reduce(m, red, [](uint32_t a, uint32_t b) { return max(a, b); });
    if (threadIdx.x < LANES && total) atomicMax(stats + 2 * (LANES * size_t(g) + threadIdx.x) + 1, total);
}

// pkl_max_kernel with the cluster-size moments of DESIGN.md S24, launched in its place while a cluster series is live: the same
// grid and the same walk over sizes[g][p][column].  The flip kernels count real positions (d = 1 positions) alone and the init
// kernels clear every entry, so padding positions and the columns of pairs that do not move read 0 and add nothing; a column
// whose counter slot out.slot0 + LANES g + c lies outside the row -- a bit the shard does not own -- is summed and dropped.
// Each thread holds S2 in 64 bits and S4 in 128 (cluster_moments.hpp); the position-lanes of a wave add up by shuffles and the
// wave's first LANES lanes add into their columns.  Bounded by the read of `sizes`, as the kernel it replaces.
template <uint32_t LANES>
__global__ __launch_bounds__(256) void pkl_max_moments_kernel(const uint32_t n_pos, const uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats,
                                                              const ClusterMomentsOut out)
{
    __shared__ uint32_t red[4][LANES];
    const uint32_t g = blockIdx.y, c = threadIdx.x & (LANES - 1), pl = threadIdx.x / LANES;
    const uint32_t *sz = sizes + size_t(g) * n_pos * LANES + c;
    uint32_t m = 0;
    ClusterMoments sum;
    for (uint32_t p = blockIdx.x * (256 / LANES) + pl; p < n_pos; p += gridDim.x * (256 / LANES)) {
        const uint32_t s = sz[size_t(LANES) * p];
        if (s) { // (most positions are no roots)
            m = max(m, s);
            sum.add_size(s);
        }
    }
#pragma unroll
    for (uint32_t sh = LANES; sh <= 32; sh *= 2) sum.add_lane_xor(int(sh));
    const uint32_t col = out.slot0 + LANES * g + c - out.first_slot;
    if ((threadIdx.x & 63u) < LANES && col < out.n_cols) sum.add_to(out.row + size_t(CLS_ROW) * col);
    const uint32_t total = pkl_reduce(m, red, [](uint32_t a, uint32_t b) { return max(a, b); });
    if (threadIdx.x < LANES && total) atomicMax(stats + 2 * (LANES * size_t(g) + threadIdx.x) + 1, total);
}

// the last launch of a step on the packed layouts: pkl_max_kernel, or its moments form while a series is live (out.row)
template <uint32_t LANES>
inline void pkl_launch_max(hipStream_t stream, uint32_t n_pos, const uint32_t *sizes, uint32_t n, uint32_t *stats, const ClusterMomentsOut &out)
{
    const dim3 grid(n_pos / (256 / LANES) < 1024u ? n_pos / (256 / LANES) : 1024u, n);
    if (out.row) hipLaunchKernelGGL(pkl_max_moments_kernel<LANES>, grid, dim3(256), 0, stream, n_pos, sizes, stats, out);
    else hipLaunchKernelGGL(pkl_max_kernel<LANES>, grid, dim3(256), 0, stream, n_pos, sizes, stats);
}

// The overlap word of a pair block, in a grid of (n_pos / 8, n_blocks) with 32 pair lanes: bit i of d[B][p] is set where the two
// replicas of pair pair0 + 32 B + i -- slot a.slots[pair] of a, slot b.slots[pair] of b -- differ at position p; 0 on padding
// and on empty lanes.
__device__ __forceinline__ void pkl_gather_word(const PkSide &a, const PkSide &b, const uint32_t n_pos, const uint32_t *__restrict__ site,
                                                const uint32_t pair0, const uint32_t n_pairs, uint32_t *__restrict__ d)
{
    const uint32_t B = blockIdx.y, i = threadIdx.x & 31u, pl = threadIdx.x >> 5, p = blockIdx.x * 8 + pl;
    const uint32_t n = pair0 + 32 * B + i;
    uint32_t x = 0;
    if (n < n_pairs && site[p] != PAD_SITE) {
        const uint32_t sa = a.slots[n], sb = b.slots[n];
        if (sa < a.n_slots && sb < b.n_slots) {
            const uint32_t ca = a.bit0 + sa, cb = b.bit0 + sb;
            x = ((a.state[size_t(ca >> 5) * n_pos + p] >> (ca & 31u)) ^ (b.state[size_t(cb >> 5) * n_pos + p] >> (cb & 31u))) & 1u;
        }
    }
    const uint64_t differ = __ballot(x != 0); // lanes 0..31: this wave's even position-lane, 32..63: the odd one
    if (i == 0) d[size_t(B) * n_pos + p] = uint32_t(differ >> (32 * (pl & 1u)));
}

} // namespace isingmc
