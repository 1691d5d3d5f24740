// Isoenergetic cluster move between the experiment pairs of a replica group: four plain stream-ordered launches
// per batch of replica groups.  Pair j of a group is bits (2 j, 2 j + 1) of every state word: the pair differs at position p
// where bit 2 j of d[p] = (w[p] ^ (w[p] >> 1)) & 0x55555555 & move_mask is set (d = 0 on padding).  The clusters are the connected
// components of the d = 1 positions along the stored adjacency; a flipped cluster swaps the two replicas' spins on it.
//   pki_init_kernel    one thread per (position, pair): label = own position, size = 0; the first n_pos / 8 threads also write the
//                      flip table (one Philox call = the 16-bit entries of eight positions)
//   pki_union_kernel   one thread per (position, pair): every owned bond (neighbour position above the own) whose two ends both
//                      have d = 1 hooks the larger root below the smaller; no bonds array, d is recomputed from the state words
//   pki_flip_kernel    one thread per (position-lane, pair), eight positions after one another: d = 1 lanes chase to the root and
//                      look the flip bit up, ballot -> one lane XORs both bits of every flipped pair into the state word; counts
//                      the d = 1 positions, the roots and the positions per root
//   pki_max_kernel     largest cluster
// Labels are laid out [group][position][pair]: a wave covers four consecutive positions x 16 pairs, so the first hop of a chase
// is one coalesced 64-byte row per position.  No kernel waits for another workgroup; every loop walks strictly decreasing
// labels (cluster_union.hpp).
#include "packed_icm_kernels.hpp"

#include <algorithm>

#include "cluster_union.hpp"
#include "packed_cluster_kernels.hpp"
#include "packed_nbr.hpp"
#include "philox.hpp"

namespace isingmc {

namespace {

constexpr uint32_t PKI_FLIP_POS = 128;         // positions per workgroup of pki_flip_kernel (n_pos is a multiple of 256)
constexpr int AGENT = __HIP_MEMORY_SCOPE_AGENT;

// per-pair combination of the 16 position-lanes of a workgroup (lane & 15 = pair) -> threads 0..15
template <typename OP>
__device__ __forceinline__ uint32_t pki_reduce_pairs(uint32_t v, uint32_t (&red)[4][16], OP op)
{
    v = op(v, uint32_t(__shfl_xor(v, 16)));
    v = op(v, uint32_t(__shfl_xor(v, 32)));
    if ((threadIdx.x & 63u) < 16) red[threadIdx.x >> 6][threadIdx.x & 15u] = v;
    __syncthreads();
    return threadIdx.x < 16 ? op(op(red[0][threadIdx.x], red[1][threadIdx.x]), op(red[2][threadIdx.x], red[3][threadIdx.x])) : 0u;
}

// 16 bits -> the even bits of a word
__device__ __forceinline__ uint32_t pki_spread(uint32_t x)
{
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}

} // namespace

// grid: (n_pos / 16, n)
__global__ __launch_bounds__(256) void pki_init_kernel(const uint32_t n_pos, const uint64_t t, const uint2 *__restrict__ group_keys,
                                                       uint32_t *__restrict__ labels, uint32_t *__restrict__ sizes, uint32_t *__restrict__ fliptab)
{
    const uint32_t g = blockIdx.y;
    const size_t idx = size_t(blockIdx.x) * 256 + threadIdx.x, base = size_t(g) * n_pos * 16;
    labels[base + idx] = uint32_t(idx >> 4);
    sizes[base + idx] = 0;
    if (idx < n_pos / 8) { // root positions 8 idx .. 8 idx + 7: position r is half r & 1 of word (r & 7) >> 1 of its call
        const uint4 v = philox4x32_10(make_uint4(uint32_t(t), uint32_t(idx), DOM_PK_ICM_FLIP, ctr2(t, 0, 0)), group_keys[g]);
        *reinterpret_cast<uint4 *>(fliptab + size_t(g) * (n_pos / 2) + 4 * idx) = v;
    }
}

// grid: (n_pos / 16, n); a wave = four consecutive positions x 16 pairs.  Padding positions own no bond and no real position has
// a padding neighbour, so `site` is not needed here.
template <typename NBR>
__global__ __launch_bounds__(256) void pki_union_kernel(const uint32_t *__restrict__ state, const NBR nbr, const uint32_t n_pos,
                                                        const uint32_t *__restrict__ move_mask, uint32_t *__restrict__ labels)
{
    const uint32_t g = blockIdx.y, j = threadIdx.x & 15u, p = blockIdx.x * 16 + (threadIdx.x >> 4);
    const uint32_t *st = state + size_t(g) * n_pos;
    const uint32_t wp = st[p];
    const uint32_t dp = (wp ^ (wp >> 1)) & move_mask[g];
    if (!((dp >> (2 * j)) & 1u)) return;
    uint32_t *lab = labels + size_t(g) * n_pos * 16 + j; // this pair's labels: lab[16 position]
    const uint32_t n_slots = nbr.slots();
    for (uint32_t k = 0; k < n_slots; k++) {
        const uint32_t q = nbr(k, p);
        if (q <= p) continue; // the end with the smaller position owns the bond
        const uint32_t wq = st[q];
        if (((wq ^ (wq >> 1)) >> (2 * j)) & 1u) cl_unite<AGENT, 16>(lab, p, q);
    }
}

// grid: (n_pos / PKI_FLIP_POS, n); thread (position-lane pl = tid / 16, pair j) visits positions base + 16 i + pl.  Nothing writes
// the labels here, and a thread reads and writes the state word of its own position alone.
__global__ __launch_bounds__(256) void pki_flip_kernel(uint32_t *__restrict__ state, const uint32_t n_pos, const uint32_t *__restrict__ site,
                                                       const uint32_t *__restrict__ move_mask, const uint32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ fliptab, uint32_t *__restrict__ sizes,
                                                       uint32_t *__restrict__ stats, uint32_t *__restrict__ minus)
{
    __shared__ uint32_t red[4][16];
    const uint32_t g = blockIdx.y, j = threadIdx.x & 15u, pl = threadIdx.x >> 4;
    const uint32_t *lab = labels + size_t(g) * n_pos * 16 + j;
    uint32_t *sz = sizes + size_t(g) * n_pos * 16 + j;
    const uint32_t *ft = fliptab + size_t(g) * (n_pos / 2);
    uint32_t *st = state + size_t(g) * n_pos;
    const uint32_t mask = move_mask[g] & 0x55555555u;
    // positions per root: consecutive positions of one root (a large cluster) add up in a register before they go out
    uint32_t n_roots = 0, n_minus = 0, run_root = 0, run = 0;
    for (uint32_t i = 0; i < PKI_FLIP_POS / 16; i++) {
        const uint32_t p = blockIdx.x * PKI_FLIP_POS + 16 * i + pl;
        const uint32_t w = st[p];
        const uint32_t d = site[p] != PKC_PAD_SITE ? (w ^ (w >> 1)) & mask : 0u;
        uint32_t flip = 0;
        if ((d >> (2 * j)) & 1u) {
            const uint32_t root = cl_find<AGENT, 16>(lab, p);
            flip = (ft[root >> 1] >> (16 * (root & 1u) + j)) & 1u;
            n_minus++;
            n_roots += root == p;
            if (run && root != run_root) {
                atomicAdd(sz + size_t(16) * run_root, run);
                run = 0;
            }
            run_root = root;
            run++;
        }
        const uint64_t flips = __ballot(flip != 0); // 16 lanes per position-lane of this wave
        const uint32_t m = uint32_t(flips >> (16 * (pl & 3u))) & 0xFFFFu;
        if (j == 0 && m) {
            const uint32_t x = pki_spread(m);
            st[p] = w ^ (x | (x << 1)); // both replicas of every flipped pair: they differ here, so this swaps their spins
        }
    }
    // the four position-lanes of a wave often end in the same root: one atomic for all of them
#pragma unroll
    for (uint32_t sh = 16; sh <= 32; sh *= 2) {
        const uint32_t o_root = uint32_t(__shfl_xor(run_root, sh)), o_run = uint32_t(__shfl_xor(run, sh));
        if (run && o_run && o_root == run_root) run = (threadIdx.x & sh) ? 0 : run + o_run;
    }
    if (run) atomicAdd(sz + size_t(16) * run_root, run);
    const uint32_t roots = pki_reduce_pairs(n_roots, red, [](uint32_t a, uint32_t c) { return a + c; });
    if (threadIdx.x < 16 && roots) atomicAdd(stats + 2 * (16 * size_t(g) + threadIdx.x), roots);
    __syncthreads(); // red is reused
    const uint32_t total = pki_reduce_pairs(n_minus, red, [](uint32_t a, uint32_t c) { return a + c; });
    if (threadIdx.x < 16 && total) atomicAdd(minus + 16 * size_t(g) + threadIdx.x, total);
}

// grid: (min(n_pos / 16, 1024), n)
__global__ __launch_bounds__(256) void pki_max_kernel(const uint32_t n_pos, const uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t red[4][16];
    const uint32_t g = blockIdx.y, j = threadIdx.x & 15u, pl = threadIdx.x >> 4;
    const uint32_t *sz = sizes + size_t(g) * n_pos * 16 + j;
    uint32_t m = 0;
    for (uint32_t p = blockIdx.x * 16 + pl; p < n_pos; p += gridDim.x * 16) m = max(m, sz[size_t(16) * p]);
    const uint32_t total = pki_reduce_pairs(m, red, [](uint32_t a, uint32_t c) { return max(a, c); });
    if (threadIdx.x < 16 && total) atomicMax(stats + 2 * (16 * size_t(g) + threadIdx.x) + 1, total);
}

hipError_t pk_icm_launch_step(hipStream_t stream, uint32_t *state, const PkGraphDev &G, const uint32_t *nbr_rj, uint32_t rj_slots, uint64_t t,
                              const uint2 *group_keys, const uint32_t *move_mask, const PkIcmWork &work, uint32_t n, uint32_t *stats,
                              uint32_t *minus)
{
    const uint32_t n_pos = G.n_pos;
    hipLaunchKernelGGL(pki_init_kernel, dim3(n_pos / 16, n), dim3(256), 0, stream, n_pos, t, group_keys, work.labels, work.sizes, work.fliptab);
    if (nbr_rj)
        hipLaunchKernelGGL(pki_union_kernel<RjNbr>, dim3(n_pos / 16, n), dim3(256), 0, stream, state, RjNbr{nbr_rj, n_pos, rj_slots}, n_pos, move_mask,
                           work.labels);
    else
        hipLaunchKernelGGL(pki_union_kernel<PkNbr>, dim3(n_pos / 16, n), dim3(256), 0, stream, state, PkNbr{G.nbr_ell, n_pos}, n_pos, move_mask,
                           work.labels);
    hipLaunchKernelGGL(pki_flip_kernel, dim3(n_pos / PKI_FLIP_POS, n), dim3(256), 0, stream, state, n_pos, G.site, move_mask, work.labels,
                       work.fliptab, work.sizes, stats, minus);
    hipLaunchKernelGGL(pki_max_kernel, dim3(std::min(n_pos / 16, 1024u), n), dim3(256), 0, stream, n_pos, work.sizes, stats);
    return hipGetLastError();
}

} // namespace isingmc
