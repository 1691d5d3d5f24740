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
//   pkl_max_kernel<16> largest cluster (packed_label.hpp); while a cluster series is live pkl_max_moments_kernel<16> in its place
//                      
// Labels are laid out [group][position][pair]: a wave covers four consecutive positions x 16 pairs, so the first hop of a chase
// is one coalesced 64-byte row per position.  No kernel waits for another workgroup; every loop walks strictly decreasing
// labels (cluster_union.hpp).  The owned-bond union loop, the counting of roots, d = 1 positions and positions per root, the
// workgroup reduction and the largest-cluster kernel are packed_label.hpp's, shared with S11 and S13.
#include "packed_icm_kernels.hpp"

#include <algorithm>

#include "packed_label.hpp"
#include "packed_nbr.hpp"
#include "philox.hpp"

namespace isingmc {

namespace {

constexpr uint32_t PKI_FLIP_POS = 128;         // positions per workgroup of pki_flip_kernel (n_pos is a multiple of 256)

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
    pkl_unite_owned<16>(lab, nbr, p, [&](uint32_t q) {
        const uint32_t wq = st[q];
        return ((wq ^ (wq >> 1)) >> (2 * j)) & 1u;
    });
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
    const uint32_t *ft = fliptab + size_t(g) * (n_pos / 2);
    uint32_t *st = state + size_t(g) * n_pos;
    const uint32_t mask = move_mask[g] & 0x55555555u;
    PklCounts<16> counts{sizes + size_t(g) * n_pos * 16 + j};
    for (uint32_t i = 0; i < PKI_FLIP_POS / 16; i++) {
        const uint32_t p = blockIdx.x * PKI_FLIP_POS + 16 * i + pl;
        const uint32_t w = st[p];
        const uint32_t d = site[p] != PAD_SITE ? (w ^ (w >> 1)) & mask : 0u;
        uint32_t flip = 0;
        if ((d >> (2 * j)) & 1u) {
            const uint32_t root = cl_find<PKL_AGENT, 16>(lab, p);
            flip = (ft[root >> 1] >> (16 * (root & 1u) + j)) & 1u;
            counts.account(p, root);
        }
        const uint64_t flips = __ballot(flip != 0); // 16 lanes per position-lane of this wave
        const uint32_t m = uint32_t(flips >> (16 * (pl & 3u))) & 0xFFFFu;
        if (j == 0 && m) {
            const uint32_t x = pki_spread(m);
            st[p] = w ^ (x | (x << 1)); // both replicas of every flipped pair: they differ here, so this swaps their spins
        }
    }
    counts.flush();
    counts.finish(red, g, stats, minus);
}

hipError_t pk_icm_launch_step(hipStream_t stream, uint32_t *state, const PkGraphDev &G, const uint32_t *nbr_rj, uint32_t rj_slots, uint64_t t,
                              const uint2 *group_keys, const uint32_t *move_mask, const PkIcmWork &work, uint32_t n, uint32_t *stats,
                              uint32_t *minus, const ClusterMomentsOut &moments)
{
    const uint32_t n_pos = G.n_pos;
    hipLaunchKernelGGL(pki_init_kernel, dim3(n_pos / 16, n), dim3(256), 0, stream, n_pos, t, group_keys, work.labels, work.sizes, work.fliptab);
    pk_nbr_dispatch(G, nbr_rj, rj_slots, [&](auto nbr) {
        hipLaunchKernelGGL(pki_union_kernel<decltype(nbr)>, dim3(n_pos / 16, n), dim3(256), 0, stream, state, nbr, n_pos, move_mask, work.labels);
    });
    hipLaunchKernelGGL(pki_flip_kernel, dim3(n_pos / PKI_FLIP_POS, n), dim3(256), 0, stream, state, n_pos, G.site, move_mask, work.labels,
                       work.fliptab, work.sizes, stats, minus);
    pkl_launch_max<16>(stream, n_pos, work.sizes, n, stats, moments);
    return hipGetLastError();
}

} // namespace isingmc
