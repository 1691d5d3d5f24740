// Isoenergetic cluster move between two replica-packed containers: plain stream-ordered launches per batch of
// pair blocks (32 pairs each; pair 32 B + i is lane i of block B).
//   pkb_inverse_kernel one thread per pair, once per move and container: (local group, bit) -> pair, for pkb_apply_kernel
//   pkb_gather_kernel  one thread per (position, pair lane): reads the pair's two slot entries and its two state words, ballots the
//                      XOR of the two bits into the overlap word d[B][p] (0 on padding and on empty lanes); label = own position,
//                      size = 0; the first n_pos / 4 threads of a block also write the flip table (one Philox call = the flip bits
//                      of 128 root positions of one pair)
//   pkb_union_kernel   one thread per (position, pair lane) with its d bit set: every owned bond (neighbour position above the
//                      own) whose other end has the d bit too hooks the larger root below the smaller; no bonds array
//   pkb_flip_kernel    one thread per (position-lane, pair lane), eight positions after one another: d = 1 lanes chase to the root
//                      and look the flip bit up, ballot -> the flip word f[B][p]; counts the d = 1 positions, the roots and the
//                      positions per root
//   pkl_max_kernel<32> (S11's instantiation, through pk_cluster_launch_max: the sizes have its layout) largest cluster
//   pkb_apply_kernel   once per container, one thread per state word: XORs the flip bit of every owned bit that belongs to a pair
//                      of the batch into the word, one plain store per changed word -- no atomics on spin words
// Labels are laid out [block][position][pair lane]: a wave covers two consecutive positions x 32 pairs, so the first hop of a
// chase is one coalesced 128-byte row per position.  No kernel waits for another workgroup; every loop walks strictly decreasing
// labels (cluster_union.hpp).  Everything that depends on blockIdx alone (the inverse-table row of a group) is wave-uniform.
// The gather of the overlap word, the owned-bond union loop, the counting of roots, d = 1 positions and positions per root and the
// workgroup reduction are packed_label.hpp's, shared with S11, S12 and S15.
#include "packed_between_kernels.hpp"

#include <algorithm>

#include "packed_label.hpp"
#include "packed_nbr.hpp"
#include "philox.hpp"

namespace isingmc {

namespace {

constexpr uint32_t PKB_FLIP_POS = 64;          // positions per workgroup of pkb_flip_kernel (n_pos is a multiple of 256)
constexpr uint32_t PKB_MAX_GRID_Y = 32768;

} // namespace

// grid: (ceil(n_pairs / 256)); inv is PKB_NO_PAIR everywhere on entry
__global__ __launch_bounds__(256) void pkb_inverse_kernel(const uint32_t *__restrict__ slots, const uint32_t bit0, const uint32_t n_slots,
                                                          const uint32_t n_pairs, uint32_t *__restrict__ inv)
{
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= n_pairs) return;
    const uint32_t s = slots[n];
    if (s < n_slots) inv[bit0 + s] = n; // (bit0 + s < 32 groups)
}

// grid: (n_pos / 8, n_blocks); a wave = two consecutive positions x 32 pair lanes.  pair0 = 32 x the batch's first block.
__global__ __launch_bounds__(256) void pkb_gather_kernel(const PkSide a, const PkSide b, const uint32_t n_pos, const uint32_t *__restrict__ site,
                                                         const uint64_t t, const uint2 *__restrict__ a_keys, const uint32_t pair0,
                                                         const uint32_t n_pairs, uint32_t *__restrict__ labels, uint32_t *__restrict__ sizes,
                                                         uint32_t *__restrict__ d, uint32_t *__restrict__ fliptab)
{
    const uint32_t B = blockIdx.y;
    pkl_gather_word(a, b, n_pos, site, pair0, n_pairs, d);
    const size_t idx = size_t(blockIdx.x) * 256 + threadIdx.x, base = size_t(B) * n_pos * 32;
    labels[base + idx] = uint32_t(idx >> 5);
    sizes[base + idx] = 0;
    if (idx < n_pos / 4) { // (whole waves: n_pos / 4 is a multiple of 64) call c of pair lane j: root positions 128 c .. 128 c + 127
        const uint32_t calls = n_pos >> 7, j = uint32_t(idx) / calls, c = uint32_t(idx) % calls, nj = pair0 + 32 * B + j;
        if (nj < n_pairs) {
            const uint32_t sa = a.slots[nj];
            if (sa < a.n_slots) {
                const uint32_t ca = a.bit0 + sa;
                const uint4 v = philox4x32_10(make_uint4(uint32_t(t), c, DOM_PK_BETWEEN_FLIP, ctr2(t, ca & 31u, 0)), a_keys[ca >> 5]);
                *reinterpret_cast<uint4 *>(fliptab + size_t(B) * n_pos + size_t(j) * (n_pos >> 5) + 4 * c) = v;
            }
        }
    }
}

// grid: (n_pos / 8, n_blocks).  Padding positions and empty lanes have d = 0: they own no bond and are nobody's neighbour here.
template <typename NBR>
__global__ __launch_bounds__(256) void pkb_union_kernel(const NBR nbr, const uint32_t n_pos, const uint32_t *__restrict__ d,
                                                        uint32_t *__restrict__ labels)
{
    const uint32_t B = blockIdx.y, i = threadIdx.x & 31u, p = blockIdx.x * 8 + (threadIdx.x >> 5);
    const uint32_t *dB = d + size_t(B) * n_pos;
    if (!((dB[p] >> i) & 1u)) return;
    uint32_t *lab = labels + size_t(B) * n_pos * 32 + i; // this pair's labels: lab[32 position]
    pkl_unite_owned<32>(lab, nbr, p, [&](uint32_t q) { return (dB[q] >> i) & 1u; });
}

// grid: (n_pos / PKB_FLIP_POS, n_blocks); thread (position-lane pl = tid / 32, pair lane i) visits positions base + 8 it + pl.
// Nothing writes the labels here.  stats / minus point at the batch's first pair.
__global__ __launch_bounds__(256) void pkb_flip_kernel(const uint32_t n_pos, const uint32_t *__restrict__ d, const uint32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ fliptab, uint32_t *__restrict__ sizes, uint32_t *__restrict__ f,
                                                       uint32_t *__restrict__ stats, uint32_t *__restrict__ minus)
{
    __shared__ uint32_t red[4][32];
    const uint32_t B = blockIdx.y, i = threadIdx.x & 31u, pl = threadIdx.x >> 5;
    const uint32_t *lab = labels + size_t(B) * n_pos * 32 + i;
    const uint32_t *ft = fliptab + size_t(B) * n_pos + size_t(i) * (n_pos >> 5);
    const uint32_t *dB = d + size_t(B) * n_pos;
    uint32_t *fB = f + size_t(B) * n_pos;
    PklCounts<32> counts{sizes + size_t(B) * n_pos * 32 + i};
    for (uint32_t it = 0; it < PKB_FLIP_POS / 8; it++) {
        const uint32_t p = blockIdx.x * PKB_FLIP_POS + 8 * it + pl;
        uint32_t flip = 0;
        if ((dB[p] >> i) & 1u) {
            const uint32_t root = cl_find<PKL_AGENT, 32>(lab, p);
            flip = (ft[root >> 5] >> (root & 31u)) & 1u;
            counts.account(p, root);
        }
        const uint64_t flips = __ballot(flip != 0); // lanes 0..31: this wave's even position-lane, 32..63: the odd one
        if (i == 0) fB[p] = uint32_t(flips >> (32 * (pl & 1u)));
    }
    counts.flush();
    counts.finish(red, B, stats, minus);
}

// grid: (n_pos / 256, groups); thread = the state word of (local group blockIdx.y, position).  The inverse-table row of the group
// is wave-uniform.  Pairs [pair0, pair0 + n_batch) are the batch's: f[(pair - pair0) >> 5][p] holds their flip bits.
__global__ __launch_bounds__(256) void pkb_apply_kernel(uint32_t *__restrict__ state, const uint32_t n_pos, const uint32_t *__restrict__ inv,
                                                        const uint32_t *__restrict__ f, const uint32_t pair0, const uint32_t n_batch)
{
    const uint32_t g = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    const uint32_t *row = inv + 32 * size_t(g);
    uint32_t x = 0;
    for (uint32_t bit = 0; bit < 32; bit++) {
        const uint32_t n = row[bit];
        if (n == PKB_NO_PAIR || n < pair0 || n - pair0 >= n_batch) continue;
        const uint32_t m = n - pair0;
        x |= ((f[size_t(m >> 5) * n_pos + p] >> (m & 31u)) & 1u) << bit;
    }
    if (x) state[size_t(g) * n_pos + p] ^= x; // the two replicas differ where a flip bit is set: the XOR on both sides swaps their spins
}

hipError_t pk_between_launch_tables(hipStream_t stream, const PkBetweenSide &a, const PkBetweenSide &b, uint32_t n_pairs)
{
    for (const PkBetweenSide *s : {&a, &b}) {
        hipError_t rc = hipMemsetAsync(s->inv, 0xFF, size_t(32) * s->groups * sizeof(uint32_t), stream);
        if (rc != hipSuccess) return rc;
        hipLaunchKernelGGL(pkb_inverse_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, stream, s->slots, s->bit0, s->n_slots, n_pairs, s->inv);
    }
    return hipGetLastError();
}

hipError_t pk_between_launch_batch(hipStream_t stream, const PkBetweenSide &a, const PkBetweenSide &b, const PkGraphDev &G, const uint32_t *nbr_rj,
                                   uint32_t rj_slots, uint64_t t, const uint2 *a_keys, const PkBetweenWork &work, uint32_t block0, uint32_t n_blocks,
                                   uint32_t n_pairs, uint32_t *stats, uint32_t *minus)
{
    const uint32_t n_pos = G.n_pos, pair0 = 32 * block0;
    hipLaunchKernelGGL(pkb_gather_kernel, dim3(n_pos / 8, n_blocks), dim3(256), 0, stream, PkSide(a), PkSide(b), n_pos, G.site, t, a_keys, pair0,
                       n_pairs, work.labels, work.sizes, work.d, work.fliptab);
    pk_nbr_dispatch(G, nbr_rj, rj_slots, [&](auto nbr) {
        hipLaunchKernelGGL(pkb_union_kernel<decltype(nbr)>, dim3(n_pos / 8, n_blocks), dim3(256), 0, stream, nbr, n_pos, work.d, work.labels);
    });
    hipLaunchKernelGGL(pkb_flip_kernel, dim3(n_pos / PKB_FLIP_POS, n_blocks), dim3(256), 0, stream, n_pos, work.d, work.labels, work.fliptab,
                       work.sizes, work.f, stats + 2 * size_t(pair0), minus + pair0);
    hipError_t rc = pk_cluster_launch_max(stream, n_pos, work.sizes, n_blocks, stats + 2 * size_t(pair0));
    if (rc != hipSuccess) return rc;
    for (const PkBetweenSide *s : {&a, &b})
        for (uint32_t g0 = 0; g0 < s->groups; g0 += PKB_MAX_GRID_Y) {
            const uint32_t ng = std::min(PKB_MAX_GRID_Y, s->groups - g0);
            hipLaunchKernelGGL(pkb_apply_kernel, dim3(n_pos / 256, ng), dim3(256), 0, stream, s->state + size_t(g0) * n_pos, n_pos,
                               s->inv + 32 * size_t(g0), work.f, pair0, 32 * n_blocks);
        }
    return hipGetLastError();
}

} // namespace isingmc
