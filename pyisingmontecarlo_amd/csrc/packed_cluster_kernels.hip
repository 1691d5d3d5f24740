// Swendsen-Wang cluster step on the replica-packed bit-sliced path: five plain stream-ordered launches per batch
// of replica groups.  One 32-bit word per position holds 32 replicas, positions are colour-major: neighbours are never in the
// same block, so the labelling has no tile stage -- it runs in global memory from the start.
//   pkc_init_kernel    one thread per (position, replica bit): label = own position, size = 0; the first n_pos / 4 threads also
//                      write the flip table (one Philox call = the flip words of four positions)
//   pkc_bonds_kernel   one thread per (adjacency slot, position): the owner (smaller position) of a bond turns the satisfied mask
//                      of the 32 replicas into the active word with 8 Philox calls
//   pkc_union_kernel   one thread per (position, replica bit): every active owned bond hooks the larger root below the smaller
//   pkc_flip_kernel    one thread per (position, replica bit), eight positions after one another: chase to the root, look the flip
//                      bit up, ballot -> XOR into the state word; counts the roots and the positions per root
//   pkl_max_kernel<32> largest cluster (packed_label.hpp; pk_cluster_launch_max launches it for S13 too); while a cluster series
//                      is live pkl_max_moments_kernel<32> in its place
// Labels are laid out [group][position][replica bit]: lane = replica bit, so the first hop of a wave is one coalesced 128-byte
// row per position.  Padding positions own no bonds, are never flipped and never counted.  The counting of roots and of
// positions per root, the workgroup reduction and the largest-cluster kernel are packed_label.hpp's, shared with S12 and S13.
#include "packed_cluster_kernels.hpp"

#include <algorithm>

#include "packed_label.hpp"
#include "philox.hpp"

namespace isingmc {

namespace {

constexpr uint32_t PKC_FLIP_POS = 64;          // positions per workgroup of pkc_flip_kernel (n_pos is a multiple of 256)

} // namespace

// grid: (n_pos / 8, n)
__global__ __launch_bounds__(256) void pkc_init_kernel(const uint32_t n_pos, const uint64_t t, const uint2 *__restrict__ group_keys,
                                                       uint32_t *__restrict__ labels, uint32_t *__restrict__ sizes, uint32_t *__restrict__ fliptab)
{
    const uint32_t g = blockIdx.y;
    const size_t idx = size_t(blockIdx.x) * 256 + threadIdx.x, base = size_t(g) * n_pos * 32;
    labels[base + idx] = uint32_t(idx >> 5);
    sizes[base + idx] = 0;
    if (idx < n_pos / 4) { // (whole waves: n_pos / 4 is a multiple of 64) root positions 4 idx .. 4 idx + 3
        const uint4 v = philox4x32_10(make_uint4(uint32_t(t), uint32_t(idx), DOM_PK_CL_FLIP, ctr2(t, 0, 0)), group_keys[g]);
        *reinterpret_cast<uint4 *>(fliptab + size_t(g) * n_pos + 4 * idx) = v;
    }
}

// grid: (n_pos / 256, PK_MAX_DEG, n)
__global__ __launch_bounds__(256) void pkc_bonds_kernel(const uint32_t *__restrict__ state, const PkGraphDev G, const uint64_t t,
                                                        const uint2 *__restrict__ group_keys, const uint64_t thr,
                                                        const uint64_t *__restrict__ thr_per_slot, uint32_t *__restrict__ bonds)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, g = blockIdx.z;
    const uint32_t x = G.nbr_ell[size_t(k) * G.n_pos + p], q = x & 0x7FFFFFFFu;
    uint32_t act = 0;
    if (x != PK_NO_NBR && p < q) { // the end with the smaller position owns the bond
        const uint32_t *st = state + size_t(g) * G.n_pos;
        const uint32_t sat = st[p] ^ st[q] ^ ((x >> 31) ? 0u : 0xFFFFFFFFu); // J s s < 0: J > 0 and the spins differ, J < 0 and they agree
        const uint2 key = group_keys[g];
        if (thr_per_slot) {
            if (sat) {
                const uint64_t *T = thr_per_slot + 32 * size_t(g); // (wave-uniform: scalar loads)
#pragma unroll 2
                for (uint32_t j = 0; j < 8; j++) {
                    const uint4 u = philox4x32_10(make_uint4(uint32_t(t), p, DOM_PK_CL_BOND, ctr2(t, k, j)), key);
                    act |= (uint32_t(u.x < T[4 * j]) | (uint32_t(u.y < T[4 * j + 1]) << 1) | (uint32_t(u.z < T[4 * j + 2]) << 2) |
                            (uint32_t(u.w < T[4 * j + 3]) << 3)) << (4 * j);
                }
                act &= sat;
            }
        } else if (thr >> 32) act = sat;
        else if (thr != 0 && sat) {
            const uint32_t T32 = uint32_t(thr);
#pragma unroll 2
            for (uint32_t j = 0; j < 8; j++) {
                const uint4 u = philox4x32_10(make_uint4(uint32_t(t), p, DOM_PK_CL_BOND, ctr2(t, k, j)), key);
                act |= (uint32_t(u.x < T32) | (uint32_t(u.y < T32) << 1) | (uint32_t(u.z < T32) << 2) | (uint32_t(u.w < T32) << 3)) << (4 * j);
            }
            act &= sat;
        }
    }
    bonds[(size_t(g) * PK_MAX_DEG + k) * G.n_pos + p] = act;
}

// grid: (n_pos / 8, n); a wave = two consecutive positions x 32 replica bits
__global__ __launch_bounds__(256) void pkc_union_kernel(const PkGraphDev G, const uint32_t *__restrict__ bonds, uint32_t *__restrict__ labels)
{
    const uint32_t g = blockIdx.y, b = threadIdx.x & 31u, p = blockIdx.x * 8 + (threadIdx.x >> 5);
    uint32_t *lab = labels + size_t(g) * G.n_pos * 32 + b; // this replica's labels: lab[32 position]
#pragma unroll
    for (uint32_t k = 0; k < uint32_t(PK_MAX_DEG); k++) {
        const uint32_t w = bonds[(size_t(g) * PK_MAX_DEG + k) * G.n_pos + p];
        if ((w >> b) & 1u) cl_unite<PKL_AGENT, 32>(lab, p, G.nbr_ell[size_t(k) * G.n_pos + p] & 0x7FFFFFFFu);
    }
}

// grid: (n_pos / PKC_FLIP_POS, n); thread (position-lane pl = tid / 32, replica bit b) visits positions base + 8 i + pl.  Nothing
// writes the labels here.
__global__ __launch_bounds__(256) void pkc_flip_kernel(uint32_t *__restrict__ state, const PkGraphDev G, const uint32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ fliptab, uint32_t *__restrict__ sizes,
                                                       uint32_t *__restrict__ stats)
{
    __shared__ uint32_t red[4][32];
    const uint32_t g = blockIdx.y, b = threadIdx.x & 31u, pl = threadIdx.x >> 5;
    const uint32_t *lab = labels + size_t(g) * G.n_pos * 32 + b;
    const uint32_t *ft = fliptab + size_t(g) * G.n_pos;
    uint32_t *st = state + size_t(g) * G.n_pos;
    PklCounts<32> counts{sizes + size_t(g) * G.n_pos * 32 + b};
    for (uint32_t i = 0; i < PKC_FLIP_POS / 8; i++) {
        const uint32_t p = blockIdx.x * PKC_FLIP_POS + 8 * i + pl;
        const bool real = G.site[p] != PAD_SITE;
        uint32_t flip = 0;
        if (real) {
            const uint32_t root = cl_find<PKL_AGENT, 32>(lab, p);
            flip = (ft[root] >> b) & 1u;
            counts.account(p, root);
        }
        const uint64_t flips = __ballot(flip != 0); // lanes 0..31: this wave's even position-lane, 32..63: the odd one
        const uint32_t word = uint32_t(flips >> (32 * (pl & 1u)));
        if (b == 0 && word) st[p] ^= word;
    }
    counts.flush();
    counts.finish(red, g, stats);
}

hipError_t pk_cluster_launch_step(hipStream_t stream, uint32_t *state, const PkGraphDev &G, uint64_t t, const uint2 *group_keys, uint64_t thr,
                                  const uint64_t *thr_per_slot, const PkClusterWork &work, uint32_t n, uint32_t *stats,
                                  const ClusterMomentsOut &moments)
{
    const uint32_t n_pos = G.n_pos;
    hipLaunchKernelGGL(pkc_init_kernel, dim3(n_pos / 8, n), dim3(256), 0, stream, n_pos, t, group_keys, work.labels, work.sizes, work.fliptab);
    hipLaunchKernelGGL(pkc_bonds_kernel, dim3(n_pos / 256, PK_MAX_DEG, n), dim3(256), 0, stream, state, G, t, group_keys, thr, thr_per_slot,
                       work.bonds);
    hipLaunchKernelGGL(pkc_union_kernel, dim3(n_pos / 8, n), dim3(256), 0, stream, G, work.bonds, work.labels);
    hipLaunchKernelGGL(pkc_flip_kernel, dim3(n_pos / PKC_FLIP_POS, n), dim3(256), 0, stream, state, G, work.labels, work.fliptab, work.sizes, stats);
    pkl_launch_max<32>(stream, n_pos, work.sizes, n, stats, moments);
    return hipGetLastError();
}

hipError_t pk_cluster_launch_max(hipStream_t stream, uint32_t n_pos, const uint32_t *sizes, uint32_t n, uint32_t *stats)
{
    hipLaunchKernelGGL(pkl_max_kernel<32>, dim3(std::min(n_pos / 8, 1024u), n), dim3(256), 0, stream, n_pos, sizes, stats);
    return hipGetLastError();
}

} // namespace isingmc
