// Per-site and per-bond sums over the samples of a run.  All kernels stream the state once and are bound by memory:
//   mom_lat_sum_kernel     checkerboard path, summed over replicas: one thread per (word position, kind); it walks the replicas in
//                          chunks of MOM_REG_CHUNK, adds each word (or agreement word) into MOM_REG_PLANES register planes, and after
//                          each chunk adds the 32 expanded counts to its own 64-bit totals
//   mom_pk_site_kernel     packed paths, summed: one thread per position, popcount under the owned mask over the groups
//   mom_pk_bond_kernel     ... one thread per edge-list entry, popcount of the agreement of its two positions' words
//   mom_add_kernel         per replica: one thread per state word, the word into the K time planes in global memory
//   mom_flush_kernel       per replica: one thread per state word, its K planes expanded into 32 32-bit totals and cleared
//   mom_add_by_rung_kernel     per rung of a tempering ladder, checkerboard path: mom_add_kernel with the source row
//                              routed through the ladder's permutation, one rung per blockIdx.y
//   mom_pk_add_by_rung_kernel  ... packed paths: one thread per position of a destination group, which gathers its word bit by bit
//                              from the slots that hold the group's 32 rungs
// One owner per total: no atomics, no reductions.
#include "moments_kernels.hpp"

#include <algorithm>

#include "vertical_counter.hpp"

namespace isingmc {

namespace {

constexpr uint32_t MOM_MAX_BLOCKS = 1u << 20; // grid-stride beyond this many workgroups
constexpr uint32_t MOM_MAX_GRID_Y = 65535;    // ... and beyond this many rungs or destination groups on blockIdx.y

// the slots of group g that the container owns: [32 g, 32 g + 32) cut with [bit0, bit0 + n_owned)
__device__ __forceinline__ uint32_t mom_owned_mask(uint32_t g, uint32_t bit0, uint32_t n_owned)
{
    const uint32_t base = 32 * g, lo = max(base, bit0), hi = min(base + 32, bit0 + n_owned);
    if (hi <= lo) return 0;
    const uint32_t width = hi - lo;
    return (width == 32 ? ~0u : (1u << width) - 1u) << (lo - base);
}

} // namespace

// grid: (ceil(2 wpp / 256), kinds); blockIdx.y = kind (moments_kernels.hpp)
__global__ __launch_bounds__(256) void mom_lat_sum_kernel(const uint32_t *__restrict__ state, const LatGeom g, const uint32_t n_replicas,
                                                          unsigned long long *__restrict__ totals)
{
    const uint32_t words = 2 * g.wpp, w = blockIdx.x * 256 + threadIdx.x, kind = blockIdx.y;
    if (w >= words) return;
    const uint32_t plane = w >= g.wpp ? 1u : 0u, q = w - plane * g.wpp, y = q / g.wpr, k = q - y * g.wpr;
    const uint32_t other = (1u - plane) * g.wpp;
    // the neighbour word(s) inside a replica: sites on odd columns find their right neighbours one compact index further
    const bool shifted = kind == 1 && ((plane + y) & 1u);
    uint32_t n1 = w, n2 = w;
    if (kind == 1) {
        n1 = other + q;
        n2 = other + y * g.wpr + (k + 1 == g.wpr ? 0 : k + 1);
    } else if (kind == 2) {
        n1 = other + (y + 1 == g.H ? 0 : y + 1) * g.wpr + k;
    }
    unsigned long long *mine = totals + size_t(kind) * 32 * words + w;
    for (uint32_t r0 = 0; r0 < n_replicas; r0 += MOM_REG_CHUNK) {
        const uint32_t n = min(MOM_REG_CHUNK, n_replicas - r0);
        const uint32_t *s = state + size_t(r0) * words;
        uint32_t planes[MOM_REG_PLANES] = {};
#pragma unroll 4
        for (uint32_t r = 0; r < n; r++, s += words) {
            uint32_t x = s[w];
            if (kind) {
                uint32_t nb = s[n1];
                if (shifted) nb = (nb >> 1) | (s[n2] << 31);
                x = ~(x ^ nb);
            }
            vc_add(planes, x);
        }
#pragma unroll
        for (int b = 0; b < 32; b++) mine[size_t(b) * words] += vc_value(planes, b);
    }
}

__global__ __launch_bounds__(256) void mom_pk_site_kernel(const uint32_t *__restrict__ state, const uint32_t n_pos, const uint32_t groups,
                                                          const uint32_t bit0, const uint32_t n_owned, unsigned long long *__restrict__ totals)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pos) return;
    unsigned long long sum = 0;
    for (uint32_t g = 0; g < groups; g++) sum += __popc(state[size_t(g) * n_pos + p] & mom_owned_mask(g, bit0, n_owned));
    totals[p] += sum;
}

__global__ __launch_bounds__(256) void mom_pk_bond_kernel(const uint32_t *__restrict__ state, const uint32_t n_pos, const uint32_t groups,
                                                          const uint32_t bit0, const uint32_t n_owned, const uint2 *__restrict__ edges,
                                                          const size_t n_edges, unsigned long long *__restrict__ totals)
{
    const size_t e = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint2 ends = edges[e];
    unsigned long long sum = 0;
    for (uint32_t g = 0; g < groups; g++) {
        const uint32_t *w = state + size_t(g) * n_pos;
        sum += __popc(~(w[ends.x] ^ w[ends.y]) & mom_owned_mask(g, bit0, n_owned));
    }
    totals[e] += sum;
}

__global__ __launch_bounds__(256) void mom_add_kernel(const uint32_t *__restrict__ state, const size_t n_words, const int k,
                                                      uint32_t *__restrict__ planes)
{
    for (size_t w = size_t(blockIdx.x) * 256 + threadIdx.x; w < n_words; w += size_t(gridDim.x) * 256)
        vc_add_strided(planes + w, n_words, k, state[w]);
}

__global__ __launch_bounds__(256) void mom_flush_kernel(uint32_t *__restrict__ planes, const size_t n_rows, const size_t row_words, const int k,
                                                        uint32_t *__restrict__ totals)
{
    const size_t n_words = n_rows * row_words;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < n_words; i += size_t(gridDim.x) * 256) {
        uint32_t p[MOM_MAX_TIME_PLANES];
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < MOM_MAX_TIME_PLANES; j++) {
            p[j] = j < k ? planes[size_t(j) * n_words + i] : 0u;
            any |= p[j];
        }
        if (!any) continue;
#pragma unroll
        for (int j = 0; j < MOM_MAX_TIME_PLANES; j++)
            if (j < k) planes[size_t(j) * n_words + i] = 0u;
        const size_t r = i / row_words, w = i - r * row_words;
        uint32_t *mine = totals + 32 * r * row_words + w;
#pragma unroll
        for (int b = 0; b < 32; b++) {
            const uint32_t v = vc_value(p, b);
            if (v) mine[size_t(b) * row_words] += v;
        }
    }
}

// grid: (word blocks, rungs): the rung is uniform per workgroup, so perm[rung] is one scalar load and both rows are streamed
__global__ __launch_bounds__(256) void mom_add_by_rung_kernel(const uint32_t *__restrict__ state, const uint32_t *__restrict__ perm,
                                                              const uint32_t n_rungs, const uint32_t row_words, const int k,
                                                              uint32_t *__restrict__ planes)
{
    const size_t n_words = size_t(n_rungs) * row_words;
    for (uint32_t rung = blockIdx.y; rung < n_rungs; rung += gridDim.y) {
        const uint32_t slot = perm[rung];
        if (slot >= n_rungs) continue; // (a permutation of the rungs: never taken)
        const uint32_t *src = state + size_t(slot) * row_words;
        uint32_t *dst = planes + size_t(rung) * row_words;
        for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < row_words; w += gridDim.x * 256) vc_add_strided(dst + w, n_words, k, src[w]);
    }
}

// grid: (position blocks, destination groups).  Destination word (G, p) takes bit b from the slot that holds rung 32 G + b: bit
// q & 31 of state word (q >> 5, p), q = bit0 + slot.  The 32 sources of the group are resolved once per workgroup into LDS -- bit
// position, source group, and the set of rungs that share that source group -- and read back wave-uniformly, so the loop below
// is scalar control flow around loads in which the lanes of a wave read consecutive positions of ONE source group: each source
// word is loaded once however many of the group's rungs it feeds.
__global__ __launch_bounds__(256) void mom_pk_add_by_rung_kernel(const uint32_t *__restrict__ state, const uint32_t *__restrict__ perm,
                                                                 const uint32_t n_rungs, const uint32_t n_pos, const uint32_t bit0,
                                                                 const uint32_t dst_groups, const size_t n_words, const int k,
                                                                 uint32_t *__restrict__ planes)
{
    __shared__ uint32_t src[32];  // bit0 + slot of rung 32 G + b; ~0u: no such rung
    __shared__ uint32_t same[32]; // the rungs b' of this group whose source lies in the same state group as b's
    __shared__ uint32_t valid;
    for (uint32_t G = blockIdx.y; G < dst_groups; G += gridDim.y) {
        if (threadIdx.x < 32) {
            const uint32_t rung = 32 * G + threadIdx.x;
            uint32_t q = ~0u;
            if (rung < n_rungs) {
                const uint32_t slot = perm[rung];
                if (slot < n_rungs) q = bit0 + slot; // (a permutation of the rungs: always)
            }
            src[threadIdx.x] = q;
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const uint32_t mine = src[threadIdx.x];
            uint32_t m = 0, v = 0;
            for (uint32_t b = 0; b < 32; b++) {
                const uint32_t q = src[b];
                if (q != ~0u) v |= 1u << b;
                if (q != ~0u && mine != ~0u && (q >> 5) == (mine >> 5)) m |= 1u << b;
            }
            same[threadIdx.x] = m;
            if (threadIdx.x == 0) valid = v;
        }
        __syncthreads();
        for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_pos; p += gridDim.x * 256) {
            uint32_t word = 0;
            for (uint32_t todo = __builtin_amdgcn_readfirstlane(valid); todo;) {
                const uint32_t b0 = __builtin_ctz(todo);
                uint32_t m = __builtin_amdgcn_readfirstlane(same[b0]);
                todo &= ~m;
                const uint32_t w = state[size_t(__builtin_amdgcn_readfirstlane(src[b0]) >> 5) * n_pos + p];
                for (; m; m &= m - 1) {
                    const uint32_t b = __builtin_ctz(m);
                    word |= ((w >> (__builtin_amdgcn_readfirstlane(src[b]) & 31u)) & 1u) << b;
                }
            }
            vc_add_strided(planes + size_t(G) * n_pos + p, n_words, k, word);
        }
        __syncthreads(); // the tables are rewritten for the next group
    }
}

namespace {

uint32_t mom_blocks(size_t items) { return uint32_t(std::min<size_t>((items + 255) / 256, MOM_MAX_BLOCKS)); }

} // namespace

hipError_t moments_launch_lattice_sum(hipStream_t stream, const uint32_t *state, const LatGeom &g, size_t n_replicas, bool with_bonds,
                                      unsigned long long *totals)
{
    if (n_replicas == 0) return hipSuccess;
    hipLaunchKernelGGL(mom_lat_sum_kernel, dim3((2 * g.wpp + 255) / 256, with_bonds ? 3 : 1), dim3(256), 0, stream, state, g, uint32_t(n_replicas),
                       totals);
    return hipGetLastError();
}

hipError_t moments_launch_packed_sum(hipStream_t stream, const uint32_t *state, uint32_t n_pos, size_t groups, uint32_t bit0, uint32_t n_owned,
                                     unsigned long long *site_totals, const uint2 *edges, size_t n_edges, unsigned long long *bond_totals)
{
    if (groups == 0) return hipSuccess;
    hipLaunchKernelGGL(mom_pk_site_kernel, dim3((n_pos + 255) / 256), dim3(256), 0, stream, state, n_pos, uint32_t(groups), bit0, n_owned, site_totals);
    if (n_edges)
        hipLaunchKernelGGL(mom_pk_bond_kernel, dim3(uint32_t((n_edges + 255) / 256)), dim3(256), 0, stream, state, n_pos, uint32_t(groups), bit0, n_owned,
                           edges, n_edges, bond_totals);
    return hipGetLastError();
}

hipError_t moments_launch_add(hipStream_t stream, const uint32_t *state, size_t n_words, int k, uint32_t *planes)
{
    if (n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(mom_add_kernel, dim3(mom_blocks(n_words)), dim3(256), 0, stream, state, n_words, k, planes);
    return hipGetLastError();
}

hipError_t moments_launch_flush(hipStream_t stream, uint32_t *planes, size_t n_rows, size_t row_words, int k, uint32_t *totals)
{
    if (n_rows * row_words == 0) return hipSuccess;
    hipLaunchKernelGGL(mom_flush_kernel, dim3(mom_blocks(n_rows * row_words)), dim3(256), 0, stream, planes, n_rows, row_words, k, totals);
    return hipGetLastError();
}

hipError_t moments_launch_add_by_rung(hipStream_t stream, const uint32_t *state, const uint32_t *perm, size_t n_rungs, size_t row_words, int k,
                                      uint32_t *planes)
{
    if (n_rungs * row_words == 0) return hipSuccess;
    hipLaunchKernelGGL(mom_add_by_rung_kernel, dim3(mom_blocks(row_words), uint32_t(std::min<size_t>(n_rungs, MOM_MAX_GRID_Y))), dim3(256), 0, stream,
                       state, perm, uint32_t(n_rungs), uint32_t(row_words), k, planes);
    return hipGetLastError();
}

hipError_t moments_launch_packed_add_by_rung(hipStream_t stream, const uint32_t *state, const uint32_t *perm, size_t n_rungs, uint32_t n_pos,
                                             uint32_t bit0, size_t n_words, int k, uint32_t *planes)
{
    const size_t dst_groups = (n_rungs + 31) / 32;
    if (dst_groups * n_pos == 0) return hipSuccess;
    hipLaunchKernelGGL(mom_pk_add_by_rung_kernel, dim3(mom_blocks(n_pos), uint32_t(std::min<size_t>(dst_groups, MOM_MAX_GRID_Y))), dim3(256), 0,
                       stream, state, perm, uint32_t(n_rungs), n_pos, bit0, uint32_t(dst_groups), n_words, k, planes);
    return hipGetLastError();
}

} // namespace isingmc
