// Swendsen-Wang cluster step: five plain stream-ordered launches per batch of replicas.
//   cl_bonds_kernel   one thread per (direction, plane, word): 8 Philox calls -> the 32 active-bond bits of the word's sites;
//                     the tail of the grid writes the flip bits of all possible roots (one Philox call per 128 site ids)
//   cl_tile_kernel    one workgroup per 64 x 32 tile: union-find over the tile's inner bonds in LDS, labels = global site ids
//   cl_merge_kernel   one thread per bond that leaves a tile (both periodic wraps included): union in global memory
//   cl_flip_kernel    one wave per 64 consecutive sites of a row: chase to the root, look the flip bit up, ballot -> the two
//                     32-spin words of the row segment; counts the roots and the sites per root
//   cl_max_kernel     largest cluster (cl_max_moments_kernel while a cluster series is live, DESIGN.md S24: the same pass also
//                     sums s^2 and s^4 over the cluster sizes into the series' row)
// Every union links a root to a SMALLER site id with an integer atomicMin, so the final root of a component is its smallest
// site id whatever the order of execution, and every loop below walks strictly decreasing labels: it ends after at most
// W H steps without waiting for any other thread.
// The isoenergetic cluster move of S9 reuses the tile, merge and max kernels between two kernels of its own (further down); S10 is
// the same move between two containers, paired through slot tables in device memory.
#include "cluster_kernels.hpp"
#include "cluster_union.hpp"
#include "philox.hpp"

namespace isingmc {

namespace {

// (union-find on a label array that other threads link concurrently: cluster_union.hpp)

// bits 0, 2, 4, ... of x, packed
__device__ __forceinline__ uint32_t even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return uint32_t(x);
}

} // namespace

// grid: (ceil(4.5 wpp / 256), n).  Thread gid < 4 wpp: bond word gid = (2 d + c) wpp + w; the wpp / 2 threads behind them: the
// flip table.
__global__ __launch_bounds__(256) void cl_bonds_kernel(const uint32_t *__restrict__ state, const LatGeom g, const uint64_t t,
                                                       const uint2 *__restrict__ keys, const uint32_t jneg_uniform, const uint64_t thr,
                                                       const uint64_t *__restrict__ thr_per_replica, uint32_t *__restrict__ bonds,
                                                       uint32_t *__restrict__ fliptab)
{
    const uint32_t r = blockIdx.y, gid = blockIdx.x * 256 + threadIdx.x;
    const uint2 key = keys[r];
    const uint32_t c0 = uint32_t(t);
    if (gid >= 4 * g.wpp) {
        const uint32_t q = gid - 4 * g.wpp; // site ids 128 q .. 128 q + 127
        if (q < g.wpp / 2) {
            const uint4 v = philox4x32_10(make_uint4(c0, q, DOM_SW_FLIP, ctr2(t, 0, 0)), key);
            *reinterpret_cast<uint4 *>(fliptab + size_t(r) * 2 * g.wpp + 4 * size_t(q)) = v;
        }
        return;
    }
    const uint32_t d = gid >= 2 * g.wpp, rem = gid - d * 2 * g.wpp, c = rem >= g.wpp, w = rem - c * g.wpp;
    const uint32_t y = w / g.wpr, k = w - y * g.wpr;
    const uint32_t *own = state + size_t(r) * 2 * g.wpp + size_t(c) * g.wpp, *oth = state + size_t(r) * 2 * g.wpp + size_t(1 - c) * g.wpp;
    uint32_t nb;
    if (d == 0) { // right neighbour: compact index i + 1 on the rows where this colour sits on odd columns, else i
        nb = oth[w];
        if ((y + c) & 1u) nb = (nb >> 1) | (oth[y * g.wpr + (k + 1 == g.wpr ? 0 : k + 1)] << 31);
    } else {
        nb = oth[(y + 1 == g.H ? 0 : y + 1) * g.wpr + k];
    }
    const uint32_t sat = own[w] ^ nb ^ jneg_uniform; // J s s < 0
    const uint64_t T = thr_per_replica ? thr_per_replica[r] : thr;
    uint32_t act = 0;
    if (T >> 32) act = sat;
    else if (T != 0) {
        const uint32_t T32 = uint32_t(T);
#pragma unroll 2
        for (uint32_t j = 0; j < 8; j++) {
            const uint4 u = philox4x32_10(make_uint4(c0, w, DOM_SW_BOND, ctr2(t, c, 8 * d + j)), key);
            act |= (uint32_t(u.x < T32) | (uint32_t(u.y < T32) << 1) | (uint32_t(u.z < T32) << 2) | (uint32_t(u.w < T32) << 3)) << (4 * j);
        }
        act &= sat;
    }
    bonds[size_t(r) * 4 * g.wpp + gid] = act;
}

// grid: (W / 64, ceil(H / CL_TILE_ROWS), n)
__global__ __launch_bounds__(256) void cl_tile_kernel(const LatGeom g, const uint32_t *__restrict__ bonds, uint32_t *__restrict__ labels,
                                                      uint32_t *__restrict__ sizes)
{
    __shared__ uint32_t lab[CL_TILE_W * CL_TILE_ROWS];
    __shared__ uint32_t sb[2][2][CL_TILE_ROWS]; // [direction][plane][row of the tile]
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const uint32_t tx = blockIdx.x, y0 = blockIdx.y * CL_TILE_ROWS, r = blockIdx.z, tid = threadIdx.x;
    const uint32_t rows = min(CL_TILE_ROWS, g.H - y0);
    const uint32_t *b = bonds + size_t(r) * 4 * g.wpp;
    if (tid < 4 * CL_TILE_ROWS) {
        const uint32_t dc = tid / CL_TILE_ROWS, ly = tid % CL_TILE_ROWS;
        sb[dc >> 1][dc & 1][ly] = ly < rows ? b[size_t(dc) * g.wpp + (y0 + ly) * g.wpr + tx] : 0u;
    }
    for (uint32_t l = tid; l < CL_TILE_W * CL_TILE_ROWS; l += 256) lab[l] = l;
    __syncthreads();
    for (uint32_t l = tid; l < CL_TILE_W * rows; l += 256) {
        const uint32_t lx = l & 63u, ly = l >> 6, c = (lx + y0 + ly) & 1u, bit = lx >> 1;
        if (lx < 63 && ((sb[0][c][ly] >> bit) & 1u)) cl_unite<WG>(lab, l, l + 1);
        if (ly + 1 < rows && ((sb[1][c][ly] >> bit) & 1u)) cl_unite<WG>(lab, l, l + CL_TILE_W);
    }
    __syncthreads();
    const size_t base = size_t(r) * g.W * g.H;
    for (uint32_t l = tid; l < CL_TILE_W * rows; l += 256) {
        const uint32_t root = cl_find<WG>(lab, l); // local order = global order inside a tile: the smallest site of the local component
        const size_t site = base + size_t(y0 + (l >> 6)) * g.W + tx * CL_TILE_W + (l & 63u);
        labels[site] = (y0 + (root >> 6)) * g.W + tx * CL_TILE_W + (root & 63u);
        sizes[site] = 0;
    }
}

// grid: (ceil((H W / 64 + ceil(H / CL_TILE_ROWS) W) / 256), n): the right bond of the last column of every tile, then the down
// bond of the last row of every tile
__global__ __launch_bounds__(256) void cl_merge_kernel(const LatGeom g, const uint32_t *__restrict__ bonds, uint32_t *__restrict__ labels)
{
    const uint32_t r = blockIdx.y, gid = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n_right = g.H * g.wpr, tile_rows = (g.H + CL_TILE_ROWS - 1) / CL_TILE_ROWS;
    uint32_t x, y, d, nbr;
    if (gid < n_right) {
        y = gid / g.wpr;
        x = (gid - y * g.wpr) * CL_TILE_W + CL_TILE_W - 1;
        d = 0;
        nbr = y * g.W + (x + 1 == g.W ? 0 : x + 1);
    } else {
        const uint32_t j = gid - n_right, ty = j / g.W;
        if (ty >= tile_rows) return;
        x = j - ty * g.W;
        y = min(ty * CL_TILE_ROWS + CL_TILE_ROWS - 1, g.H - 1);
        d = 1;
        nbr = (y + 1 == g.H ? 0 : y + 1) * g.W + x;
    }
    const uint32_t c = (x + y) & 1u;
    const uint32_t word = bonds[size_t(r) * 4 * g.wpp + size_t(2 * d + c) * g.wpp + y * g.wpr + (x >> 6)];
    if ((word >> ((x >> 1) & 31u)) & 1u) cl_unite<__HIP_MEMORY_SCOPE_AGENT>(labels + size_t(r) * g.W * g.H, y * g.W + x, nbr);
}

// grid: (ceil(wpp / 4), n); wave `seg` owns sites 64 seg .. 64 seg + 63 = word seg of both planes.  Nothing writes the labels here.
__global__ __launch_bounds__(256) void cl_flip_kernel(uint32_t *__restrict__ state, const LatGeom g, const uint32_t *__restrict__ labels,
                                                      const uint32_t *__restrict__ fliptab, uint32_t *__restrict__ sizes,
                                                      uint32_t *__restrict__ stats)
{
    const uint32_t r = blockIdx.y, seg = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (seg >= g.wpp) return; // (the whole wave)
    const size_t N = size_t(g.W) * g.H;
    const uint32_t *lab = labels + size_t(r) * N;
    const uint32_t site = seg * 64 + lane;
    uint32_t root = lab[site];
    for (uint32_t p = lab[root]; p != root; p = lab[root]) root = p;
    const uint32_t flip = (fliptab[size_t(r) * (N / 32) + (root >> 5)] >> (root & 31u)) & 1u;
    const uint64_t flips = __ballot(flip != 0), roots = __ballot(root == site);
    // sites per root: lanes with the root of the first pending lane add up in one atomic (a row segment inside a large cluster
    // is one root); after four rounds the rest go one by one
    uint32_t *sz = sizes + size_t(r) * N;
    uint64_t pending = __ballot(1);
    for (int it = 0; it < 4 && pending; it++) {
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint32_t lr = __shfl(root, leader);
        const uint64_t same = __ballot(root == lr);
        if (int(lane) == leader) atomicAdd(sz + lr, uint32_t(__popcll(same)));
        pending &= ~same;
    }
    if ((pending >> lane) & 1ull) atomicAdd(sz + root, 1u);
    const uint32_t y = seg / g.wpr;
    uint32_t *st = state + size_t(r) * 2 * g.wpp;
    // even columns belong to plane y & 1, odd columns to the other one; compact index = column >> 1
    if (lane == 0) {
        st[size_t(y & 1u) * g.wpp + seg] ^= even_bits(flips);
        if (roots) atomicAdd(stats + 2 * r, uint32_t(__popcll(roots)));
    } else if (lane == 1) {
        st[size_t((y + 1) & 1u) * g.wpp + seg] ^= even_bits(flips >> 1);
    }
}

// grid: (ceil(N / 1024), n): four sites per thread (N is a multiple of 128)
__global__ __launch_bounds__(256) void cl_max_kernel(const uint32_t *__restrict__ sizes, const uint32_t quads, uint32_t *__restrict__ stats)
{
    const uint32_t r = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    uint32_t m = 0;
    if (q < quads) {
        const uint4 v = reinterpret_cast<const uint4 *>(sizes + size_t(r) * 4 * quads)[q];
        m = max(max(v.x, v.y), max(v.z, v.w));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, uint32_t(__shfl_xor(m, o)));
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(stats + 2 * r + 1, m);
}

// cl_max_kernel with the cluster-size moments of DESIGN.md S24, launched in its place while a cluster series is live: the same
// grid, the same uint4 loads, the same atomicMax.  Each thread holds S2 in 64 bits and S4 in 128 (cluster_moments.hpp); the wave
// adds up by shuffles and lane 0 adds into the row's column of replica / pair r of the batch: three 64-bit atomics per wave that
// saw a root.  Bounded by the read of `sizes`, 4 bytes per site, as the kernel it replaces.
__global__ __launch_bounds__(256) void cl_max_moments_kernel(const uint32_t *__restrict__ sizes, const uint32_t quads, uint32_t *__restrict__ stats,
                                                             const ClusterMomentsOut out)
{
    const uint32_t r = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    uint32_t m = 0;
    ClusterMoments sum;
    if (q < quads) {
        const uint4 v = reinterpret_cast<const uint4 *>(sizes + size_t(r) * 4 * quads)[q];
        m = max(max(v.x, v.y), max(v.z, v.w));
        if (m) { // (most sites are no roots)
            sum.add_size(v.x);
            sum.add_size(v.y);
            sum.add_size(v.z);
            sum.add_size(v.w);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, uint32_t(__shfl_xor(m, o)));
    if (!m) return; // (the whole wave: no root among its 256 sites)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum.add_lane_xor(o);
    if ((threadIdx.x & 63u) != 0) return;
    atomicMax(stats + 2 * r + 1, m);
    const uint32_t col = out.slot0 + r - out.first_slot;
    if (col < out.n_cols) sum.add_to(out.row + size_t(CLS_ROW) * col);
}

// one thread per column of the row
__global__ __launch_bounds__(256) void cls_store_kernel(const uint32_t *__restrict__ stats, const uint32_t *__restrict__ minus,
                                                        const unsigned long long nvars, const uint32_t first_slot, const uint32_t n_cols,
                                                        unsigned long long *__restrict__ row)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cols) return;
    const size_t slot = size_t(first_slot) + c;
    unsigned long long *col = row + size_t(CLS_ROW) * c;
    col[CLS_N_CLUSTERS] = stats[2 * slot];
    col[CLS_LARGEST] = stats[2 * slot + 1];
    col[CLS_SITES] = minus ? minus[slot] : nvars;
}

hipError_t cluster_series_launch_store(hipStream_t stream, const uint32_t *stats, const uint32_t *minus, unsigned long long nvars,
                                       uint32_t first_slot, uint32_t n_cols, unsigned long long *row)
{
    if (n_cols == 0) return hipSuccess;
    hipLaunchKernelGGL(cls_store_kernel, dim3((n_cols + 255) / 256), dim3(256), 0, stream, stats, minus, nvars, first_slot, n_cols, row);
    return hipGetLastError();
}

// the last launch of a step on a lattice: the largest cluster of every labelling problem, with the moments while a series is live
static void cl_launch_max(hipStream_t stream, const uint32_t *sizes, uint32_t quads, uint32_t n, uint32_t *stats, const ClusterMomentsOut &out)
{
    if (out.row) hipLaunchKernelGGL(cl_max_moments_kernel, dim3((quads + 255) / 256, n), dim3(256), 0, stream, sizes, quads, stats, out);
    else hipLaunchKernelGGL(cl_max_kernel, dim3((quads + 255) / 256, n), dim3(256), 0, stream, sizes, quads, stats);
}

// ---- isoenergetic cluster move between the replicas of a pair ------------------------------------------------
// Four launches of their own around the unchanged labelling: icm_bonds_kernel -> cl_tile_kernel -> cl_merge_kernel ->
// icm_flip_kernel -> cl_max_kernel, with n = number of pairs.  Pair p = replicas 2 p and 2 p + 1 of `state`; q = spins of the
// first XOR spins of the second (a set bit: q_i = -1); a bond is active iff both ends have their q bit set.  The couplings
// are never read.

// grid: (ceil(4.5 wpp / 256), n_pairs), laid out as cl_bonds_kernel.  Thread gid < 4 wpp: bond word gid = (2 d + c) wpp + w;
// tail thread j < wpp / 2 behind them: the flip bits of site ids 128 j .. 128 j + 127 and the q = -1 sites among those 128
// sites (words 2 j and 2 j + 1 of both planes), summed over the wave into one atomicAdd.
// (the body of both bond kernels: sa / sb = the planes of the pair's two replicas, key = the key of the first)
__device__ __forceinline__ void icm_bonds_body(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb, const LatGeom &g,
                                               const uint64_t t, const uint2 key, const uint32_t p, uint32_t *__restrict__ bonds,
                                               uint32_t *__restrict__ fliptab, uint32_t *__restrict__ minus)
{
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < 4 * g.wpp) {
        const uint32_t d = gid >= 2 * g.wpp, rem = gid - d * 2 * g.wpp, c = rem >= g.wpp, w = rem - c * g.wpp;
        const uint32_t y = w / g.wpr, k = w - y * g.wpr;
        const uint32_t own = size_t(c) * g.wpp, oth = size_t(1 - c) * g.wpp;
        uint32_t nb;
        if (d == 0) { // right neighbour: compact index i + 1 on the rows where this colour sits on odd columns, else i
            nb = sa[oth + w] ^ sb[oth + w];
            if ((y + c) & 1u) {
                const uint32_t w1 = oth + y * g.wpr + (k + 1 == g.wpr ? 0 : k + 1);
                nb = (nb >> 1) | ((sa[w1] ^ sb[w1]) << 31);
            }
        } else {
            const uint32_t w1 = oth + (y + 1 == g.H ? 0 : y + 1) * g.wpr + k;
            nb = sa[w1] ^ sb[w1];
        }
        bonds[size_t(p) * 4 * g.wpp + gid] = (sa[own + w] ^ sb[own + w]) & nb;
    }
    if ((gid | 63u) < 4 * g.wpp) return; // (the whole wave: no tail thread in it)
    uint32_t cnt = 0;
    const uint32_t j = gid - 4 * g.wpp; // wraps for the bond threads of a mixed wave: never below wpp / 2 then
    if (gid >= 4 * g.wpp && j < g.wpp / 2) {
        const uint4 v = philox4x32_10(make_uint4(uint32_t(t), j, DOM_ICM_FLIP, ctr2(t, 0, 0)), key);
        *reinterpret_cast<uint4 *>(fliptab + size_t(p) * 2 * g.wpp + 4 * size_t(j)) = v;
        cnt = __popc(sa[2 * j] ^ sb[2 * j]) + __popc(sa[2 * j + 1] ^ sb[2 * j + 1]) + __popc(sa[g.wpp + 2 * j] ^ sb[g.wpp + 2 * j]) +
              __popc(sa[g.wpp + 2 * j + 1] ^ sb[g.wpp + 2 * j + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += uint32_t(__shfl_xor(cnt, o));
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(minus + p, cnt);
}

__global__ __launch_bounds__(256) void icm_bonds_kernel(const uint32_t *__restrict__ state, const LatGeom g, const uint64_t t,
                                                        const uint2 *__restrict__ keys, uint32_t *__restrict__ bonds,
                                                        uint32_t *__restrict__ fliptab, uint32_t *__restrict__ minus)
{
    const uint32_t p = blockIdx.y;
    const uint32_t *sa = state + size_t(2 * p) * 2 * g.wpp;
    icm_bonds_body(sa, sa + 2 * g.wpp, g, t, keys[2 * p], p, bonds, fliptab, minus);
}

// The same between two containers: pair p = replica slots_a[p] behind state_a and replica slots_b[p] behind
// state_b; keys_a[slots_a[p]] draws the flip bits.  The two table reads are wave-uniform (blockIdx.y): scalar loads.
__global__ __launch_bounds__(256) void icm_bonds_between_kernel(const uint32_t *__restrict__ state_a, const uint32_t *__restrict__ state_b,
                                                                const uint32_t *__restrict__ slots_a, const uint32_t *__restrict__ slots_b,
                                                                const LatGeom g, const uint64_t t, const uint2 *__restrict__ keys_a,
                                                                uint32_t *__restrict__ bonds, uint32_t *__restrict__ fliptab,
                                                                uint32_t *__restrict__ minus)
{
    const uint32_t p = blockIdx.y, ra = slots_a[p], rb = slots_b[p];
    icm_bonds_body(state_a + size_t(ra) * 2 * g.wpp, state_b + size_t(rb) * 2 * g.wpp, g, t, keys_a[ra], p, bonds, fliptab, minus);
}

// grid: (ceil(wpp / 4), n_pairs); wave `seg` owns sites 64 seg .. 64 seg + 63 = word seg of both planes of both replicas.
// A q = +1 site has no active bond: it is a singleton label that neither flips nor counts.
// (the body of both flip kernels)
__device__ __forceinline__ void icm_flip_body(uint32_t *__restrict__ sa, uint32_t *__restrict__ sb, const LatGeom &g, const uint32_t p,
                                              const uint32_t *__restrict__ labels, const uint32_t *__restrict__ fliptab,
                                              uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats)
{
    const uint32_t seg = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (seg >= g.wpp) return; // (the whole wave)
    const size_t N = size_t(g.W) * g.H;
    const uint32_t y = seg / g.wpr;
    // even columns belong to plane y & 1, odd columns to the other one; compact index = column >> 1
    const size_t we = size_t(y & 1u) * g.wpp + seg, wo = size_t((y + 1) & 1u) * g.wpp + seg;
    const uint32_t qe = sa[we] ^ sb[we], qo = sa[wo] ^ sb[wo];
    const bool q = (((lane & 1u) ? qo : qe) >> (lane >> 1)) & 1u;
    const uint32_t *lab = labels + size_t(p) * N;
    const uint32_t site = seg * 64 + lane;
    uint32_t root = site;
    if (q) {
        root = lab[site];
        for (uint32_t r = lab[root]; r != root; r = lab[root]) root = r;
    }
    const uint32_t flip = (fliptab[size_t(p) * (N / 32) + (root >> 5)] >> (root & 31u)) & 1u;
    const uint64_t flips = __ballot(q && flip != 0), roots = __ballot(q && root == site);
    // sites per root, as in cl_flip_kernel, over the q = -1 lanes only
    uint32_t *sz = sizes + size_t(p) * N;
    uint64_t pending = __ballot(q);
    for (int it = 0; it < 4 && pending; it++) {
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint32_t lr = __shfl(root, leader);
        const uint64_t same = __ballot(q && root == lr);
        if (int(lane) == leader) atomicAdd(sz + lr, uint32_t(__popcll(same)));
        pending &= ~same;
    }
    if ((pending >> lane) & 1ull) atomicAdd(sz + root, 1u);
    if (!flips && !roots) return; // (the whole wave)
    const uint32_t fe = even_bits(flips), fo = even_bits(flips >> 1);
    if (lane == 0) {
        sa[we] ^= fe;
        if (roots) atomicAdd(stats + 2 * p, uint32_t(__popcll(roots)));
    } else if (lane == 1) sa[wo] ^= fo;
    else if (lane == 2) sb[we] ^= fe;
    else if (lane == 3) sb[wo] ^= fo;
}

__global__ __launch_bounds__(256) void icm_flip_kernel(uint32_t *__restrict__ state, const LatGeom g, const uint32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ fliptab, uint32_t *__restrict__ sizes,
                                                       uint32_t *__restrict__ stats)
{
    const uint32_t p = blockIdx.y;
    uint32_t *sa = state + size_t(2 * p) * 2 * g.wpp;
    icm_flip_body(sa, sa + 2 * g.wpp, g, p, labels, fliptab, sizes, stats);
}

__global__ __launch_bounds__(256) void icm_flip_between_kernel(uint32_t *__restrict__ state_a, uint32_t *__restrict__ state_b,
                                                               const uint32_t *__restrict__ slots_a, const uint32_t *__restrict__ slots_b,
                                                               const LatGeom g, const uint32_t *__restrict__ labels,
                                                               const uint32_t *__restrict__ fliptab, uint32_t *__restrict__ sizes,
                                                               uint32_t *__restrict__ stats)
{
    const uint32_t p = blockIdx.y;
    icm_flip_body(state_a + size_t(slots_a[p]) * 2 * g.wpp, state_b + size_t(slots_b[p]) * 2 * g.wpp, g, p, labels, fliptab, sizes, stats);
}

hipError_t cluster_launch_step(hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t, const uint2 *keys, uint32_t jneg_uniform,
                               uint64_t thr, const uint64_t *thr_per_replica, const ClusterWork &work, uint32_t n, uint32_t *stats,
                               const ClusterMomentsOut &moments)
{
    const uint32_t wpp = g.wpp, tile_rows = (g.H + CL_TILE_ROWS - 1) / CL_TILE_ROWS;
    const uint32_t border = g.H * g.wpr + tile_rows * g.W, quads = g.W * g.H / 4;
    hipLaunchKernelGGL(cl_bonds_kernel, dim3((4 * wpp + wpp / 2 + 255) / 256, n), dim3(256), 0, stream, state, g, t, keys, jneg_uniform, thr,
                       thr_per_replica, work.bonds, work.fliptab);
    hipLaunchKernelGGL(cl_tile_kernel, dim3(g.wpr, tile_rows, n), dim3(256), 0, stream, g, work.bonds, work.labels, work.sizes);
    hipLaunchKernelGGL(cl_merge_kernel, dim3((border + 255) / 256, n), dim3(256), 0, stream, g, work.bonds, work.labels);
    hipLaunchKernelGGL(cl_flip_kernel, dim3((wpp + 3) / 4, n), dim3(256), 0, stream, state, g, work.labels, work.fliptab, work.sizes, stats);
    cl_launch_max(stream, work.sizes, quads, n, stats, moments);
    return hipGetLastError();
}

hipError_t icm_launch_step(hipStream_t stream, uint32_t *state, const LatGeom &g, uint64_t t, const uint2 *keys, const ClusterWork &work,
                           uint32_t n_pairs, uint32_t *stats, uint32_t *minus_sites, const ClusterMomentsOut &moments)
{
    const uint32_t wpp = g.wpp, tile_rows = (g.H + CL_TILE_ROWS - 1) / CL_TILE_ROWS;
    const uint32_t border = g.H * g.wpr + tile_rows * g.W, quads = g.W * g.H / 4;
    hipLaunchKernelGGL(icm_bonds_kernel, dim3((4 * wpp + wpp / 2 + 255) / 256, n_pairs), dim3(256), 0, stream, state, g, t, keys, work.bonds,
                       work.fliptab, minus_sites);
    hipLaunchKernelGGL(cl_tile_kernel, dim3(g.wpr, tile_rows, n_pairs), dim3(256), 0, stream, g, work.bonds, work.labels, work.sizes);
    hipLaunchKernelGGL(cl_merge_kernel, dim3((border + 255) / 256, n_pairs), dim3(256), 0, stream, g, work.bonds, work.labels);
    hipLaunchKernelGGL(icm_flip_kernel, dim3((wpp + 3) / 4, n_pairs), dim3(256), 0, stream, state, g, work.labels, work.fliptab, work.sizes, stats);
    cl_launch_max(stream, work.sizes, quads, n_pairs, stats, moments);
    return hipGetLastError();
}

hipError_t icm_between_launch_step(hipStream_t stream, uint32_t *state_a, uint32_t *state_b, const uint32_t *slots_a, const uint32_t *slots_b,
                                   const LatGeom &g, uint64_t t, const uint2 *keys_a, const ClusterWork &work, uint32_t n_pairs, uint32_t *stats,
                                   uint32_t *minus_sites)
{
    const uint32_t wpp = g.wpp, tile_rows = (g.H + CL_TILE_ROWS - 1) / CL_TILE_ROWS;
    const uint32_t border = g.H * g.wpr + tile_rows * g.W, quads = g.W * g.H / 4;
    hipLaunchKernelGGL(icm_bonds_between_kernel, dim3((4 * wpp + wpp / 2 + 255) / 256, n_pairs), dim3(256), 0, stream, state_a, state_b, slots_a,
                       slots_b, g, t, keys_a, work.bonds, work.fliptab, minus_sites);
    hipLaunchKernelGGL(cl_tile_kernel, dim3(g.wpr, tile_rows, n_pairs), dim3(256), 0, stream, g, work.bonds, work.labels, work.sizes);
    hipLaunchKernelGGL(cl_merge_kernel, dim3((border + 255) / 256, n_pairs), dim3(256), 0, stream, g, work.bonds, work.labels);
    hipLaunchKernelGGL(icm_flip_between_kernel, dim3((wpp + 3) / 4, n_pairs), dim3(256), 0, stream, state_a, state_b, slots_a, slots_b, g,
                       work.labels, work.fliptab, work.sizes, stats);
    hipLaunchKernelGGL(cl_max_kernel, dim3((quads + 255) / 256, n_pairs), dim3(256), 0, stream, work.sizes, quads, stats);
    return hipGetLastError();
}

} // namespace isingmc
