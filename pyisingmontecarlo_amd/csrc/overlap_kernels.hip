// Spin and link overlaps between replica pairs: one counting launch per form, plus a gather for arbitrary pairs of
// replica-packed containers.
//   ovl_lat_kernel / ovl_lat_between_kernel   checkerboard path, one grid row per pair: one thread per colour-0 word of d = sa ^ sb;
//                      D = popcount of both planes' words, B = the four bonds of the colour-0 sites (every bond joins a colour-0
//                      site to a colour-1 site: each bond once)
//   ovl_pk_count_kernel<NBR, PAIRED>          packed paths, one grid row per replica group (PAIRED: x = (w ^ (w >> 1)) & 0x55555555
//                      formed on the fly, 16 pair columns) or per pair block (the gathered words, 32 pair columns); one thread per
//                      position and OVL_PK_ITER positions after one another: bit-sliced carry-save counters per column, then one
//                      ballot per (column, counter plane)
//   ovl_pk_gather_kernel                      one thread per (position, pair lane): the overlap words of pair blocks, through the
//                      gather that S13's pkb_gather_kernel uses (packed_label.hpp)
// Every kernel reduces in the wavefront, across its four waves through LDS, and ends with one 64-bit atomic per counter and
// workgroup.  Nothing is written but the accumulators and the gather's own workspace.
#include "overlap_kernels.hpp"

#include <algorithm>

#include "packed_label.hpp"
#include "packed_nbr.hpp"

namespace isingmc {

namespace {

constexpr uint32_t OVL_LAT_WORDS = 4;      // colour-0 words per thread of the checkerboard kernels (a workgroup covers 1024 words)
constexpr uint32_t OVL_MAX_GRID_Y = 32768;
constexpr int OVL_B_PLANES = 7;            // counts up to OVL_PK_ITER x 31 slots per thread and column
static_assert(OVL_PK_ITER < (1u << OVL_D_PLANES) && OVL_PK_ITER * 31 < (1u << OVL_B_PLANES), "the bit-sliced counters must hold a thread's counts");
static_assert(PK_MAX_DEG <= 31, "OVL_B_PLANES is sized for at most 31 adjacency slots");

// the body of both checkerboard kernels: sa / sb = the planes of the pair's two replicas, acc = the pair's two accumulators
__device__ __forceinline__ void ovl_lat_body(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb, const LatGeom &g,
                                             const bool link, unsigned long long *__restrict__ acc)
{
    __shared__ uint32_t red[2][4];
    uint32_t D = 0, B = 0;
    const uint32_t *a1 = sa + g.wpp, *b1 = sb + g.wpp; // plane 1
    for (uint32_t i = 0; i < OVL_LAT_WORDS; i++) {
        const uint32_t w = (blockIdx.x * OVL_LAT_WORDS + i) * 256 + threadIdx.x;
        if (w >= g.wpp) break;
        const uint32_t own = sa[w] ^ sb[w], ce = a1[w] ^ b1[w];
        D += __popc(own) + __popc(ce);
        if (!link) continue;
        const uint32_t y = w / g.wpr, k = w - y * g.wpr;
        const uint32_t wu = ((y == 0 ? g.H : y) - 1) * g.wpr + k, wd = (y + 1 == g.H ? 0 : y + 1) * g.wpr + k;
        uint32_t si;
        if (y & 1u) { // colour-0 sites on odd columns: their horizontal neighbours have compact indices {i, i + 1}
            const uint32_t ws = y * g.wpr + (k + 1 == g.wpr ? 0 : k + 1);
            si = (ce >> 1) | ((a1[ws] ^ b1[ws]) << 31);
        } else {      // on even columns: {i - 1, i}
            const uint32_t ws = y * g.wpr + (k == 0 ? g.wpr : k) - 1;
            si = (ce << 1) | ((a1[ws] ^ b1[ws]) >> 31);
        }
        B += __popc(own ^ ce) + __popc(own ^ si) + __popc(own ^ a1[wu] ^ b1[wu]) + __popc(own ^ a1[wd] ^ b1[wd]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        D += uint32_t(__shfl_xor(D, off));
        B += uint32_t(__shfl_xor(B, off));
    }
    if ((threadIdx.x & 63u) == 0) {
        red[0][threadIdx.x >> 6] = D;
        red[1][threadIdx.x >> 6] = B;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t total = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (total) atomicAdd(acc + threadIdx.x, (unsigned long long)total);
    }
}

} // namespace

// grid: (ceil(wpp / (256 OVL_LAT_WORDS)), n_pairs); pair p = replicas 2 p and 2 p + 1 of `state`
__global__ __launch_bounds__(256) void ovl_lat_kernel(const uint32_t *__restrict__ state, const LatGeom g, const uint32_t link,
                                                      unsigned long long *__restrict__ out)
{
    const uint32_t p = blockIdx.y;
    const uint32_t *sa = state + size_t(2 * p) * 2 * g.wpp;
    ovl_lat_body(sa, sa + 2 * g.wpp, g, link != 0, out + 2 * size_t(p));
}

// The same with pair p = replica slots_a[p] behind state_a and replica slots_b[p] behind state_b.  The two table reads are
// wave-uniform (blockIdx.y): scalar loads.
__global__ __launch_bounds__(256) void ovl_lat_between_kernel(const uint32_t *__restrict__ state_a, const uint32_t *__restrict__ state_b,
                                                              const uint32_t *__restrict__ slots_a, const uint32_t *__restrict__ slots_b,
                                                              const LatGeom g, const uint32_t link, unsigned long long *__restrict__ out)
{
    const uint32_t p = blockIdx.y;
    ovl_lat_body(state_a + size_t(slots_a[p]) * 2 * g.wpp, state_b + size_t(slots_b[p]) * 2 * g.wpp, g, link != 0, out + 2 * size_t(p));
}

// grid: (ceil(n_pos / (256 OVL_PK_ITER)), items).  words: [items][n_pos] -- PAIRED: the state words of replica groups, 16 pair columns
// at the even bits of x = (w ^ (w >> 1)) & 0x55555555; else the gathered overlap words of pair blocks, 32 columns.  n_slots: the
// adjacency slots to walk (0: D alone).  A bond is counted from its end with the smaller position (the neighbour accessor returns
// a position that is not above the own one for unused slots): every stored bond once, duplicated entries once each.  Padding
// positions count for nothing and are nobody's neighbour.  out: [items][COLS][2].
template <typename NBR, bool PAIRED>
__global__ __launch_bounds__(256) void ovl_pk_count_kernel(const uint32_t *__restrict__ words, const NBR nbr, const uint32_t n_slots,
                                                           const uint32_t n_pos, const uint32_t *__restrict__ site,
                                                           unsigned long long *__restrict__ out)
{
    constexpr uint32_t COLS = PAIRED ? 16 : 32, STEP = PAIRED ? 2 : 1;
    __shared__ uint32_t red[4][2 * COLS];
    const uint32_t *w = words + size_t(blockIdx.y) * n_pos;
    const auto overlap_word = [&](uint32_t p) {
        const uint32_t x = w[p];
        return PAIRED ? (x ^ (x >> 1)) & 0x55555555u : x;
    };
    uint32_t cd[OVL_D_PLANES] = {}, cb[OVL_B_PLANES] = {};
    for (uint32_t it = 0; it < OVL_PK_ITER; it++) {
        const uint32_t p = (blockIdx.x * OVL_PK_ITER + it) * 256 + threadIdx.x;
        if (p >= n_pos) break;
        if (site[p] == PAD_SITE) continue;
        const uint32_t xp = overlap_word(p);
        ovl_csa_add(cd, xp);
        for (uint32_t k = 0; k < n_slots; k++) {
            const uint32_t q = nbr(k, p);
            if (q > p) ovl_csa_add(cb, xp ^ overlap_word(q));
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0; // lane j < COLS: D of column j; lane COLS + j: B of column j
#pragma unroll
    for (uint32_t j = 0; j < COLS; j++) {
        const uint32_t dj = ovl_column_total(cd, STEP * j);
        if (lane == j) mine = dj;
    }
    if (n_slots) {
#pragma unroll
        for (uint32_t j = 0; j < COLS; j++) {
            const uint32_t bj = ovl_column_total(cb, STEP * j);
            if (lane == COLS + j) mine = bj;
        }
    }
    if (lane < 2 * COLS) red[threadIdx.x >> 6][lane] = mine;
    __syncthreads();
    if (threadIdx.x < 2 * COLS) {
        const uint32_t total = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        const uint32_t which = threadIdx.x / COLS, j = threadIdx.x % COLS;
        if (total) atomicAdd(out + 2 * (size_t(blockIdx.y) * COLS + j) + which, (unsigned long long)total);
    }
}

// grid: (n_pos / 8, n_blocks); a wave = two consecutive positions x 32 pair lanes.  pair0 = 32 x the batch's first block.
__global__ __launch_bounds__(256) void ovl_pk_gather_kernel(const PkSide a, const PkSide b, const uint32_t n_pos, const uint32_t *__restrict__ site,
                                                            const uint32_t pair0, const uint32_t n_pairs, uint32_t *__restrict__ d)
{
    pkl_gather_word(a, b, n_pos, site, pair0, n_pairs, d);
}

hipError_t overlap_launch_lattice(hipStream_t stream, const uint32_t *state_a, const uint32_t *state_b, const uint32_t *slots_a,
                                  const uint32_t *slots_b, const LatGeom &g, bool link, size_t n_pairs, unsigned long long *out)
{
    const uint32_t blocks = (g.wpp + 256 * OVL_LAT_WORDS - 1) / (256 * OVL_LAT_WORDS);
    for (size_t p0 = 0; p0 < n_pairs; p0 += OVL_MAX_GRID_Y) {
        const uint32_t n = uint32_t(std::min<size_t>(OVL_MAX_GRID_Y, n_pairs - p0));
        if (slots_a)
            hipLaunchKernelGGL(ovl_lat_between_kernel, dim3(blocks, n), dim3(256), 0, stream, state_a, state_b, slots_a + p0, slots_b + p0, g,
                               uint32_t(link), out + 2 * p0);
        else
            hipLaunchKernelGGL(ovl_lat_kernel, dim3(blocks, n), dim3(256), 0, stream, state_a + 2 * p0 * 2 * size_t(g.wpp), g, uint32_t(link),
                               out + 2 * p0);
    }
    return hipGetLastError();
}

namespace {

template <bool PAIRED>
void ovl_pk_launch_count(hipStream_t stream, const uint32_t *words, const PkGraphDev &G, const uint32_t *nbr_rj, uint32_t rj_slots, bool link,
                         uint32_t items, unsigned long long *out)
{
    const uint32_t n_pos = G.n_pos, blocks = (n_pos + 256 * OVL_PK_ITER - 1) / (256 * OVL_PK_ITER);
    pk_nbr_dispatch(G, nbr_rj, rj_slots, [&](auto nbr) {
        hipLaunchKernelGGL((ovl_pk_count_kernel<decltype(nbr), PAIRED>), dim3(blocks, items), dim3(256), 0, stream, words, nbr,
                           link ? nbr.slots() : 0u, n_pos, G.site, out);
    });
}

} // namespace

hipError_t overlap_launch_packed_pairs(hipStream_t stream, const uint32_t *state, const PkGraphDev &G, const uint32_t *nbr_rj,
                                       uint32_t rj_slots, bool link, size_t groups, unsigned long long *out)
{
    for (size_t g0 = 0; g0 < groups; g0 += OVL_MAX_GRID_Y)
        ovl_pk_launch_count<true>(stream, state + g0 * G.n_pos, G, nbr_rj, rj_slots, link, uint32_t(std::min<size_t>(OVL_MAX_GRID_Y, groups - g0)),
                                  out + 2 * 16 * g0);
    return hipGetLastError();
}

hipError_t overlap_launch_packed_gather(hipStream_t stream, const PkSide &a, const PkSide &b, const PkGraphDev &G, uint32_t block0,
                                        uint32_t n_blocks, uint32_t n_pairs, uint32_t *d)
{
    hipLaunchKernelGGL(ovl_pk_gather_kernel, dim3(G.n_pos / 8, n_blocks), dim3(256), 0, stream, a, b, G.n_pos, G.site, 32 * block0, n_pairs, d);
    return hipGetLastError();
}

hipError_t overlap_launch_packed_tables(hipStream_t stream, const PkSide &a, const PkSide &b, const PkGraphDev &G,
                                        const uint32_t *nbr_rj, uint32_t rj_slots, bool link, uint32_t block0, uint32_t n_blocks,
                                        uint32_t n_pairs, uint32_t *d, unsigned long long *out)
{
    (void)overlap_launch_packed_gather(stream, a, b, G, block0, n_blocks, n_pairs, d);
    ovl_pk_launch_count<false>(stream, d, G, nbr_rj, rj_slots, link, n_blocks, out + 2 * 32 * size_t(block0));
    return hipGetLastError();
}

} // namespace isingmc
