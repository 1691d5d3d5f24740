// Spin overlaps resolved by a class label per site: one counting launch per form.
//   ovl_lat_class_kernel / ovl_lat_class_between_kernel   checkerboard path, one grid row per pair and 1024 words of each plane per
//                      workgroup: d = sa ^ sb once per word, then for every table one LDS atomic of popcount(d) where the word's 32
//                      sites share a class (rows: a word lies inside one row), else one LDS atomic per set bit of d through the
//                      word's 128-byte line of classes; the histogram u32[n_tables][n_classes] lives in dynamic LDS
//   ovl_pk_class_kernel<PAIRED>                           packed paths, one workgroup per (segment, replica group or pair block): a
//                      segment is at most 1024 positions of ONE class, so the bit-sliced carry-save counters of
//                      ovl_pk_count_kernel need no class dimension; column totals by ballot, as its D half takes them
// Every kernel ends with at most one 64-bit atomic per non-zero counter and workgroup.  Nothing is written but the accumulators.
#include "overlap_class_kernels.hpp"

#include <algorithm>

#include "host_logic.hpp"
#include "kernel_pick.hpp"
#include "lat_class_count.hpp"

namespace isingmc {

namespace {

static_assert(CLASS_SEGMENT_MAX == 256 * OVL_PK_ITER, "a segment is what one workgroup of ovl_pk_class_kernel counts");
static_assert(CLASS_NONE == OVC_NO_CLASS, "host_logic.cpp class_segments drops the positions without a class");

// the body of both checkerboard kernels: sa / sb = the planes of the pair's two replicas, acc = the pair's [n_tables][n_classes];
// the counting itself is lat_class_count (lat_class_count.hpp) over d = sa ^ sb, once per word
__device__ __forceinline__ void ovl_lat_class_body(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb, const LatGeom &g,
                                                   const LatClassDev &C, unsigned long long *__restrict__ acc)
{
    lat_class_count([&](uint32_t pw) { return sa[pw] ^ sb[pw]; }, g, C, acc);
}

} // namespace

// grid: (lat_class_blocks, n_pairs); pair p = replicas 2 p and 2 p + 1 of `state`; dynamic LDS: 4 bytes per bin
__global__ __launch_bounds__(256) void ovl_lat_class_kernel(const uint32_t *__restrict__ state, const LatGeom g, const LatClassDev C,
                                                            unsigned long long *__restrict__ out)
{
    const uint32_t p = blockIdx.y;
    const uint32_t *sa = state + size_t(2 * p) * 2 * g.wpp;
    ovl_lat_class_body(sa, sa + 2 * g.wpp, g, C, out + size_t(p) * C.n_tables * C.n_classes);
}

// The same with pair p = replica slots_a[p] behind state_a and replica slots_b[p] behind state_b (wave-uniform table reads).
__global__ __launch_bounds__(256) void ovl_lat_class_between_kernel(const uint32_t *__restrict__ state_a, const uint32_t *__restrict__ state_b,
                                                                    const uint32_t *__restrict__ slots_a, const uint32_t *__restrict__ slots_b,
                                                                    const LatGeom g, const LatClassDev C, unsigned long long *__restrict__ out)
{
    const uint32_t p = blockIdx.y;
    ovl_lat_class_body(state_a + size_t(slots_a[p]) * 2 * g.wpp, state_b + size_t(slots_b[p]) * 2 * g.wpp, g, C,
                       out + size_t(p) * C.n_tables * C.n_classes);
}

// grid: (C.n_seg, items).  words: [items][n_pos] -- PAIRED: the state words of replica groups, 16 pair columns at the even bits of
// x = (w ^ (w >> 1)) & 0x55555555; else gathered overlap words of pair blocks, 32 columns.  The segment's positions carry a class
// and are no padding (class_segments dropped the others), so nothing is tested here.  out: [items][COLS][n_tables][n_classes].
template <bool PAIRED>
__global__ __launch_bounds__(256) void ovl_pk_class_kernel(const uint32_t *__restrict__ words, const uint32_t n_pos, const PkClassDev C,
                                                           unsigned long long *__restrict__ out)
{
    constexpr uint32_t COLS = PAIRED ? 16 : 32, STEP = PAIRED ? 2 : 1;
    __shared__ uint32_t red[4][COLS];
    const uint32_t *w = words + size_t(blockIdx.y) * n_pos;
    const uint4 seg = C.seg[blockIdx.x]; // wave-uniform
    const uint32_t *order = C.order + seg.z;
    uint32_t cd[OVL_D_PLANES] = {};
    for (uint32_t it = 0; it < OVL_PK_ITER; it++) {
        const uint32_t i = it * 256 + threadIdx.x;
        if (i >= seg.w) break;
        const uint32_t x = w[order[i]];
        ovl_csa_add(cd, PAIRED ? (x ^ (x >> 1)) & 0x55555555u : x);
    }
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0; // lane j < COLS: D of column j
#pragma unroll
    for (uint32_t j = 0; j < COLS; j++) {
        const uint32_t dj = ovl_column_total(cd, STEP * j);
        if (lane == j) mine = dj;
    }
    if (lane < COLS) red[threadIdx.x >> 6][lane] = mine;
    __syncthreads();
    if (threadIdx.x < COLS) {
        const uint32_t total = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (total)
            atomicAdd(out + ((size_t(blockIdx.y) * COLS + threadIdx.x) * C.n_tables + seg.x) * C.n_classes + seg.y, (unsigned long long)total);
    }
}

hipError_t overlap_class_launch_lattice(hipStream_t stream, const uint32_t *state_a, const uint32_t *state_b, const uint32_t *slots_a,
                                        const uint32_t *slots_b, const LatGeom &g, const LatClassDev &C, uint32_t n_pairs,
                                        unsigned long long *out)
{
    const uint32_t blocks = lat_class_blocks(g);
    const uint32_t lds = C.n_tables * C.n_classes * uint32_t(sizeof(uint32_t));
    if (slots_a)
        hipLaunchKernelGGL(ovl_lat_class_between_kernel, dim3(blocks, n_pairs), dim3(256), lds, stream, state_a, state_b, slots_a, slots_b, g, C, out);
    else
        hipLaunchKernelGGL(ovl_lat_class_kernel, dim3(blocks, n_pairs), dim3(256), lds, stream, state_a, g, C, out);
    return hipGetLastError();
}

hipError_t overlap_class_launch_packed(hipStream_t stream, const uint32_t *words, uint32_t n_pos, bool paired, const PkClassDev &C,
                                       uint32_t items, unsigned long long *out)
{
    if (C.n_seg == 0) return hipSuccess; // every site without a class: the accumulators stay zero
    pick(paired, [&](auto PAIRED) {
        hipLaunchKernelGGL(ovl_pk_class_kernel<PAIRED.value>, dim3(C.n_seg, items), dim3(256), 0, stream, words, n_pos, C, out);
    });
    return hipGetLastError();
}

} // namespace isingmc
