// The lag ring's two kernels: one pass reads the current configuration once and the live snapshots once each, counts
// the differing sites per replica and lag, and replaces the oldest snapshot.
//   acr_lat_kernel   checkerboard path: a workgroup covers 1024 words of one replica, a thread keeps ACR_LAT_WORDS of them in
//                    registers; per lag the popcounts of cur ^ snapshot are reduced in the wavefront and added to an LDS counter per
//                    lag; one 64-bit atomic per workgroup and lag at the end
//   acr_pk_kernel    packed paths: a workgroup covers 2048 positions of one replica group, a thread keeps ACR_PK_ITER words; per lag
//                    the xor words go into a bit-sliced carry-save counter per replica column (the pieces of overlap_kernels.hpp),
//                    one ballot per (column, plane) gives the wave's 32 column totals, LDS gathers them over the four waves and
//                    ACR_PK_LAG_TILE lags, and every thread then owns one (lag, column) total: one 64-bit atomic each
// Both end with the store of the thread's own words into the write slot: the words of the slot that is replaced were read by this very
// thread, earlier in program order (autocorr_kernels.hpp states the rule).
#include "autocorr_kernels.hpp"

#include <algorithm>

#include "overlap_kernels.hpp"

namespace isingmc {

// grid: n_replicas x blocks_per_row workgroups in x; lds: one counter per lag
__global__ __launch_bounds__(256) void acr_lat_kernel(const uint32_t *__restrict__ state, uint32_t *ring, const uint32_t row_words,
                                                      const uint32_t blocks_per_row, const size_t slot_words, const uint32_t n_lags,
                                                      const uint32_t live, const uint32_t write_slot, unsigned long long *__restrict__ diff)
{
    __shared__ uint32_t sums[ACR_MAX_LAGS + 1];
    const uint32_t r = blockIdx.x / blocks_per_row, b = blockIdx.x - r * blocks_per_row;
    for (uint32_t l = threadIdx.x; l <= live; l += 256) sums[l] = 0;
    __syncthreads();
    const size_t row = size_t(r) * row_words;
    uint32_t cur[ACR_LAT_WORDS], w[ACR_LAT_WORDS];
#pragma unroll
    for (uint32_t i = 0; i < ACR_LAT_WORDS; i++) {
        w[i] = (b * ACR_LAT_WORDS + i) * 256 + threadIdx.x;
        cur[i] = w[i] < row_words ? state[row + w[i]] : 0u;
    }
    for (uint32_t l = 1; l <= live; l++) {
        const uint32_t *snap = ring + size_t(acr_slot_of_lag(write_slot, l, n_lags)) * slot_words + row;
        uint32_t d = 0;
#pragma unroll
        for (uint32_t i = 0; i < ACR_LAT_WORDS; i++)
            if (w[i] < row_words) d += __popc(cur[i] ^ snap[w[i]]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += uint32_t(__shfl_xor(d, off));
        if ((threadIdx.x & 63u) == 0 && d) atomicAdd(&sums[l], d);
    }
    uint32_t *dst = ring + size_t(write_slot) * slot_words + row;
#pragma unroll
    for (uint32_t i = 0; i < ACR_LAT_WORDS; i++)
        if (w[i] < row_words) dst[w[i]] = cur[i];
    __syncthreads();
    for (uint32_t l = 1 + threadIdx.x; l <= live; l += 256) {
        const uint32_t total = sums[l];
        if (total) atomicAdd(diff + size_t(r) * (n_lags + 1) + l, (unsigned long long)total);
    }
}

// grid: (ceil(n_pos / (256 ACR_PK_ITER)), groups); lds: [ACR_PK_LAG_TILE][32] column totals
__global__ __launch_bounds__(256) void acr_pk_kernel(const uint32_t *__restrict__ state, uint32_t *ring, const uint32_t *__restrict__ site,
                                                     const uint32_t n_pos, const size_t slot_words, const uint32_t bit0, const uint32_t n_owned,
                                                     const uint32_t n_lags, const uint32_t live, const uint32_t write_slot,
                                                     unsigned long long *__restrict__ diff)
{
    static_assert(ACR_PK_LAG_TILE * 32 == 256, "every thread owns one (lag, column) total of a tile");
    static_assert(ACR_PK_ITER < (1u << ACR_PK_PLANES), "the bit-sliced counters must hold a thread's counts");
    __shared__ uint32_t tile[ACR_PK_LAG_TILE][32];
    const uint32_t G = blockIdx.y;
    // the owned slots [bit0, bit0 + n_owned) that fall into group G, as a mask of its bits (wave-uniform)
    const uint64_t lo = std::max<uint64_t>(bit0, 32ull * G), hi = std::min<uint64_t>(uint64_t(bit0) + n_owned, 32ull * G + 32);
    const uint32_t owned = hi > lo ? uint32_t(((1ull << (hi - lo)) - 1) << (lo - 32ull * G)) : 0u;
    const size_t row = size_t(G) * n_pos;
    uint32_t cur[ACR_PK_ITER], p[ACR_PK_ITER], mask[ACR_PK_ITER];
#pragma unroll
    for (uint32_t i = 0; i < ACR_PK_ITER; i++) {
        p[i] = (blockIdx.x * ACR_PK_ITER + i) * 256 + threadIdx.x;
        const bool in = p[i] < n_pos;
        cur[i] = in ? state[row + p[i]] : 0u;
        mask[i] = in && site[p[i]] != PAD_SITE ? owned : 0u;
    }
    tile[threadIdx.x >> 5][threadIdx.x & 31u] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t l0 = 1; l0 <= live; l0 += ACR_PK_LAG_TILE) {
        const uint32_t n = std::min(ACR_PK_LAG_TILE, live + 1 - l0);
        for (uint32_t t = 0; t < n; t++) {
            const uint32_t *snap = ring + size_t(acr_slot_of_lag(write_slot, l0 + t, n_lags)) * slot_words + row;
            uint32_t c[ACR_PK_PLANES] = {};
#pragma unroll
            for (uint32_t i = 0; i < ACR_PK_ITER; i++)
                if (p[i] < n_pos) ovl_csa_add(c, (cur[i] ^ snap[p[i]]) & mask[i]);
            uint32_t mine = 0; // lane j < 32: the wave's total of column j
#pragma unroll
            for (uint32_t j = 0; j < 32; j++) {
                const uint32_t dj = ovl_column_total(c, j);
                if (lane == j) mine = dj;
            }
            if (lane < 32 && mine) atomicAdd(&tile[t][lane], mine);
        }
        __syncthreads();
        {
            const uint32_t t = threadIdx.x >> 5, j = threadIdx.x & 31u, total = tile[t][j];
            if (total) { // (t < n: the rows beyond hold zero)
                atomicAdd(diff + (size_t(G) * 32 + j) * (n_lags + 1) + l0 + t, (unsigned long long)total);
                tile[t][j] = 0;
            }
        }
        __syncthreads();
    }
    uint32_t *dst = ring + size_t(write_slot) * slot_words + row;
#pragma unroll
    for (uint32_t i = 0; i < ACR_PK_ITER; i++)
        if (p[i] < n_pos) dst[p[i]] = cur[i];
}

hipError_t autocorr_launch_lattice(hipStream_t stream, const uint32_t *state, uint32_t *ring, size_t n_replicas, size_t row_words, uint32_t n_lags,
                                   uint32_t live, uint32_t write_slot, unsigned long long *diff)
{
    const size_t per_block = 256 * size_t(ACR_LAT_WORDS), blocks_per_row = (row_words + per_block - 1) / per_block;
    if (n_replicas == 0 || row_words == 0) return hipSuccess;
    if (n_lags < 1 || n_lags > ACR_MAX_LAGS || live > n_lags || write_slot >= n_lags || (row_words >> 32) ||
        blocks_per_row * n_replicas > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(acr_lat_kernel, dim3(uint32_t(blocks_per_row * n_replicas)), dim3(256), 0, stream, state, ring, uint32_t(row_words),
                       uint32_t(blocks_per_row), n_replicas * row_words, n_lags, live, write_slot, diff);
    return hipGetLastError();
}

hipError_t autocorr_launch_packed(hipStream_t stream, const uint32_t *state, uint32_t *ring, const uint32_t *site, uint32_t n_pos, size_t groups,
                                  uint32_t bit0, uint32_t n_owned, uint32_t n_lags, uint32_t live, uint32_t write_slot, unsigned long long *diff)
{
    constexpr size_t MAX_GRID_Y = 32768;
    if (groups == 0 || n_pos == 0) return hipSuccess;
    if (n_lags < 1 || n_lags > ACR_MAX_LAGS || live > n_lags || write_slot >= n_lags) return hipErrorInvalidValue;
    const uint32_t blocks = (n_pos + 256 * ACR_PK_ITER - 1) / (256 * ACR_PK_ITER);
    const size_t slot_words = groups * size_t(n_pos);
    for (size_t g0 = 0; g0 < groups; g0 += MAX_GRID_Y) { // (a second launch from 2^20 replicas on; the slots it owns move with it)
        const size_t n = std::min(MAX_GRID_Y, groups - g0);
        const uint64_t first = 32 * uint64_t(g0), lo = std::max<uint64_t>(bit0, first), hi = uint64_t(bit0) + n_owned;
        hipLaunchKernelGGL(acr_pk_kernel, dim3(blocks, uint32_t(n)), dim3(256), 0, stream, state + g0 * n_pos, ring + g0 * n_pos, site, n_pos,
                           slot_words, uint32_t(lo - first), uint32_t(hi > lo ? std::min<uint64_t>(hi - lo, 32 * uint64_t(n)) : 0), n_lags, live,
                           write_slot, diff + 32 * g0 * (size_t(n_lags) + 1));
    }
    return hipGetLastError();
}

} // namespace isingmc
