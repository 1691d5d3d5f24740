// Population annealing: weights, prefix sum, source table and the two gathers of a resampling step.
// Every sum below is an exact 64-bit integer sum, so no result depends on the order in which it is taken; the only f64
// arithmetic that shapes a result is the exponent x = -(dbeta (E - E_ref)), written with the explicitly rounded intrinsics so
// that nothing can be contracted (host twin: pa_sources in host_logic.cpp).
#include "pa_kernels.hpp"

#include <algorithm>

#include "det_exp.hpp"
#include "philox.hpp"
#include "sum128.hpp"

namespace isingmc {

namespace {

constexpr size_t PA_MAX_GRID_Y = 32768;

// ---- weights ---------------------------------------------------------------------------------------------------------------
// One workgroup walks the population twice: reference energy and mean, then the weights and their sum.  (R = 2^20: 1024
// elements per thread and pass, far below one sweep of such a population.)  The f64 mean is taken in a fixed order -- the same
// bits from run to run -- but no decision depends on it.
__global__ __launch_bounds__(1024) void pa_weights_kernel(const double *__restrict__ energies, uint32_t R, double dbeta, uint2 key,
                                                          uint64_t step, unsigned long long *__restrict__ weights, PaRecord *rec)
{
    __shared__ double s_ext[1024], s_sum[1024];
    __shared__ unsigned long long s_w[1024];
    const uint32_t tid = threadIdx.x;
    const bool want_min = dbeta >= 0.0;
    double ext = energies[0], sum = 0.0;
    for (uint32_t r = tid; r < R; r += 1024) {
        const double v = energies[r];
        ext = want_min ? (v < ext ? v : ext) : (v > ext ? v : ext);
        sum += v;
    }
    s_ext[tid] = ext;
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t off = 512; off > 0; off >>= 1) {
        if (tid < off) {
            const double a = s_ext[tid], b = s_ext[tid + off];
            s_ext[tid] = want_min ? (b < a ? b : a) : (b > a ? b : a);
            s_sum[tid] += s_sum[tid + off];
        }
        __syncthreads();
    }
    const double eref = s_ext[0];
    unsigned long long acc = 0;
    for (uint32_t r = tid; r < R; r += 1024) {
        const double x = -__dmul_rn(dbeta, __dsub_rn(energies[r], eref));
        const unsigned long long w = (unsigned long long)(det_exp(x) * 4294967296.0); // in [0, 2^32]: the product is exact
        weights[r] = w;
        acc += w;
    }
    s_w[tid] = acc;
    __syncthreads();
    for (uint32_t off = 512; off > 0; off >>= 1) {
        if (tid < off) s_w[tid] += s_w[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned long long S = s_w[0];
        const uint4 rnd = philox4x32_10(make_uint4(uint32_t(step), uint32_t(step >> 32), 0u, DOM_PA_RESAMPLE), key);
        const unsigned long long U = ((unsigned long long)rnd.y << 32) | rnd.x;
        rec->sum = S;
        rec->eref = eref;
        rec->distinct = 0;
        rec->mean = s_sum[0] / double(R);
        rec->u = __umul64hi(U, S);
    }
}

// ---- inclusive prefix sum, three passes ------------------------------------------------------------------------------------
__device__ __forceinline__ void pa_block_scan_256(unsigned long long *s, uint32_t tid)
{
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const unsigned long long t = tid >= off ? s[tid - off] : 0ull;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
}

// pass 1: every workgroup scans its PA_SCAN_BLOCK elements in place and leaves their sum
__global__ __launch_bounds__(256) void pa_scan_block_kernel(unsigned long long *c, uint32_t R, unsigned long long *block_sums)
{
    __shared__ unsigned long long s[256];
    const uint32_t tid = threadIdx.x;
    const size_t base = size_t(blockIdx.x) * PA_SCAN_BLOCK + 4 * tid;
    unsigned long long v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = base + k < R ? c[base + k] : 0ull;
    v[1] += v[0];
    v[2] += v[1];
    v[3] += v[2];
    s[tid] = v[3];
    __syncthreads();
    pa_block_scan_256(s, tid);
    const unsigned long long before = tid ? s[tid - 1] : 0ull;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (base + k < R) c[base + k] = v[k] + before;
    if (tid == 255) block_sums[blockIdx.x] = s[255];
}

// pass 2: one workgroup turns the block sums into the blocks' offsets (exclusive prefix sum), 1024 at a time with a carry
__global__ __launch_bounds__(1024) void pa_scan_sums_kernel(unsigned long long *sums, uint32_t n)
{
    __shared__ unsigned long long s[1024];
    const uint32_t tid = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + tid;
        const unsigned long long v = i < n ? sums[i] : 0ull;
        s[tid] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 1024; off <<= 1) {
            const unsigned long long t = tid >= off ? s[tid - off] : 0ull;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        if (i < n) sums[i] = carry + s[tid] - v;
        carry += s[1023];
        __syncthreads();
    }
}

// pass 3: the offsets go onto the blocks
__global__ __launch_bounds__(256) void pa_scan_add_kernel(unsigned long long *c, uint32_t R, const unsigned long long *__restrict__ offsets)
{
    const size_t base = size_t(blockIdx.x) * PA_SCAN_BLOCK + 4 * threadIdx.x;
    const unsigned long long off = offsets[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (base + k < R) c[base + k] += off;
}

// ---- source table ----------------------------------------------------------------------------------------------------------
// the unique r with R C[r - 1] <= j S + u < R C[r]: the smallest r whose R C[r] exceeds j S + u.  The products need 128 bits:
// (hi, lo) pairs, compared word by word.
__device__ __forceinline__ uint32_t pa_source_of(const unsigned long long *__restrict__ c, uint32_t R, unsigned long long S,
                                                 unsigned long long u, uint32_t j)
{
    const unsigned long long p_lo = (unsigned long long)j * S, t_lo = p_lo + u;
    const unsigned long long t_hi = __umul64hi((unsigned long long)j, S) + (t_lo < p_lo ? 1ull : 0ull);
    uint32_t a = 0, b = R - 1; // j S + u < R S = R C[R - 1]: the answer is in [0, R - 1]
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        const unsigned long long cm = c[m];
        const unsigned long long q_hi = __umul64hi((unsigned long long)R, cm), q_lo = (unsigned long long)R * cm;
        if (t_hi < q_hi || (t_hi == q_hi && t_lo < q_lo)) b = m;
        else a = m + 1;
    }
    return a;
}

__global__ __launch_bounds__(256) void pa_sources_kernel(const unsigned long long *__restrict__ c, uint32_t R, PaRecord *rec,
                                                         uint32_t *__restrict__ src)
{
    __shared__ uint32_t s_src[256];
    const uint32_t tid = threadIdx.x;
    const size_t j64 = size_t(blockIdx.x) * 256 + tid;
    const bool live = j64 < R;
    const uint32_t j = uint32_t(j64);
    const unsigned long long S = c[R - 1], u = rec->u;
    const uint32_t mine = live ? pa_source_of(c, R, S, u, j) : 0xFFFFFFFFu;
    s_src[tid] = mine;
    __syncthreads();
    int first = 0; // the first slot of its source (the table is non-decreasing)
    if (live) {
        src[j] = mine;
        first = j == 0 || (tid ? s_src[tid - 1] : pa_source_of(c, R, S, u, j - 1)) != mine;
    }
    const int n = __syncthreads_count(first);
    if (tid == 0 && n) atomicAdd(&rec->distinct, (unsigned long long)n);
}

// ---- gathers ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pa_gather_u32_kernel(const uint32_t *__restrict__ in, const uint32_t *__restrict__ src, uint32_t R,
                                                            uint32_t *__restrict__ out)
{
    const size_t j = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (j < R) out[j] = in[src[j]];
}

// rows of nv elements of type T (uint4: the 16-byte form; uint32_t otherwise); blockIdx.y = the new slot
template <typename T>
__global__ void pa_row_gather_kernel(const T *__restrict__ in, T *__restrict__ out, const uint32_t *__restrict__ src, uint32_t r0, uint32_t nv)
{
    const uint32_t j = r0 + blockIdx.y;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nv) out[size_t(j) * nv + i] = in[size_t(src[j]) * nv + i];
}

// One thread per position of a target group (blockIdx.y).  The group's 32 table entries are the same for the whole launch row:
// uniform loads.  A source word is fetched again only when the source GROUP changes from one bit to the next -- with the
// monotone tables of a resampling that is rare (a group's 32 slots mostly copy from one or two groups).
__global__ __launch_bounds__(256) void pa_bit_gather_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                            const uint32_t *__restrict__ src, uint32_t R, uint32_t g0, uint32_t n_pos,
                                                            const uint32_t *__restrict__ site)
{
    const uint32_t tg = g0 + blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pos) return;
    const size_t own = size_t(tg) * n_pos + p;
    const uint32_t old = in[own];
    uint32_t word = old;
    if (site[p] != PAD_SITE) {
        const uint32_t nb = min(32u, R - 32u * tg); // slots of this group the container owns
        uint32_t cur_g = 0xFFFFFFFFu, cur_w = 0u, acc = 0u;
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t sj = src[32u * tg + b], sg = sj >> 5;
            if (sg != cur_g) {
                cur_g = sg;
                cur_w = in[size_t(sg) * n_pos + p];
            }
            acc |= ((cur_w >> (sj & 31u)) & 1u) << b;
        }
        const uint32_t mask = nb == 32u ? 0xFFFFFFFFu : (1u << nb) - 1u;
        word = (old & ~mask) | acc;
    }
    out[own] = word;
}

// ---- step chooser ------------------------------------------------------------------------------------------
// Grid-wide passes over E[R], 256 threads per workgroup, grid-stride; every workgroup reduces what it saw and adds it to the
// record with one atomic per word.  Integer sums and an integer maximum: no result depends on the order of the workgroups.
constexpr uint32_t PAC_THREADS = 256, PAC_WAVES = PAC_THREADS / 64, PAC_MAX_BLOCKS = 2048;

// f64 -> u64 that orders like the values (the bits of a finite double; -0 sorts below +0, which no decision sees)
__device__ __forceinline__ unsigned long long pac_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b >> 63 ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double pac_key_value(unsigned long long key)
{
    return __longlong_as_double((long long)(key >> 63 ? key & 0x7FFFFFFFFFFFFFFFull : ~key));
}

__device__ __forceinline__ unsigned long long pac_weight(double dbeta, double d)
{
    const double x = -__dmul_rn(dbeta, d);
    return (unsigned long long)(det_exp(x) * 4294967296.0); // in [0, 2^32]: the weight of pa_weights_kernel
}

// E_ref = min E: rec->eref_key = max of ~key
__global__ __launch_bounds__(PAC_THREADS) void pa_choose_min_kernel(const double *__restrict__ energies, uint32_t R, PaChoose *rec)
{
    __shared__ unsigned long long s_k[PAC_WAVES];
    unsigned long long best = 0;
    for (size_t r = size_t(blockIdx.x) * PAC_THREADS + threadIdx.x; r < R; r += size_t(gridDim.x) * PAC_THREADS) {
        const unsigned long long k = ~pac_key(energies[r]);
        best = k > best ? k : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63u) == 0) s_k[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < PAC_WAVES; w++) best = s_k[w] > best ? s_k[w] : best;
        atomicMax(&rec->eref_key, best);
    }
}

// sum pass: S[j] += W_r(candidate j), NC candidates (16 in the first round, 15 afterwards), the running sums in registers
template <int NC>
__global__ __launch_bounds__(PAC_THREADS) void pa_choose_sum_kernel(const double *__restrict__ energies, uint32_t R, PaChoose *rec)
{
    __shared__ unsigned long long s_part[PAC_WAVES][PA_CHOOSE_CANDIDATES];
    if (rec->done) return; // (uniform)
    const double eref = pac_key_value(~rec->eref_key);
    double dbeta[NC];
    unsigned long long acc[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
        dbeta[j] = rec->dbeta[j];
        acc[j] = 0;
    }
    for (size_t r = size_t(blockIdx.x) * PAC_THREADS + threadIdx.x; r < R; r += size_t(gridDim.x) * PAC_THREADS) {
        const double d = __dsub_rn(energies[r], eref);
#pragma unroll
        for (int j = 0; j < NC; j++) acc[j] += pac_weight(dbeta[j], d);
    }
#pragma unroll
    for (int j = 0; j < NC; j++) {
        for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o);
        if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < uint32_t(NC)) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < PAC_WAVES; w++) v += s_part[w][threadIdx.x];
        if (v) atomicAdd(&rec->sum[threadIdx.x], v);
    }
}

// overlap pass: N[j] += min(S[j], R W_r(candidate j)), 128-bit sums (every term is at most 2^63: W <= 2^32, R <= 2^31, S <= R 2^32)
template <int NC>
__global__ __launch_bounds__(PAC_THREADS) void pa_choose_overlap_kernel(const double *__restrict__ energies, uint32_t R, PaChoose *rec)
{
    __shared__ unsigned long long s_lo[PAC_WAVES][PA_CHOOSE_CANDIDATES], s_hi[PAC_WAVES][PA_CHOOSE_CANDIDATES];
    if (rec->done) return; // (uniform)
    const double eref = pac_key_value(~rec->eref_key);
    double dbeta[NC];
    unsigned long long S[NC];
    Sum128 acc[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
        dbeta[j] = rec->dbeta[j];
        S[j] = rec->sum[j];
    }
    for (size_t r = size_t(blockIdx.x) * PAC_THREADS + threadIdx.x; r < R; r += size_t(gridDim.x) * PAC_THREADS) {
        const double d = __dsub_rn(energies[r], eref);
#pragma unroll
        for (int j = 0; j < NC; j++) {
            const unsigned long long rw = (unsigned long long)R * pac_weight(dbeta[j], d);
            acc[j].add(rw < S[j] ? rw : S[j], 0ull);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; j++) {
        for (int o = 32; o > 0; o >>= 1) acc[j].add_lane_xor(o);
        if ((threadIdx.x & 63u) == 0) {
            s_lo[threadIdx.x >> 6][j] = acc[j].lo;
            s_hi[threadIdx.x >> 6][j] = acc[j].hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < uint32_t(NC)) {
        Sum128 v;
        for (uint32_t w = 0; w < PAC_WAVES; w++) v.add(s_lo[w][threadIdx.x], s_hi[w][threadIdx.x]);
        if (v.lo | v.hi) v.atomic_add_to(&rec->num_lo[threadIdx.x], &rec->num_hi[threadIdx.x]);
    }
}

// One wave.  round 0 opens the search; round 1 .. 4 counts the leading candidates whose predicate N 2^32 >= t32 R S holds
// (128-bit compare), moves (lo, width), keeps S and N of the candidate that becomes lo, clears the accumulators and writes the
// next round's candidates -- or, behind the last round, the result.
__global__ __launch_bounds__(64) void pa_choose_decide_kernel(PaChoose *rec, uint32_t R, double unit, unsigned long long t32, uint32_t round)
{
    const uint32_t j = threadIdx.x;
    if (rec->done) return; // (uniform)
    uint32_t lo = 0, width = PA_CHOOSE_GRID;
    if (round > 0) {
        lo = rec->lo;
        width = rec->width;
        const uint32_t step = width / PA_CHOOSE_CANDIDATES, nc = round == 1 ? PA_CHOOSE_CANDIDATES : PA_CHOOSE_CANDIDATES - 1;
        bool holds = false;
        unsigned long long S = 0, n_lo = 0, n_hi = 0;
        if (j < nc) {
            S = rec->sum[j];
            n_lo = rec->num_lo[j];
            n_hi = rec->num_hi[j];
            const unsigned long long l_hi = (n_hi << 32) | (n_lo >> 32), l_lo = n_lo << 32; // N < 2^94
            const unsigned long long a = t32 * R;                                            // <= 2^63
            const unsigned long long r_hi = __umul64hi(a, S), r_lo = a * S;
            holds = l_hi > r_hi || (l_hi == r_hi && l_lo >= r_lo);
        }
        const unsigned long long fails = ~__ballot(holds);           // (the lanes from nc on fail)
        const uint32_t jstar = uint32_t(__ffsll((long long)fails)) - 1u; // the leading candidates that hold: 0 .. nc
        const bool last = round == PA_CHOOSE_ROUNDS;
        // the candidate that becomes lo -- or k = 1, which the last round evaluates first when lo stays 0
        const uint32_t keep = jstar ? jstar - 1u : (last && lo == 0 ? 0u : 0xFFFFFFFFu);
        __syncthreads(); // (every lane has read its accumulators)
        if (j == keep) {
            rec->sum_k = S;
            rec->num_lo_k = n_lo;
            rec->num_hi_k = n_hi;
        }
        lo += jstar * step;
        width = step;
        if (j == 0) {
            const bool all = round == 1 && jstar == PA_CHOOSE_CANDIDATES;
            if (all || last) {
                const uint32_t k = lo ? lo : 1u;
                rec->k = k;
                rec->dbeta_k = __dmul_rn(double(k), unit);
                rec->done = all ? 1u : 0u;
            }
        }
    }
    if (j == 0) {
        rec->lo = lo;
        rec->width = width;
    }
    if (j < PA_CHOOSE_CANDIDATES) {
        rec->sum[j] = 0;
        rec->num_lo[j] = 0;
        rec->num_hi[j] = 0;
        rec->dbeta[j] = __dmul_rn(double(lo + (j + 1u) * (width / PA_CHOOSE_CANDIDATES)), unit);
    }
}

} // namespace

hipError_t pa_launch_choose(hipStream_t stream, const double *energies, uint32_t R, double unit, unsigned long long t32, PaChoose *rec)
{
    const unsigned blocks = unsigned(std::min<size_t>((size_t(R) + PAC_THREADS - 1) / PAC_THREADS, PAC_MAX_BLOCKS));
    hipError_t err = hipMemsetAsync(rec, 0, sizeof(PaChoose), stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(pa_choose_min_kernel, dim3(blocks), dim3(PAC_THREADS), 0, stream, energies, R, rec);
    hipLaunchKernelGGL(pa_choose_decide_kernel, dim3(1), dim3(64), 0, stream, rec, R, unit, t32, 0u);
    for (uint32_t round = 1; round <= PA_CHOOSE_ROUNDS; round++) {
        if (round == 1) {
            hipLaunchKernelGGL(pa_choose_sum_kernel<16>, dim3(blocks), dim3(PAC_THREADS), 0, stream, energies, R, rec);
            hipLaunchKernelGGL(pa_choose_overlap_kernel<16>, dim3(blocks), dim3(PAC_THREADS), 0, stream, energies, R, rec);
        } else {
            hipLaunchKernelGGL(pa_choose_sum_kernel<15>, dim3(blocks), dim3(PAC_THREADS), 0, stream, energies, R, rec);
            hipLaunchKernelGGL(pa_choose_overlap_kernel<15>, dim3(blocks), dim3(PAC_THREADS), 0, stream, energies, R, rec);
        }
        hipLaunchKernelGGL(pa_choose_decide_kernel, dim3(1), dim3(64), 0, stream, rec, R, unit, t32, round);
    }
    return hipGetLastError();
}

hipError_t pa_launch_weights(hipStream_t stream, const double *energies, uint32_t R, double dbeta, uint64_t seed, uint64_t step,
                             unsigned long long *weights, PaRecord *rec)
{
    hipLaunchKernelGGL(pa_weights_kernel, dim3(1), dim3(1024), 0, stream, energies, R, dbeta, make_uint2(uint32_t(seed), uint32_t(seed >> 32)),
                       step, weights, rec);
    return hipGetLastError();
}

hipError_t pa_launch_scan(hipStream_t stream, unsigned long long *c, uint32_t R, unsigned long long *block_sums)
{
    const unsigned nb = unsigned(pa_scan_blocks(R));
    hipLaunchKernelGGL(pa_scan_block_kernel, dim3(nb), dim3(256), 0, stream, c, R, block_sums);
    hipLaunchKernelGGL(pa_scan_sums_kernel, dim3(1), dim3(1024), 0, stream, block_sums, uint32_t(nb));
    hipLaunchKernelGGL(pa_scan_add_kernel, dim3(nb), dim3(256), 0, stream, c, R, block_sums);
    return hipGetLastError();
}

hipError_t pa_launch_sources(hipStream_t stream, const unsigned long long *c, uint32_t R, PaRecord *rec, uint32_t *src)
{
    hipLaunchKernelGGL(pa_sources_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, c, R, rec, src);
    return hipGetLastError();
}

hipError_t pa_launch_gather_u32(hipStream_t stream, const uint32_t *in, const uint32_t *src, uint32_t R, uint32_t *out)
{
    hipLaunchKernelGGL(pa_gather_u32_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, in, src, R, out);
    return hipGetLastError();
}

hipError_t pa_launch_row_gather(hipStream_t stream, const uint32_t *in, uint32_t *out, const uint32_t *src, size_t R, size_t state_words)
{
    // the 16-byte form needs whole uint4 rows at 16-byte aligned addresses (true of every lattice the recogniser accepts with
    // at least 128 sites: state_words = W H / 32)
    const bool wide = state_words % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const uint32_t nv = uint32_t(wide ? state_words / 4 : state_words);
    const unsigned threads = nv <= 64 ? 64u : 256u;
    for (size_t r0 = 0; r0 < R; r0 += PA_MAX_GRID_Y) {
        const dim3 grid((nv + threads - 1) / threads, unsigned(std::min(PA_MAX_GRID_Y, R - r0)));
        if (wide)
            hipLaunchKernelGGL(pa_row_gather_kernel<uint4>, grid, dim3(threads), 0, stream, reinterpret_cast<const uint4 *>(in),
                               reinterpret_cast<uint4 *>(out), src, uint32_t(r0), nv);
        else
            hipLaunchKernelGGL(pa_row_gather_kernel<uint32_t>, grid, dim3(threads), 0, stream, in, out, src, uint32_t(r0), nv);
    }
    return hipGetLastError();
}

hipError_t pa_launch_bit_gather(hipStream_t stream, const uint32_t *in, uint32_t *out, const uint32_t *src, uint32_t R, size_t groups,
                                uint32_t n_pos, const uint32_t *site)
{
    for (size_t g0 = 0; g0 < groups; g0 += PA_MAX_GRID_Y)
        hipLaunchKernelGGL(pa_bit_gather_kernel, dim3((n_pos + 255) / 256, unsigned(std::min(PA_MAX_GRID_Y, groups - g0))), dim3(256), 0, stream,
                           in, out, src, R, uint32_t(g0), n_pos, site);
    return hipGetLastError();
}

} // namespace isingmc
