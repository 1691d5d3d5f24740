// General edge-list path: greedy-coloured independent sets, CSR gather, f64 local fields.
// Replaces the serial do_time_step loop (lattice.rs:204-207) for any graph the lattice recogniser
// rejects.  DESIGN.md S4; the CPU oracle (engine C) reproduces the configurations bit for bit, which
// is why every f64 operation below is written out (explicit fma, -ffp-contract=off).
//
// Layout: sites are renumbered colour-major ("positions"), each colour class padded to a multiple
// of 64 so that one wavefront covers 64 positions of ONE class = exactly two packed state words;
// the flip mask of a wave is its __ballot, written by lane 0 -- no atomics.
#pragma once
#include "det_exp.hpp"
#include "general_types.hpp"
#include "philox.hpp"

namespace isingmc {

constexpr int GEN_ROW_BATCH = 8; // directed edges of a CSR row fetched together

// sum_e J_e s_q in adjacency order; the row is fetched in batches (see gen_sweep_kernel)
template <typename WT>
__device__ __forceinline__ double local_field(const GenGraphDev &G, const uint32_t *__restrict__ st,
                                              uint32_t p)
{
    const WT *w = static_cast<const WT *>(G.w);
    double field = 0.0;
    const uint32_t end = G.rowptr[p + 1];
    for (uint32_t e0 = G.rowptr[p]; e0 < end; e0 += GEN_ROW_BATCH) {
        uint32_t q[GEN_ROW_BATCH], word[GEN_ROW_BATCH];
        double j[GEN_ROW_BATCH];
#pragma unroll
        for (int i = 0; i < GEN_ROW_BATCH; i++) {
            const uint32_t e = min(e0 + i, end - 1);
            q[i] = G.nbr[e];
            j[i] = double(w[e]);
        }
#pragma unroll
        for (int i = 0; i < GEN_ROW_BATCH; i++) word[i] = st[q[i] >> 5];
#pragma unroll
        for (int i = 0; i < GEN_ROW_BATCH; i++)
            if (e0 + i < end) field += ((word[i] >> (q[i] & 31)) & 1u) ? j[i] : -j[i];
    }
    return field;
}

// One colour class of one timestep.  A thread owns one site for RB replicas (blockIdx.y = replica
// group): the CSR row (index + coupling per directed edge, the dominant stream) is read once per RB
// replicas instead of once per replica; only the bit gathers stay per replica.  The per-site
// arithmetic is replica-local and unchanged, so the result does not depend on RB.
template <typename WT, int RB>
__global__ __launch_bounds__(256) void gen_sweep_kernel(
    uint32_t *__restrict__ state, const GenGraphDev G, const uint32_t class_begin,
    const uint32_t class_end, const uint64_t t, const uint2 *__restrict__ keys,
    const double beta_uniform, const double *__restrict__ beta_replica, const uint32_t n_replicas)
{
    const uint32_t r0 = blockIdx.y * RB;
    const uint32_t p = class_begin + blockIdx.x * 256 + threadIdx.x;
    if (p >= class_end) return; // class sizes are multiples of 64: whole waves leave together
    const uint32_t site = G.site[p];
    const WT *w = static_cast<const WT *>(G.w);
    double field[RB];
#pragma unroll
    for (int k = 0; k < RB; k++) field[k] = 0.0;
    if (site != PAD_SITE) {
        // The row in batches of GEN_ROW_BATCH directed edges: all indices and couplings of a batch go out
        // together, then all state words of a replica -- two round trips per batch.  One edge per loop iteration
        // (index, then word) was two DEPENDENT round trips per edge: a degree-6 site waited twelve times, and
        // mid-size launches (too few waves to hide it) ran at a fifth of the big-graph rate.  The sum keeps the
        // adjacency order (f64 addition is not associative; the oracle adds in that order).
        const uint32_t end = G.rowptr[p + 1];
        for (uint32_t e0 = G.rowptr[p]; e0 < end; e0 += GEN_ROW_BATCH) {
            uint32_t q[GEN_ROW_BATCH];
            double j[GEN_ROW_BATCH];
#pragma unroll
            for (int i = 0; i < GEN_ROW_BATCH; i++) {
                const uint32_t e = min(e0 + i, end - 1); // clamped: a valid address; the term is skipped below
                q[i] = G.nbr[e];
                j[i] = double(w[e]);
            }
#pragma unroll
            for (int k = 0; k < RB; k++) {
                if (r0 + k >= n_replicas) break; // wave-uniform
                const uint32_t *st = state + size_t(r0 + k) * G.n_words;
                uint32_t word[GEN_ROW_BATCH];
#pragma unroll
                for (int i = 0; i < GEN_ROW_BATCH; i++) word[i] = st[q[i] >> 5];
#pragma unroll
                for (int i = 0; i < GEN_ROW_BATCH; i++)
                    if (e0 + i < end) field[k] += ((word[i] >> (q[i] & 31)) & 1u) ? j[i] : -j[i];
            }
        }
    }
    const double bias = (site != PAD_SITE && G.bias) ? G.bias[p] : 0.0;
#pragma unroll
    for (int k = 0; k < RB; k++) {
        const uint32_t r = r0 + k;
        if (r >= n_replicas) break; // wave-uniform
        uint32_t *st = state + size_t(r) * G.n_words;
        bool flip = false;
        if (site != PAD_SITE) {
            const double beta = beta_replica ? beta_replica[r] : beta_uniform;
            const double si = ((st[p >> 5] >> (p & 31)) & 1u) ? 1.0 : -1.0;
            const double dE = 2.0 * si * (bias - field[k]);
            flip = dE <= 0.0;
            if (!flip) {
                const uint4 rnd =
                    philox4x32_10(make_uint4(uint32_t(t), site >> 1, ctr2(t, 0, 0), DOM_GEN_SWEEP), keys[r]);
                const uint64_t x = (site & 1u) ? (uint64_t(rnd.w) << 32 | rnd.z) : (uint64_t(rnd.y) << 32 | rnd.x);
                const double u = double(x >> 11) * (1.0 / 9007199254740992.0);
                flip = u < det_exp(-beta * dE);
            }
        }
        const unsigned long long mask = __ballot(flip);
        if ((threadIdx.x & 63) == 0 && mask) {
            st[p >> 5] ^= uint32_t(mask);
            st[(p >> 5) + 1] ^= uint32_t(mask >> 32);
        }
    }
}

// random start: packed word w = Philox(key, (0, w>>2, 0, "GENI"))[w&3], padding bits cleared
__global__ __launch_bounds__(256) void gen_init_kernel(uint32_t *__restrict__ state, const GenGraphDev G,
                                                       const uint2 *__restrict__ keys, const uint32_t first_replica)
{
    const uint32_t r = first_replica + blockIdx.y;
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= G.n_words) return;
    const uint4 rnd = philox4x32_10(make_uint4(0, w >> 2, 0, DOM_GEN_INIT), keys[r]);
    uint32_t v = (w & 3) == 0 ? rnd.x : (w & 3) == 1 ? rnd.y : (w & 3) == 2 ? rnd.z : rnd.w;
    uint32_t valid = 0;
    for (int b = 0; b < 32; b++) valid |= uint32_t(G.site[32 * w + b] != PAD_SITE) << b;
    state[size_t(r) * G.n_words + w] = v & valid;
}

// per-block partial sums of E = sum_i s_i (field_i / 2 - h_i) and of M = sum_i s_i.
// partial_e[r][block], partial_m[r][block]; a second pass adds them in a fixed order, so the result
// is reproducible run to run (no floating-point atomics).
template <typename WT>
__global__ __launch_bounds__(256) void gen_measure_kernel(const uint32_t *__restrict__ state,
                                                          const GenGraphDev G,
                                                          double *__restrict__ partial_e,
                                                          long long *__restrict__ partial_m)
{
    __shared__ double se[4];
    __shared__ long long sm[4];
    const uint32_t r = blockIdx.y;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    const uint32_t *st = state + size_t(r) * G.n_words;
    double e = 0.0;
    long long m = 0;
    if (p < G.n_pos && G.site[p] != PAD_SITE) {
        const double si = ((st[p >> 5] >> (p & 31)) & 1u) ? 1.0 : -1.0;
        const double field = local_field<WT>(G, st, p);
        e = si * (0.5 * field - (G.bias ? G.bias[p] : 0.0));
        m = (long long)si;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        e += __shfl_xor(e, off);
        m += __shfl_xor(m, off);
    }
    if ((threadIdx.x & 63) == 0) { se[threadIdx.x >> 6] = e; sm[threadIdx.x >> 6] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial_e[size_t(r) * gridDim.x + blockIdx.x] = (se[0] + se[1]) + (se[2] + se[3]);
        partial_m[size_t(r) * gridDim.x + blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
}

// fixed-order tree sum of one replica's partials: out_e[r], out_m[r]
__global__ __launch_bounds__(256) void gen_reduce_kernel(const double *__restrict__ partial_e,
                                                         const long long *__restrict__ partial_m, const uint32_t n_partials,
                                                         double *__restrict__ out_e, long long *__restrict__ out_m)
{
    __shared__ double se[256];
    __shared__ long long sm[256];
    const uint32_t r = blockIdx.x;
    double e = 0.0;
    long long m = 0;
    for (uint32_t i = threadIdx.x; i < n_partials; i += 256) {
        e += partial_e[size_t(r) * n_partials + i];
        m += partial_m[size_t(r) * n_partials + i];
    }
    se[threadIdx.x] = e;
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (int(threadIdx.x) < s) { se[threadIdx.x] += se[threadIdx.x + s]; sm[threadIdx.x] += sm[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out_e[r] = se[0]; out_m[r] = sm[0]; }
}

// ------------------------------------------------------------------------------------------------
// LDS-resident variant for small graphs (packed state <= GEN_RESIDENT_MAX_BYTES): one workgroup owns
// one replica for `timesteps` whole timesteps, all colour classes, with the spins in LDS and a
// workgroup barrier between classes -- instead of n_colours launches per timestep.  Same per-site
// arithmetic and Philox counters as gen_sweep_kernel => same configurations.
// energies_out (optional): E after every timestep, [replica][timesteps], reduced in a fixed order.
// ------------------------------------------------------------------------------------------------
// STAGE: the graph itself (row pointers, neighbour positions, couplings, biases, site ids) is copied into LDS once per launch.
// A timestep of a small graph is a chain of DEPENDENT loads per colour class -- site -> row pointer -> neighbour -> spin word --
// and from global memory each link costs an L2 round trip although nothing but the spins ever changes: 2.2 us per timestep for
// 16 x 16 (c1).  Same arithmetic in the same order: bit-identical.
template <typename WT, int STAGE>
__global__ __launch_bounds__(1024) void gen_resident_kernel(
    uint32_t *__restrict__ state, const GenGraphDev G, const uint64_t t0, const uint32_t timesteps,
    const uint2 *__restrict__ keys, const double *__restrict__ beta_steps, const uint32_t beta_stride,
    const double *__restrict__ beta_replica, double *__restrict__ energies_out, const double self_energy, const uint32_t edges2)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t st[];
    __shared__ double red[16];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    uint32_t *mine = state + size_t(r) * G.n_words;
    for (uint32_t i = tid; i < G.n_words; i += nthreads) st[i] = mine[i];
    const uint2 key = keys[r];
    GenGraphDev L = G;                                     // the arrays the loops below read: global, or their LDS copies
    const WT *w = static_cast<const WT *>(G.w);
    if constexpr (STAGE != 0) {
        uint32_t off = (G.n_words + 1u) & ~1u;
        if constexpr (STAGE == 1) {
            double *s_bias = reinterpret_cast<double *>(st + off);
            if (G.bias) off += 2 * G.n_pos;
            WT *s_w = reinterpret_cast<WT *>(st + off);
            off += edges2 * uint32_t(sizeof(WT) / 4);
            off = (off + 1u) & ~1u;
            if (G.bias)
                for (uint32_t i = tid; i < G.n_pos; i += nthreads) s_bias[i] = G.bias[i];
            for (uint32_t i = tid; i < edges2; i += nthreads) s_w[i] = w[i];
            L.bias = G.bias ? s_bias : nullptr;
            w = s_w;
        }
        uint32_t *s_rowptr = st + off;
        uint32_t *s_site = s_rowptr + G.n_pos + 1;
        uint32_t *s_nbr = s_site + G.n_pos;
        for (uint32_t i = tid; i <= G.n_pos; i += nthreads) s_rowptr[i] = G.rowptr[i];
        for (uint32_t i = tid; i < G.n_pos; i += nthreads) s_site[i] = G.site[i];
        for (uint32_t i = tid; i < edges2; i += nthreads) s_nbr[i] = G.nbr[i];
        L.rowptr = s_rowptr; L.site = s_site; L.nbr = s_nbr;
    }
    __syncthreads();
    for (uint32_t k = 0; k < timesteps; k++) {
        const uint64_t t = t0 + k;
        const double beta = beta_replica ? beta_replica[r] : beta_steps[size_t(k) * beta_stride];
        for (uint32_t c = 0; c < G.n_colours; c++) {
            const uint32_t begin = G.class_base[c], end = G.class_base[c + 1];
            for (uint32_t p = begin + tid; p < end; p += nthreads) { // whole waves: class sizes are multiples of 64
                const uint32_t site = L.site[p];
                bool flip = false;
                if (site != PAD_SITE) {
                    double field = 0.0;
                    for (uint32_t e = L.rowptr[p], ee = L.rowptr[p + 1]; e < ee; e++) {
                        const uint32_t q = L.nbr[e];
                        const double j = double(w[e]);
                        field += ((st[q >> 5] >> (q & 31)) & 1u) ? j : -j;
                    }
                    const double si = ((st[p >> 5] >> (p & 31)) & 1u) ? 1.0 : -1.0;
                    const double dE = 2.0 * si * ((L.bias ? L.bias[p] : 0.0) - field);
                    flip = dE <= 0.0;
                    if (!flip) {
                        const uint4 rnd = philox4x32_10(make_uint4(uint32_t(t), site >> 1, ctr2(t, 0, 0), DOM_GEN_SWEEP), key);
                        const uint64_t x = (site & 1u) ? (uint64_t(rnd.w) << 32 | rnd.z) : (uint64_t(rnd.y) << 32 | rnd.x);
                        const double u = double(x >> 11) * (1.0 / 9007199254740992.0);
                        flip = u < det_exp(-beta * dE);
                    }
                }
                const unsigned long long mask = __ballot(flip);
                if ((tid & 63) == 0 && mask) {
                    st[p >> 5] ^= uint32_t(mask);
                    st[(p >> 5) + 1] ^= uint32_t(mask >> 32);
                }
            }
            __syncthreads();
        }
        if (energies_out) {
            double e = 0.0;
            for (uint32_t p = tid; p < G.n_pos; p += nthreads) {
                if (L.site[p] == PAD_SITE) continue;
                double field = 0.0;
                for (uint32_t ed = L.rowptr[p], ee = L.rowptr[p + 1]; ed < ee; ed++) {
                    const uint32_t q = L.nbr[ed];
                    const double j = double(w[ed]);
                    field += ((st[q >> 5] >> (q & 31)) & 1u) ? j : -j;
                }
                const double si = ((st[p >> 5] >> (p & 31)) & 1u) ? 1.0 : -1.0;
                e += si * (0.5 * field - (L.bias ? L.bias[p] : 0.0));
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
            if ((tid & 63) == 0) red[tid >> 6] = e;
            __syncthreads();
            if (tid == 0) {
                double sum = 0.0;
                for (uint32_t wv = 0; wv < (nthreads + 63) / 64; wv++) sum += red[wv];
                energies_out[size_t(r) * timesteps + k] = sum + self_energy;
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < G.n_words; i += nthreads) mine[i] = st[i];
}

} // namespace isingmc
