// Kernels of the on-stream parallel tempering (tempering.hip launches them through tempering_types.hpp): the exchange round, and
// what turns the measurement counters of the checkerboard and the bit-sliced packed path into energies and threshold tables.
#include "tempering_types.hpp"

#include "det_exp.hpp"
#include "energy_from_counts.hpp"
#include "packed_types.hpp"
#include "philox.hpp"

namespace isingmc {

// ------------------------------------------------------------------------------------------------
// Parallel-tempering exchange round ON THE STREAM (host twin: pt_swap_round in
// host_logic.cpp -- same Philox counters, same det_exp, hence the same decisions).  One workgroup:
// the pairs (i, i+1) of the round's parity are disjoint, so one thread per pair swaps perm entries in
// place; then every rung relabels its slot's beta / thresholds if the slot is local.  No host sync.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void pt_swap_kernel(const PtDev P, uint64_t *__restrict__ thr_local /*thr_words words per local slot*/,
                                                       double *__restrict__ beta_local, const uint32_t apply_only)
{
    const unsigned long long round = P.counters[0];
    __syncthreads(); // everyone has read the round before thread 0 bumps it
    // ladder statistics: off costs this one uniform branch
    const bool stats = P.stats != nullptr && !apply_only;
    PtStats S{};
    if (stats) {
        S = pt_stats_view(P.stats, P.n_rungs);
        for (uint32_t i = threadIdx.x; i < P.n_rungs; i += blockDim.x) // a configuration counts at the beta it was just swept at
            pt_stats_add_energy(S.sum_e[i], S.sum_e2[i], P.slot_energy[P.perm[i]]);
        __syncthreads(); // the permutation before the round has been read
    }
    unsigned swaps = 0;
    for (uint32_t i = uint32_t(round & 1) + 2 * threadIdx.x; !apply_only && i + 1 < P.n_rungs; i += 2 * blockDim.x) {
        const uint32_t sa = P.perm[i], sb = P.perm[i + 1];
        const double d = (P.ladder[i] - P.ladder[i + 1]) * (P.slot_energy[sa] - P.slot_energy[sb]);
        bool accept = d >= 0.0;
        if (!accept) {
            const uint4 rnd = philox4x32_10(make_uint4(i, uint32_t(round), uint32_t(round >> 32), 0x50545357u),
                                            make_uint2(P.seed_lo, P.seed_hi));
            const uint64_t x = (uint64_t(rnd.y) << 32) | rnd.x;
            accept = double(x >> 11) * (1.0 / 9007199254740992.0) < det_exp(d);
        }
        if (accept) {
            P.perm[i] = sb;
            P.perm[i + 1] = sa;
            swaps++;
        }
        if (stats) { // the deciding thread is the pair's only writer
            S.attempts[i] += 1;
            if (accept) S.accepts[i] += 1;
        }
    }
    if (swaps) atomicAdd(&P.counters[1], (unsigned long long)swaps);
    __syncthreads();
    if (stats && P.n_rungs >= 2) { // replica flow, from the permutation after the round
        if (threadIdx.x == 0) {
            const uint32_t cold = P.perm[0], hot = P.perm[P.n_rungs - 1];
            if (S.labels[cold] == PT_LABEL_DOWN) S.round_trips[cold] += 1;
            S.labels[cold] = PT_LABEL_UP;
            S.labels[hot] = PT_LABEL_DOWN;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < P.n_rungs; i += blockDim.x) {
            const uint8_t label = S.labels[P.perm[i]];
            if (label == PT_LABEL_UP) S.n_up[i] += 1;
            if (label == PT_LABEL_DOWN) S.n_down[i] += 1;
        }
    }
    if (stats && threadIdx.x == 0) *S.rounds += 1;
    for (uint32_t i = threadIdx.x; i < P.n_rungs; i += blockDim.x) {
        const uint32_t slot = P.perm[i];
        if (slot >= P.slot_offset && slot < P.slot_offset + P.n_local) {
            const uint32_t r = slot - P.slot_offset;
            if (beta_local) beta_local[r] = P.ladder[i];
            if (P.ladder_thr)
                for (uint32_t k = 0; k < P.thr_words; k++) thr_local[size_t(P.thr_words) * r + k] = P.ladder_thr[size_t(P.thr_words) * i + k];
        }
    }
    if (threadIdx.x == 0 && !apply_only) P.counters[0] = round + 1;
}

// lattice energies from the satisfied-bond counters: E = |J| (n_bonds - 2 sat)  (exact in f64)
__global__ void lat_energy_from_counts_kernel(unsigned long long *__restrict__ meas, const uint32_t n,
                                              const double jabs, const long long n_bonds, double *__restrict__ out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) {
        out[r] = lat_energy_of_counts(jabs, n_bonds, meas[2 * size_t(r)]);
        meas[2 * size_t(r)] = 0; // the counters are left zeroed for the next measurement (no memset per round)
        meas[2 * size_t(r) + 1] = 0;
    }
}

// Energies of the local slots of a bit-sliced packed container from the measurement counters: E = |J| (undirected bonds - directed
// satisfied count) + self loops -- the arithmetic of the host's pk_energy, hence the same bits.
__global__ void pk_energy_from_counts_kernel(const unsigned long long *__restrict__ meas, const uint32_t first_slot,
                                             const uint32_t n, const double jabs, const double half_directed,
                                             const double self_energy, double *__restrict__ out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = pk_energy_of_counts(jabs, half_directed, self_energy, meas[2 * size_t(first_slot + r)]);
}

// Threshold tables of every group from per-slot thresholds (slot_thr[slot][m - 1] = T_m(beta of the slot), written by the exchange
// kernel): what pk_fill_table builds on the host for isingmc_states_set_betas, bit for bit.  One wavefront per group; lane r < 32 =
// replica bit r; slots at or beyond n_owned take the last owned slot's thresholds (as the host does).
__global__ void pk_tables_from_slots_kernel(const unsigned long long *__restrict__ slot_thr, const uint32_t n_owned,
                                            uint32_t *__restrict__ tabs)
{
    const uint32_t g = blockIdx.x, lane = threadIdx.x; // 64 threads
    uint32_t *tab = tabs + size_t(g) * PK_TAB_WORDS;
    const uint32_t slot = min(32u * g + (lane & 31u), n_owned - 1u);
    for (uint32_t m = 0; m < uint32_t(PK_MAX_DEG); m++) {
        const unsigned long long T = lane < 32 ? slot_thr[size_t(slot) * PK_MAX_DEG + m] : 0ull;
        const uint32_t all = uint32_t(__ballot(lane < 32 && (T >> THR_BITS) != 0));
        if (lane == 0) tab[PK_TAB_ALL + m] = all;
        const uint32_t hi = uint32_t(T >> 32) & ((1u << N_PLANES) - 1);
        for (int p = 0; p < N_PLANES; p++) {
            const uint32_t w = uint32_t(__ballot(lane < 32 && ((hi >> (N_PLANES - 1 - p)) & 1u)));
            if (lane == 0) tab[PK_TAB_TBW + m * N_PLANES + p] = w;
        }
        if (lane < 32) tab[PK_TAB_LO + m * 32 + lane] = uint32_t(T);
    }
}

hipError_t pt_launch_swap(hipStream_t stream, const PtDev &P, uint64_t *thr_local, double *beta_local, bool apply_only)
{
    hipLaunchKernelGGL(pt_swap_kernel, dim3(1), dim3(1024), 0, stream, P, thr_local, beta_local, apply_only ? 1u : 0u);
    return hipGetLastError();
}

hipError_t lat_launch_energy_from_counts(hipStream_t stream, unsigned long long *meas, uint32_t n, double jabs, long long n_bonds, double *out)
{
    hipLaunchKernelGGL(lat_energy_from_counts_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, meas, n, jabs, n_bonds, out);
    return hipGetLastError();
}

hipError_t pk_launch_energy_from_counts(hipStream_t stream, const unsigned long long *meas, uint32_t first_slot, uint32_t n, double jabs,
                                        double half_directed, double self_energy, double *out)
{
    hipLaunchKernelGGL(pk_energy_from_counts_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, meas, first_slot, n, jabs, half_directed,
                       self_energy, out);
    return hipGetLastError();
}

hipError_t pk_launch_tables_from_slots(hipStream_t stream, const unsigned long long *slot_thr, uint32_t n_owned, uint32_t n_groups, uint32_t *tabs)
{
    hipLaunchKernelGGL(pk_tables_from_slots_kernel, dim3(n_groups), dim3(64), 0, stream, slot_thr, n_owned, tabs);
    return hipGetLastError();
}

} // namespace isingmc
