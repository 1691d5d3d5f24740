// On-stream parallel tempering: the device view of a ladder and the launchers of tempering_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace isingmc {

struct PtDev {
    const double *ladder;        // beta per rung
    const uint64_t *ladder_thr;  // per rung, host-computed: lattice {T3, T4} (exp of glibc); real-coupling path: one word = its RjBeta; else nullptr
    uint32_t thr_words;          // 64-bit words of ladder_thr per rung (2 / 1)
    uint32_t *perm;              // rung -> global slot
    const double *slot_energy;   // all slots (gathered)
    unsigned long long *counters; // [0] = round, [1] = total swaps
    uint32_t n_rungs, slot_offset, n_local;
    uint32_t seed_lo, seed_hi;
    unsigned long long *stats;   // ladder statistics: the block PtStats lays out; nullptr = off
};

// Ladder statistics: ONE device block per ladder, the 8-byte arrays first, the label bytes behind them.
// attempts / accepts: per pair (i, i + 1), at the lower rung; n_up / n_down / sum_e / sum_e2: per rung; round_trips / labels: per
// GLOBAL slot.  Every exchange implementation updates it by the same rule (host twin: pt_statistics_round in host_logic.cpp).
constexpr uint8_t PT_LABEL_NONE = 0, PT_LABEL_UP = 1, PT_LABEL_DOWN = 2;
struct PtStats {
    unsigned long long *attempts, *accepts, *n_up, *n_down;
    double *sum_e, *sum_e2;
    unsigned long long *round_trips, *rounds;
    uint8_t *labels;
};
__host__ __device__ inline size_t pt_stats_words(uint32_t n) { return 7 * size_t(n) + 1 - (n ? 2 : 0); } // 2 (n - 1) + 2 n + 2 n + n + 1
__host__ __device__ inline size_t pt_stats_bytes(uint32_t n) { return 8 * (pt_stats_words(n) + (size_t(n) + 7) / 8); }
__host__ __device__ inline PtStats pt_stats_view(unsigned long long *base, uint32_t n)
{
    const size_t pairs = n ? n - 1 : 0;
    PtStats S;
    S.attempts = base;
    S.accepts = S.attempts + pairs;
    S.n_up = S.accepts + pairs;
    S.n_down = S.n_up + n;
    S.sum_e = reinterpret_cast<double *>(S.n_down + n);
    S.sum_e2 = S.sum_e + n;
    S.round_trips = reinterpret_cast<unsigned long long *>(S.sum_e2 + n);
    S.rounds = S.round_trips + n;
    S.labels = reinterpret_cast<uint8_t *>(S.rounds + 1);
    return S;
}
// one rung's addition of a round: the product and the two additions each rounded on its own (no fused multiply-add, whatever the
// translation unit's contraction setting), so that numpy reproduces the sums bit for bit
__device__ inline void pt_stats_add_energy(double &sum_e, double &sum_e2, const double e)
{
#pragma clang fp contract(off)
    const double sq = e * e;
    sum_e = sum_e + e;
    sum_e2 = sum_e2 + sq;
}

// one exchange round (apply_only: no exchanges, the relabelling alone); thr_local: P.thr_words words per local slot
hipError_t pt_launch_swap(hipStream_t stream, const PtDev &P, uint64_t *thr_local, double *beta_local, bool apply_only);
// out[r] = energy of replica r < n from the measurement counters; the lattice form leaves the counters zeroed
hipError_t lat_launch_energy_from_counts(hipStream_t stream, unsigned long long *meas, uint32_t n, double jabs, long long n_bonds, double *out);
hipError_t pk_launch_energy_from_counts(hipStream_t stream, const unsigned long long *meas, uint32_t first_slot, uint32_t n, double jabs,
                                        double half_directed, double self_energy, double *out);
// the threshold tables of n_groups groups from slot_thr[slot][PK_MAX_DEG], slots at or beyond n_owned taking the last owned one's
hipError_t pk_launch_tables_from_slots(hipStream_t stream, const unsigned long long *slot_thr, uint32_t n_owned, uint32_t n_groups, uint32_t *tabs);

} // namespace isingmc
