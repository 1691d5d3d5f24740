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
};

// one exchange round (apply_only: no exchanges, the relabelling alone); thr_local: P.thr_words words per local slot
hipError_t pt_launch_swap(hipStream_t stream, const PtDev &P, uint64_t *thr_local, double *beta_local, bool apply_only);
// out[r] = energy of replica r < n from the measurement counters; the lattice form leaves the counters zeroed
hipError_t lat_launch_energy_from_counts(hipStream_t stream, unsigned long long *meas, uint32_t n, double jabs, long long n_bonds, double *out);
hipError_t pk_launch_energy_from_counts(hipStream_t stream, const unsigned long long *meas, uint32_t first_slot, uint32_t n, double jabs,
                                        double half_directed, double self_energy, double *out);
// the threshold tables of n_groups groups from slot_thr[slot][PK_MAX_DEG], slots at or beyond n_owned taking the last owned one's
hipError_t pk_launch_tables_from_slots(hipStream_t stream, const unsigned long long *slot_thr, uint32_t n_owned, uint32_t n_groups, uint32_t *tabs);

} // namespace isingmc
