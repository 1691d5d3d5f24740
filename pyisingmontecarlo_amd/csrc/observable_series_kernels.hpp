// The observable series: the kernels that turn the integer counters of a measurement into the entries of a row of the
// device-resident log -- energy, magnetisation and magnetisation by site class of every column -- so that no measurement has to come
// back to the host to be finished.  Launch interface of observable_series_kernels.hip.
//   energy          the arithmetic of the energy_from_counts kernels of the tempering rounds (energy_from_counts.hpp): the bits of
//                   isingmc_get_energies
//   magnetisation   2 up - nvars
//   by class        2 U[t][c] - size[t][c], U = the up spins among the sites of class c of table t
// A column is a replica slot of the container, or with a permutation (rung -> slot, read here, on the device) a rung of its ladder.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "overlap_class_kernels.hpp"

namespace isingmc {

enum ObsFamily : uint32_t { OBS_LATTICE = 0, OBS_PACKED = 1, OBS_REAL = 2 };

// Counters -> the energy and magnetisation entries of one row.  Column i reads the counter pair of slot
// first_slot + (perm ? perm[i] : i): the energy from cnt_e[2 slot] (OBS_REAL: and cnt_e[2 slot + 1], the two levels), the up spins
// from cnt_u[2 slot + 1].  row_e / row_m: [n_columns], either may be nullptr (its counters are then not read).  The counters are
// read only.
struct ObsStore {
    const unsigned long long *cnt_e, *cnt_u;
    const uint32_t *perm; // device, [n_columns]; nullptr: the identity
    double *row_e;
    long long *row_m;
    uint32_t family, first_slot, n_columns;
    int k_energy;                            // OBS_REAL
    double jabs, half_directed, self_energy; // half_directed: OBS_PACKED
    long long n_bonds, nvars;                // n_bonds: OBS_LATTICE
};
hipError_t obs_launch_store(hipStream_t stream, const ObsStore &S);

// One batch of class counters into one row.  acc: [n_slots][bins] up-spin counts of the slots [slot0, slot0 + n_slots); column i reads
// slot first_slot + (perm ? perm[i] : i) and is skipped when that slot is not in the batch.  Written:
// row[i * bins + b] = 2 acc[slot - slot0][b] - sizes[b].  The launch covers the columns [column0, column0 + n_columns) of the row:
// all of them with a permutation, and without one only those whose slots the batch holds (obs_batch_columns).
struct ObsClassStore {
    const unsigned long long *acc;
    const unsigned long long *sizes; // [bins] (device)
    const uint32_t *perm;
    long long *row;
    unsigned long long slot0, n_slots;
    uint32_t first_slot, column0, n_columns, bins;
};
// without a permutation: the columns of a row of `columns` columns whose slots first_slot + i lie in [slot0, slot0 + n_slots)
inline void obs_batch_columns(unsigned long long slot0, unsigned long long n_slots, uint32_t first_slot, uint32_t columns,
                              uint32_t *column0, uint32_t *n_columns)
{
    const unsigned long long lo = slot0 > first_slot ? slot0 - first_slot : 0;
    const unsigned long long hi = slot0 + n_slots > first_slot ? slot0 + n_slots - first_slot : 0;
    *column0 = uint32_t(lo < columns ? lo : columns);
    *n_columns = uint32_t((hi < columns ? hi : columns) - *column0);
}
hipError_t obs_launch_class_store(hipStream_t stream, const ObsClassStore &S);

// Checkerboard path: the up spins of replicas [0, n) behind `state` (2 wpp words each) by class: out[n][n_tables][n_classes], ZERO on
// entry.  n <= 32768, n_tables * n_classes <= OVC_MAX_BINS.  Nothing is written but the accumulators.
hipError_t obs_launch_lat_class(hipStream_t stream, const uint32_t *state, const LatGeom &g, const LatClassDev &C, uint32_t n,
                                unsigned long long *out);

} // namespace isingmc
