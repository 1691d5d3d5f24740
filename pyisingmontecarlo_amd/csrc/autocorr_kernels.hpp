// Spin autocorrelation over time lags ("the lag ring"): exact integer counts between the configurations as they are
// and L stored ones.  A ring holds L snapshots of the state buffer in its own layout, ring u32[L][state words], and the sums
// diff u64[rows][L + 1].  Sample j (0, 1, ... since the last reset), with live = min(j, L) and write_slot = j mod L:
//   for l = 1 .. live:  diff[row][l] += #{sites of the row's replica that differ between now and snapshot acr_slot_of_lag(write_slot, l, L)}
//   then the current configuration becomes snapshot write_slot -- the slot that held lag L, the oldest, once the ring is full.
// ONE launch does both: every word of the slot that is replaced is written by the thread that read it in the same launch (its lag-L
// term comes first in program order), and no other slot is written; nothing else reads the ring.  diff[row][0] is never touched.
// No coupling, bias or random number is read and no state word is written.
// Launch interface of autocorr_kernels.hip (a translation unit of its own: nothing here is instantiated beside the sweep kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "autocorr_ring.hpp"
#include "packed_types.hpp"

namespace isingmc {

constexpr uint32_t ACR_MAX_LAGS = 256;
constexpr uint32_t ACR_LAT_WORDS = 4;    // state words per thread of the checkerboard kernel (a workgroup covers 1024 words)
constexpr uint32_t ACR_PK_ITER = 8;      // positions per thread of the packed kernel (a workgroup covers 2048 positions)
constexpr int ACR_PK_PLANES = 4;         // counts up to ACR_PK_ITER per thread and replica column
constexpr uint32_t ACR_PK_LAG_TILE = 8;  // lags whose 32 column totals a workgroup gathers in LDS before it adds them to the sums

// Checkerboard path (state u32[R][row_words], row_words = 2 wpp: every bit is a site).  A row of diff is a replica.
// R ceil(row_words / 1024) workgroups must stay below 2^31 (hipErrorInvalidValue otherwise).
hipError_t autocorr_launch_lattice(hipStream_t stream, const uint32_t *state, uint32_t *ring, size_t n_replicas, size_t row_words, uint32_t n_lags,
                                   uint32_t live, uint32_t write_slot, unsigned long long *diff);

// Replica-packed paths (state u32[groups][n_pos], replica slot s = bit s & 31 of group s >> 5): the container owns the slots
// [bit0, bit0 + n_owned).  A row of diff is a slot, diff u64[32 groups][L + 1]; the rows of unowned slots stay zero, and padding
// positions (site[p] == PAD_SITE) count for nothing.  The snapshot keeps whole words, unowned bits and padding included.
hipError_t autocorr_launch_packed(hipStream_t stream, const uint32_t *state, uint32_t *ring, const uint32_t *site, uint32_t n_pos, size_t groups,
                                  uint32_t bit0, uint32_t n_owned, uint32_t n_lags, uint32_t live, uint32_t write_slot, unsigned long long *diff);

} // namespace isingmc
