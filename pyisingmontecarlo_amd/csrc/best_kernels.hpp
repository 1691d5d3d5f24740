// Each replica's lowest-energy configuration, kept on the device.  One update at absolute timestep t, from the f64
// energies e[r] of the current configurations (energies_enqueue):
//   e[r] < best_e[r]  =>  best_e[r] = e[r], best_t[r] = t, best_state[r] = state[r]           (strictly: ties keep the earliest t)
// Records start at +inf, so the first update records every replica.  The decision is one small launch; the conditional copy is one
// launch over the state buffer in which rows (checkerboard) or replica groups (packed) without an improved replica touch no memory.
// Launch interface of best_kernels.hip (a translation unit of its own: nothing here is instantiated beside the tuned sweep
// kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace isingmc {

// One thread per counter slot.  Checkerboard (packed = false): slot = replica r < n, out[r] = 1 / 0.  Packed: slot = (group, bit) of
// n_groups groups, replica r = slot - bit0 when 0 <= r < n (the other bits belong to another shard or to nobody and never improve);
// out[group] = the group's 32-bit mask of improved replicas.  *improved += the number of improved replicas.
hipError_t best_launch_decide(hipStream_t stream, bool packed, const double *energy, uint32_t n, uint32_t bit0, uint32_t n_groups, uint64_t t,
                              double *best_e, unsigned long long *best_t, uint32_t *out, unsigned long long *improved);

// Checkerboard path, state u32[R][state_words]: best[r][:] = state[r][:] where flags[r] != 0.  Moves 16 bytes per thread:
// state_words must be a multiple of 4 and both buffers 16-byte aligned (hipErrorInvalidValue otherwise; every lattice the
// recogniser accepts has state_words = W H / 32 with W a multiple of 64 and H even, a multiple of 8).
hipError_t best_launch_keep_rows(hipStream_t stream, const uint32_t *state, uint32_t *best, const uint32_t *flags, size_t R, size_t state_words);

// Packed paths, state u32[groups][n_pos]: best[g][p] = (best[g][p] & ~m) | (state[g][p] & m) with m = masks[g].  m == 0: the group
// touches no memory; m == every bit of the group this container owns (bit0, n as above): a plain copy, best is not read (the bits
// nobody owns take the state's).  n_pos is a multiple of 256 (the colour classes are padded to it): 16 bytes per thread.
hipError_t best_launch_keep_bits(hipStream_t stream, const uint32_t *state, uint32_t *best, const uint32_t *masks, uint32_t n, uint32_t bit0,
                                 size_t groups, uint32_t n_pos);

} // namespace isingmc
