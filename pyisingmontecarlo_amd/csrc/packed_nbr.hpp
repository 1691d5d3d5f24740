// Neighbour accessors of the two replica-packed families for the cluster kernels that read no coupling (S12:
// packed_icm_kernels.hip, S13: packed_between_kernels.hip): position of the neighbour in adjacency slot k of position p when p
// owns that bond (the neighbour's position is above p), else a position that is never above p.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "packed_types.hpp"

namespace isingmc {

struct PkNbr { // bit-sliced family: PK_MAX_DEG slots, PK_NO_NBR in unused ones, the coupling's sign in bit 31
    const uint32_t *nbr_ell;
    uint32_t n_pos;
    __device__ __forceinline__ uint32_t slots() const { return uint32_t(PK_MAX_DEG); }
    __device__ __forceinline__ uint32_t operator()(uint32_t k, uint32_t p) const
    {
        const uint32_t x = nbr_ell[size_t(k) * n_pos + p];
        return x == PK_NO_NBR ? 0u : x & 0x7FFFFFFFu;
    }
};
struct RjNbr { // real-coupling family: n_slots slots, the own position in unused ones
    const uint32_t *nbr;
    uint32_t n_pos, n_slots;
    __device__ __forceinline__ uint32_t slots() const { return n_slots; }
    __device__ __forceinline__ uint32_t operator()(uint32_t k, uint32_t p) const { return nbr[size_t(k) * n_pos + p]; }
};

} // namespace isingmc
