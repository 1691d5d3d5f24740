// Neighbour accessors of the two replica-packed families for the kernels that read no coupling (S12: packed_icm_kernels.hip,
// S13: packed_between_kernels.hip, S15: the link overlaps of overlap_kernels.hip): position of the neighbour in adjacency slot k
// of position p when p owns that bond (the neighbour's position is above p), else a position that is never above p.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "packed_types.hpp"

namespace isingmc {

struct PkNbr { // bit-sliced family: PK_MAX_DEG slots, PK_NO_NBR in unused ones, the coupling's sign in bit 31
    const uint32_t *nbr_ell;
    uint32_t n_pos;
    __host__ __device__ __forceinline__ uint32_t slots() const { return uint32_t(PK_MAX_DEG); }
    __device__ __forceinline__ uint32_t operator()(uint32_t k, uint32_t p) const
    {
        const uint32_t x = nbr_ell[size_t(k) * n_pos + p];
        return x == PK_NO_NBR ? 0u : x & 0x7FFFFFFFu;
    }
};
struct RjNbr { // real-coupling family: n_slots slots, the own position in unused ones
    const uint32_t *nbr;
    uint32_t n_pos, n_slots;
    __host__ __device__ __forceinline__ uint32_t slots() const { return n_slots; }
    __device__ __forceinline__ uint32_t operator()(uint32_t k, uint32_t p) const { return nbr[size_t(k) * n_pos + p]; }
};

// launch(accessor) with the accessor of the container's family.  nbr_rj == nullptr: the neighbours of G.nbr_ell; else
// nbr_rj[slot][n_pos] with rj_slots slots.
template <typename LAUNCH>
inline void pk_nbr_dispatch(const PkGraphDev &G, const uint32_t *nbr_rj, uint32_t rj_slots, LAUNCH launch)
{
    if (nbr_rj) launch(RjNbr{nbr_rj, G.n_pos, rj_slots});
    else launch(PkNbr{G.nbr_ell, G.n_pos});
}

} // namespace isingmc
