// Layout of the general edge-list path (general_kernels.hpp) as the host sees it: the padding mark of every position -> site
// table, the device view of the CSR graph, the LDS sizes of the resident kernel.  Plain C++ (host_logic.hpp includes it);
// the launchers are in general_launch.hpp.
#pragma once
#include <cstdint>

namespace isingmc {

constexpr uint32_t PAD_SITE = 0xFFFFFFFFu;

struct GenGraphDev {
    const uint32_t *rowptr;  // n_pos + 1
    const uint32_t *nbr;     // neighbour POSITIONS
    const void *w;           // couplings, float (when lossless) or double
    const double *bias;      // per position, or nullptr (all zero)
    const uint32_t *site;    // original site id per position, PAD_SITE on padding
    const uint32_t *class_base; // n_colours + 1 positions (device copy of the colour-class boundaries)
    uint32_t n_colours;
    uint32_t n_pos;          // multiple of 64
    uint32_t n_words;        // n_pos / 32
};

constexpr uint32_t GEN_RESIDENT_MAX_BYTES = 32 * 1024; // packed state of a replica of gen_resident_kernel

// LDS words the staged variant needs behind the state words (see gen_resident_kernel STAGE); edges2 = directed edges
// stage: 1 = everything, 2 = the topology only (row pointers, site ids, neighbour positions: the links of the dependent chain;
// couplings and biases stay in global memory, their addresses do not depend on loaded data)
inline uint32_t gen_stage_words(uint32_t n_pos, uint32_t edges2, bool has_bias, uint32_t w_bytes, int stage)
{
    uint32_t off = ((n_pos / 32) + 1u) & ~1u;             // state words, then 8-byte alignment
    if (stage == 1) {
        if (has_bias) off += 2 * n_pos;                    // f64 bias per position
        off += edges2 * (w_bytes / 4);                     // couplings (f32 or f64)
        off = (off + 1u) & ~1u;
    }
    return off + (n_pos + 1) + n_pos + edges2;             // rowptr, site, nbr
}

} // namespace isingmc
