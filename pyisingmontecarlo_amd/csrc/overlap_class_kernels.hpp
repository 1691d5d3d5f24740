// Spin overlaps resolved by a class label per site: for a pair (a, b) with d_i = s_i^a xor s_i^b the kernels count
//   D[t][c] = sites i with cls[t][i] == c and d_i = 1            (out[t][c] = size[t][c] - 2 D[t][c], formed by the host)
// into 64-bit accumulators, ZERO on entry.  Nothing is read but the configurations and the class layouts below, nothing is
// written but the accumulators.  Launch interface of overlap_class_kernels.hip (a translation unit of its own, as
// overlap_kernels.hip is: nothing here is instantiated beside the tuned sweep kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "overlap_kernels.hpp"

namespace isingmc {

constexpr uint32_t OVC_NO_CLASS = 0xFFFFFFFFu; // == ISINGMC_NO_CLASS
constexpr uint32_t OVC_MIXED = 0xFFFFFFFEu;    // word_cls: the 32 sites of the word do not share one class
constexpr uint32_t OVC_MAX_BINS = 8192;        // n_tables * n_classes: the checkerboard kernels' histogram, 32 KiB of LDS

// Checkerboard path: the tables in plane order.
//   cls[t][plane][w][bit]   the class of the site at bit `bit` of word w of colour plane `plane`: one 128-byte line per word
//   word_cls[t][plane][w]   the class all 32 sites of that word share (OVC_NO_CLASS: none of them is counted), or OVC_MIXED
struct LatClassDev {
    const uint32_t *cls;
    const uint32_t *word_cls;
    uint32_t n_tables, n_classes;
};

// slots_a == nullptr: pair p = replicas (2 p, 2 p + 1) of state_a; else replica slots_a[p] of state_a and slots_b[p] of state_b
// (device tables).  out[n_pairs][n_tables][n_classes].  n_pairs <= 32768.
hipError_t overlap_class_launch_lattice(hipStream_t stream, const uint32_t *state_a, const uint32_t *state_b, const uint32_t *slots_a,
                                        const uint32_t *slots_b, const LatGeom &g, const LatClassDev &C, uint32_t n_pairs,
                                        unsigned long long *out);

// Replica-packed families: the positions of every table sorted by class and cut into segments (host_logic.hpp class_segments).
struct PkClassDev {
    const uint32_t *order; // positions, class after class, table after table
    const uint4 *seg;      // {table, class, first, count}: order[first, first + count) are positions of that class, count <= 1024
    uint32_t n_seg;
    uint32_t n_tables, n_classes;
};

// words: [items][n_pos].  paired: the state words of replica groups, pair column j = bits (2 j, 2 j + 1), 16 columns per item; else
// gathered overlap words (overlap_launch_packed_gather), 32 columns per item.  out[items][columns][n_tables][n_classes].
// items <= 32768.
hipError_t overlap_class_launch_packed(hipStream_t stream, const uint32_t *words, uint32_t n_pos, bool paired, const PkClassDev &C,
                                       uint32_t items, unsigned long long *out);

} // namespace isingmc
