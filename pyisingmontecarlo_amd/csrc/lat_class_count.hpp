// Counting the set bits of one word stream by site class on the checkerboard path: the device code that the overlap class kernels
// (overlap_class_kernels.hip: the word is sa ^ sb of a pair) and the class kernel of the observable series
// (observable_series_kernels.hip: the word is the configuration itself) share.  A workgroup of 256 threads covers LAT_CLASS_WORDS x 256
// words of each colour plane; the histogram u32[n_tables][n_classes] lives in dynamic LDS (at most OVC_MAX_BINS bins) and is flushed
// with at most one 64-bit atomic per non-zero bin.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "overlap_class_kernels.hpp"

namespace isingmc {

constexpr uint32_t LAT_CLASS_WORDS = 4; // words of each plane per thread (a workgroup covers 1024 words)
// a histogram bin counts at most the sites of both planes' words of one workgroup
static_assert(uint64_t(256) * LAT_CLASS_WORDS * 32 * 2 <= 0xFFFFFFFFull, "the LDS histogram's bins are 32 bits wide");

// word(pw): the word to count at index pw = plane * wpp + w of a replica's planes (and of a table's layout); acc = [n_tables][n_classes].
// Where the word's 32 sites share a class (rows: a word lies inside one row) one LDS atomic of its popcount, else one LDS atomic per
// set bit through the word's 128-byte line of classes.
template <typename Word>
__device__ __forceinline__ void lat_class_count(const Word word, const LatGeom &g, const LatClassDev &C, unsigned long long *__restrict__ acc)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t hist[]; // [n_tables][n_classes]
    const uint32_t bins = C.n_tables * C.n_classes;
    for (uint32_t i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    __syncthreads();
    for (uint32_t i = 0; i < LAT_CLASS_WORDS; i++) {
        const uint32_t w = (blockIdx.x * LAT_CLASS_WORDS + i) * 256 + threadIdx.x;
        if (w >= g.wpp) break;
        for (uint32_t plane = 0; plane < 2; plane++) {
            const uint32_t pw = plane * g.wpp + w;
            const uint32_t d = word(pw);
            if (!d) continue;
            for (uint32_t t = 0; t < C.n_tables; t++) {
                const size_t tw = size_t(t) * 2 * g.wpp + pw;
                uint32_t *h = hist + t * C.n_classes;
                const uint32_t shared = C.word_cls[tw];
                if (shared != OVC_MIXED) {
                    if (shared != OVC_NO_CLASS) atomicAdd(h + shared, uint32_t(__popc(d)));
                    continue;
                }
                const uint32_t *line = C.cls + tw * 32;
                for (uint32_t rest = d; rest; rest &= rest - 1) {
                    const uint32_t c = line[__ffs(rest) - 1];
                    if (c != OVC_NO_CLASS) atomicAdd(h + c, 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < bins; i += 256) {
        const uint32_t total = hist[i];
        if (total) atomicAdd(acc + i, (unsigned long long)total);
    }
}

inline uint32_t lat_class_blocks(const LatGeom &g) { return (g.wpp + 256 * LAT_CLASS_WORDS - 1) / (256 * LAT_CLASS_WORDS); }

} // namespace isingmc
