// Kernel of the overlap series: accumulators -> row entries.  See overlap_series_kernels.hpp.
#include "overlap_series_kernels.hpp"

#include <algorithm>

namespace isingmc {

constexpr unsigned OSR_THREADS = 256;
constexpr unsigned long long OSR_MAX_BLOCKS = 4096; // a grid-stride loop covers what is left

// one thread per (column, bin); bins run fastest, so that a wave reads accumulators and writes row entries that lie together
__global__ void __launch_bounds__(OSR_THREADS) osr_store_kernel(const OsrStore S)
{
    const unsigned long long total = S.n_columns * S.bins, stride = (unsigned long long)gridDim.x * OSR_THREADS;
    for (unsigned long long idx = (unsigned long long)blockIdx.x * OSR_THREADS + threadIdx.x; idx < total; idx += stride) {
        const unsigned long long c = idx / S.bins, column = S.column0 + c;
        const uint32_t i = uint32_t(idx - c * S.bins);
        if (column < S.first_column) continue;
        const unsigned long long p = column - S.first_column;
        if (p >= S.n_pairs) continue;
        S.row[p * S.row_stride + S.offset + i] = (long long)S.sizes[i] - 2ll * (long long)S.acc[c * S.acc_stride + i];
    }
}

hipError_t osr_launch_store(hipStream_t stream, const OsrStore &S)
{
    const unsigned long long total = S.n_columns * S.bins;
    if (total == 0) return hipSuccess;
    const unsigned blocks = unsigned(std::min<unsigned long long>((total + OSR_THREADS - 1) / OSR_THREADS, OSR_MAX_BLOCKS));
    hipLaunchKernelGGL(osr_store_kernel, dim3(blocks), dim3(OSR_THREADS), 0, stream, S);
    return hipGetLastError();
}

} // namespace isingmc
