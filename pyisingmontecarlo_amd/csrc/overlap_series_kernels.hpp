// The overlap series: the one kernel that turns the accumulators of an overlap measurement (overlap_kernels.hpp,
// overlap_class_kernels.hpp) into the entries of a row of the device-resident log, so that no measurement has to come back to the
// host to be finished.  An accumulator counts the sites (bonds) at which the two replicas of a pair differ; the entry is
//   size - 2 * count          (nvars - 2 D, n_edges - 2 B, sizes[t][c] - 2 D[t][c])
// the exact integer isingmc_overlaps / isingmc_overlaps_by_class return.  Launch interface of overlap_series_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace isingmc {

// One batch of accumulator columns into one row.  Column c of the batch is column `column0 + c` of the whole measurement -- a pair
// of the call, or one of the 16 pair columns of a replica group / 32 pair columns of a pair block, which need not exist -- and holds
// `bins` counts at acc[c * acc_stride ...].  Pair p of the row is column `first_column + p`; columns before it or from
// first_column + n_pairs on are skipped.  Written: row[p * row_stride + offset + i] = sizes[i] - 2 acc[c * acc_stride + i] for
// i < bins.  Nothing else of the row is touched, and the accumulators are read only.
struct OsrStore {
    const unsigned long long *acc;
    const unsigned long long *sizes; // [bins] (device)
    long long *row;
    unsigned long long column0, first_column, n_columns, n_pairs;
    uint32_t acc_stride, bins, row_stride, offset;
};

hipError_t osr_launch_store(hipStream_t stream, const OsrStore &S);

} // namespace isingmc
