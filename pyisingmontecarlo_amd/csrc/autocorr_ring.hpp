// The slot arithmetic of the lag ring, host and device: the one place that says where a lag lives.  Sample j is
// stored in slot j mod L, so with write_slot = j mod L the snapshot of sample j - l (1 <= l <= min(j, L)) is in slot
// (write_slot - l) mod L; lag L is the write slot itself.  Plain C++ (no HIP include): host_logic.cpp builds its plan from it.
#pragma once
#include <cstdint>

#if defined(__HIP__) // (the HIP language mode, with or without the runtime's header: the attributes are the compiler's own)
#define ACR_HD __host__ __device__ inline
#else
#define ACR_HD inline
#endif

namespace isingmc {

ACR_HD uint32_t acr_slot_of_lag(uint32_t write_slot, uint32_t lag, uint32_t n_lags)
{
    return write_slot >= lag ? write_slot - lag : write_slot + n_lags - lag;
}

} // namespace isingmc
