// The deterministic exponential of the device code: shared by the f64 CSR sweep, the tempering exchange and the population
// annealing weights (host twin: det_exp_host in host_logic.cpp; oracle twin: orc_det_exp).
#pragma once
#include <hip/hip_runtime.h>

namespace isingmc {

// exp(x) for x = -beta dE, IEEE f64 ops + fma only (same bits as the oracle's orc_det_exp)
__device__ __forceinline__ double det_exp(double x)
{
    if (x >= 0.0) return 1.0;
    if (x < -40.0) return 0.0; // below 2^-53: can never beat a 53-bit uniform
    const double LOG2E = 1.4426950408889634074;
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double kf = floor(fma(x, LOG2E, 0.5));
    double r = fma(-kf, LN2_HI, x);
    r = fma(-kf, LN2_LO, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const long long k = (long long)kf; // in [-58, 0]
    return p * __longlong_as_double((1023ll + k) << 52);
}

} // namespace isingmc
