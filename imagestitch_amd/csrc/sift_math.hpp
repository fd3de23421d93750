// sift_math.hpp — float32 expf and exp2f in plain C++ that the host compiler and the device compiler both take, beside proj_math.hpp and in
// its style: the float argument is widened to double (exact), a fixed sequence of double + - * / runs - IEEE on host and device alike, no
// contraction (-ffp-contract=off) - and the result is rounded to float ONCE.  One core serves both:
//   k = rint(x / ln 2) (the 1.5 * 2^52 trick), r = (x - k LN2_HI) - k LN2_LO with LN2_HI the first 32 bits of ln 2 (k LN2_HI is exact),
//   exp(r) on |r| <= ln 2 / 2 by the Taylor polynomial of degree 11 in Horner form (its remainder is below 2e-13), times 2^k built from
//   bits ((k + 1023) << 52: exact).
//   pm_expf   NaN -> NaN; x > 89 -> +inf; x < -104 -> 0; else the core on (double)x.
//   pm_exp2f  NaN -> NaN; x > 129 -> +inf; x < -151 -> 0; else the core on (double)x * ln 2.
// The result is within one ulp of the correctly rounded value - measured: DESIGN.md §8 "Features finder, SIFT" has the table - and the same
// bits everywhere.  tests/helpers/sift_np.py repeats both operation for operation; isx_selftest_sift_math runs the host compilation and
// isx_selftest_sift_math_device the device compilation.  Internal.
#pragma once
#include "proj_math.hpp"

namespace isxpm {

constexpr double PM_INV_LN2 = 1.44269504088896338700e+00;
constexpr double PM_LN2_HI = 6.93147180369123816490e-01;    // the first 32 bits of ln 2
constexpr double PM_LN2_LO = 1.90821492927058770002e-10;    // ln 2 - PM_LN2_HI
constexpr double PM_LN2 = 6.93147180559945286227e-01;

// exp of |x| < 700 in double
ISX_HD inline double pm_exp_core(double x) {
    const double k = ((x * PM_INV_LN2) + PM_RND) - PM_RND;
    const double r = (x - (k * PM_LN2_HI)) - (k * PM_LN2_LO);
    double p = 1.0 / 39916800.0;
    p = (1.0 / 3628800.0) + (r * p);
    p = (1.0 / 362880.0) + (r * p);
    p = (1.0 / 40320.0) + (r * p);
    p = (1.0 / 5040.0) + (r * p);
    p = (1.0 / 720.0) + (r * p);
    p = (1.0 / 120.0) + (r * p);
    p = (1.0 / 24.0) + (r * p);
    p = (1.0 / 6.0) + (r * p);
    p = (1.0 / 2.0) + (r * p);
    p = 1.0 + (r * (1.0 + (r * p)));
    const long long bits = ((long long)k + 1023ll) << 52;
    return p * __builtin_bit_cast(double, bits);
}
ISX_HD inline float pm_expf(float x) {
    if (x != x) return pm_nan();
    if (x > 89.f) return __builtin_huge_valf();
    if (x < -104.f) return 0.f;
    return (float)pm_exp_core((double)x);
}
ISX_HD inline float pm_exp2f(float x) {
    if (x != x) return pm_nan();
    if (x > 129.f) return __builtin_huge_valf();
    if (x < -151.f) return 0.f;
    return (float)pm_exp_core((double)x * PM_LN2);
}

}  // namespace isxpm
