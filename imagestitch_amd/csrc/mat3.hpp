// mat3.hpp — Mat::inv() and Mat * Mat of a 3 x 3 CV_64F as tests/helpers/estimator_np.py restates them (inv3, mul3), in plain C++ that the
// host compiler and the device compiler both take.  estimator.hip and bundle.hip call them; the arithmetic is one text, evaluated as written
// (-ffp-contract=off).  Internal.
#pragma once

#if defined(__HIPCC__)
#define ISX_HD __host__ __device__
#else
#define ISX_HD
#endif

// Mat::inv() of a 3 x 3 CV_64F: cofactors times the reciprocal determinant, nine zeros for a determinant of exactly 0
ISX_HD inline void es_inv3(const double* m, double* t) {
    const double a = (m[4] * m[8]) - (m[5] * m[7]);
    const double b = (m[3] * m[8]) - (m[5] * m[6]);
    const double c = (m[3] * m[7]) - (m[4] * m[6]);
    double d = ((m[0] * a) - (m[1] * b)) + (m[2] * c);
    if (!(d != 0.0)) {
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = 0.0;
        return;
    }
    d = 1.0 / d;
    t[0] = ((m[4] * m[8]) - (m[5] * m[7])) * d; t[1] = ((m[2] * m[7]) - (m[1] * m[8])) * d; t[2] = ((m[1] * m[5]) - (m[2] * m[4])) * d;
    t[3] = ((m[5] * m[6]) - (m[3] * m[8])) * d; t[4] = ((m[0] * m[8]) - (m[2] * m[6])) * d; t[5] = ((m[2] * m[3]) - (m[0] * m[5])) * d;
    t[6] = ((m[3] * m[7]) - (m[4] * m[6])) * d; t[7] = ((m[1] * m[6]) - (m[0] * m[7])) * d; t[8] = ((m[0] * m[4]) - (m[1] * m[3])) * d;
}

ISX_HD inline void es_mul3(const double* a, const double* b, double* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = ((a[3 * r] * b[c]) + (a[3 * r + 1] * b[3 + c])) + (a[3 * r + 2] * b[6 + c]);
}
