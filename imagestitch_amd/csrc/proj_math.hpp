// proj_math.hpp — float32 sinf, cosf, atan2f, atanf and acosf in plain C++ that the host compiler and the device compiler both take, and the
// two maps of the fisheye and the stereographic projector (cv::detail::FisheyeProjector / StereographicProjector, OpenCV 3.4.x
// warpers_inl.hpp - recalled, UNPINNED) written with them.  A kernel cannot call the host's libm and v_sin_f32 / v_cos_f32 are not
// reproducible against a model, so the five calls are restated: each widens its float argument to double (exact), runs a fixed sequence of
// double + - * / sqrt operations - IEEE on host and device alike, no contraction (-ffp-contract=off) - and rounds to float ONCE.  The result
// is within one ulp of the correctly rounded value (DESIGN.md §8 "Fisheye and stereographic projectors" has the measured table) and the same
// bits everywhere.  tests/helpers/polar_np.py repeats every function operation for operation; isx_selftest_proj_math runs the host
// compilation and isx_selftest_proj_math_device the device compilation.  Internal.
//   sinf, cosf  |x| <= 2^28: k = rint(x 2 / pi), r = (x - k P1) - k P1T with P1 the first 25 bits of pi / 2 (k P1 is exact), FreeBSD's
//               k_sinf.c / k_cosf.c polynomials on |r| <= pi / 4.  Beyond 2^28, for an infinity and for a NaN: NaN - the defined fallback
//               (mapBackward then fails its z > 0 test and writes the (-1, -1) sentinel).
//   atanf       fdlibm's s_atan.c: break points 7/16, 11/16, 19/16, 39/16, one division, 11 coefficients; selects, no branch.
//   atan2f      NaN -> NaN; y == 0 -> +-0 or +-pi by the sign BIT of x; x == 0 -> +-pi / 2; both infinite -> +-pi / 4, +-3 pi / 4; else
//               atan(|y / x|), pi - that for x < 0, with the sign of y.
//   acosf       |x| > 1 or NaN -> NaN; else bundle_math.hpp's bm_acos rounded to float.
#pragma once
#include <cmath>

#include "bundle_math.hpp"

namespace isxpm {

constexpr float PM_PI_F = (float)3.1415926535897932384626433832795;
constexpr double PM_RND = 6755399441055744.0;               // 1.5 * 2^52: (t + PM_RND) - PM_RND is t rounded to an integer, ties to even
constexpr double PM_INVPIO2 = 6.36619772367581382433e-01;
constexpr double PM_PIO2_1 = 1.57079631090164184570e+00;    // the first 25 bits of pi / 2
constexpr double PM_PIO2_1T = 1.58932547735281966916e-08;   // pi / 2 - PM_PIO2_1
constexpr float PM_TRIG_MAX = 268435456.f;                  // 2^28
constexpr double PM_PI = 3.14159265358979311600e+00, PM_PIO2 = 1.57079632679489655800e+00, PM_PIO4 = 7.85398163397448278999e-01,
                 PM_3PIO4 = 2.35619449019234483700e+00;

ISX_HD inline float pm_nan() { return __builtin_nanf(""); }

ISX_HD inline double pm_ksin(double r) {
    const double z = r * r, w = z * z;
    const double t = -0.000198393348360966317347 + (z * 0.0000027183114939898219064);
    const double s = z * r;
    return (r + (s * (-0.166666666416265235595 + (z * 0.0083333293858894631756)))) + ((s * w) * t);
}
ISX_HD inline double pm_kcos(double r) {
    const double z = r * r, w = z * z;
    const double t = -0.00138867637746099294692 + (z * 0.0000243904487962774090654);
    return ((1.0 + (z * -0.499999997251031003120)) + (w * 0.0416666233237390631894)) + ((w * z) * t);
}
// sinf and cosf of one argument share the reduction and both polynomials
ISX_HD inline void pm_sincosf(float xf, float& sn, float& cs) {
    const bool ok = __builtin_fabsf(xf) <= PM_TRIG_MAX;                // false for a NaN
    const double x = ok ? (double)xf : 0.0;
    const double k = ((x * PM_INVPIO2) + PM_RND) - PM_RND;
    const double r = (x - (k * PM_PIO2_1)) - (k * PM_PIO2_1T);
    const double q = k - (4.0 * (((k * 0.25) + PM_RND) - PM_RND));       // k modulo 4 as one of -2 .. 2
    const double s = pm_ksin(r), c = pm_kcos(r);
    const double sd = q == 0.0 ? s : (q == 1.0 ? c : (q == -1.0 ? -c : -s));
    const double cd = q == 0.0 ? c : (q == 1.0 ? -s : (q == -1.0 ? s : -c));
    sn = ok ? (float)sd : pm_nan();
    cs = ok ? (float)cd : pm_nan();
}
ISX_HD inline float pm_sinf(float x) { float s, c; pm_sincosf(x, s, c); return s; }
ISX_HD inline float pm_cosf(float x) { float s, c; pm_sincosf(x, s, c); return c; }

// atan of a >= 0 (an infinity included) in double
ISX_HD inline double pm_atan_d(double a) {
    double n = a, d = 1.0, hi = 0.0;
    if (a >= 0.4375) { n = (2.0 * a) - 1.0; d = 2.0 + a; hi = 4.63647609000806093515e-01; }
    if (a >= 0.6875) { n = a - 1.0; d = a + 1.0; hi = 7.85398163397448278999e-01; }
    if (a >= 1.1875) { n = a - 1.5; d = 1.0 + (1.5 * a); hi = 9.82793723247329054082e-01; }
    if (a >= 2.4375) { n = -1.0; d = a; hi = 1.57079632679489655800e+00; }
    const double t = n / d;
    const double z = t * t, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + (w * (1.42857142725034663711e-01 + (w * (9.09088713343650656196e-02 + (w * (6.66107313738753120669e-02 +
                      (w * (4.97687799461593236017e-02 + (w * 1.62858201153657823623e-02))))))))));
    const double s2 = w * (-1.99999999998764832476e-01 + (w * (-1.11111104054623557880e-01 + (w * (-7.69187620504482999495e-02 + (w * (-5.83357013379057348645e-02 +
                      (w * -3.65315727442169155270e-02))))))));
    return hi - ((t * (s1 + s2)) - t);
}
ISX_HD inline float pm_atanf(float x) {
    if (x != x) return pm_nan();
    return (float)__builtin_copysign(pm_atan_d(__builtin_fabs((double)x)), (double)x);
}
ISX_HD inline float pm_atan2f(float yf, float xf) {
    if (xf != xf || yf != yf) return pm_nan();
    const double y = (double)yf, x = (double)xf;
    double r;
    if (y == 0.0) r = __builtin_signbit(x) ? PM_PI : 0.0;
    else if (x == 0.0) r = PM_PIO2;
    else if (__builtin_isinf(x) && __builtin_isinf(y)) r = x > 0.0 ? PM_PIO4 : PM_3PIO4;
    else {
        const double t = pm_atan_d(__builtin_fabs(y / x));
        r = x < 0.0 ? PM_PI - t : t;
    }
    return (float)__builtin_copysign(r, y);
}
ISX_HD inline float pm_acosf(float x) {
    if (!(__builtin_fabsf(x) <= 1.f)) return pm_nan();
    return (float)isxbm::bm_acos((double)x);
}

// ---- the two projectors ---------------------------------------------------------------------------------------------------------------------
// FisheyeProjector / StereographicProjector::mapForward: every float operation rounded on its own, in the order written
template <bool STEREO>
ISX_HD inline void pm_map_forward(const float* r_kinv, float scale, float x, float y, float& u, float& v) {
    const float x_ = r_kinv[0] * x + r_kinv[1] * y + r_kinv[2];
    const float y_ = r_kinv[3] * x + r_kinv[4] * y + r_kinv[5];
    const float z_ = r_kinv[6] * x + r_kinv[7] * y + r_kinv[8];
    const float u_ = pm_atan2f(x_, z_);
    const float v_ = PM_PI_F - pm_acosf(y_ / sqrtf(x_ * x_ + y_ * y_ + z_ * z_));
    float su, cu;
    pm_sincosf(u_, su, cu);
    if (STEREO) {
        float sv, cv;
        pm_sincosf(v_, sv, cv);
        const float r = sv / (1.f - cv);
        u = scale * r * cu;
        v = scale * r * su;
    } else {
        u = scale * v_ * cu;
        v = scale * v_ * su;
    }
}
// mapBackward, with the z > 0 test and the (-1, -1) sentinel of W:56-61
template <bool STEREO>
ISX_HD inline void pm_map_backward(const float* k_rinv, float scale, float u, float v, float& x, float& y) {
    u /= scale;
    v /= scale;
    const float u_ = pm_atan2f(v, u);
    const float r = sqrtf(u * u + v * v);
    const float v_ = STEREO ? 2.f * pm_atanf(1.f / r) : r;
    float sinv, cosv, su, cu;
    pm_sincosf(PM_PI_F - v_, sinv, cosv);
    pm_sincosf(u_, su, cu);
    const float x_ = sinv * su, y_ = cosv, z_ = sinv * cu;
    x = k_rinv[0] * x_ + k_rinv[1] * y_ + k_rinv[2] * z_;
    y = k_rinv[3] * x_ + k_rinv[4] * y_ + k_rinv[5] * z_;
    const float z = k_rinv[6] * x_ + k_rinv[7] * y_ + k_rinv[8] * z_;
    if (z > 0) { x /= z; y /= z; }
    else x = y = -1;
}

}  // namespace isxpm
