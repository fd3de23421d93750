// bundle_math.hpp — the per-camera arithmetic of BundleAdjusterRay (W:189-194) in plain C++ that the host compiler and the device compiler
// both take: sin, cos and acos restated in + - * / sqrt (the Levenberg-Marquardt loop of bundle.hip ends on comparisons at rounding level, so
// a library sin that differs by an ulp between host, device and model would change its length), cvRodrigues2 in both directions, the polar
// factor of setUpInitialCameraParams, R * K.inv() and the ray of calcError.  tests/helpers/bundle_np.py repeats every function operation for
// operation (DESIGN.md §8 "Bundle adjuster"); isx_selftest_bundle_math runs the host compilation and isx_selftest_bundle_math_device the
// device compilation of every function here, item by item (tests/test_gpu_bundle_math.py).  Every expression is evaluated as written,
// left to right, no contraction (-ffp-contract=off).  Also here: the edge matrix and the two residuals of BundleAdjusterReproj's calcError
// (tests/helpers/bundle_reproj_np.py), and the 3 x 3 Jacobi as a template, run in float32 by the wave correction.  Internal.
#pragma once
#include <cfloat>
#include <cmath>

#include "mat3.hpp"

namespace isxbm {

// ---- sin, cos, acos: absolute error below 1e-12 on |x| <= 4 pi (acos: on [-1, 1]) -------------------------------------------------------
// The polynomials and constants are fdlibm's (k_sin.c, k_cos.c, e_acos.c, e_rem_pio2.c); the reduction is its two-constant Cody-Waite step,
// exact for the |k| <= 2^20 quarter turns a rotation vector can reach.  Past 2^51 the result is meaningless but the same everywhere; a NaN
// gives a NaN.
constexpr double BM_RND = 6755399441055744.0;               // 1.5 * 2^52: (t + BM_RND) - BM_RND is t rounded to an integer, ties to even
constexpr double BM_INVPIO2 = 6.36619772367581382433e-01;   // 2 / pi
constexpr double BM_PIO2_1 = 1.57079632673412561417e+00;    // the first 33 bits of pi / 2
constexpr double BM_PIO2_1T = 6.07710050650619224932e-11;   // pi / 2 - BM_PIO2_1
constexpr double BM_PIO2_HI = 1.57079632679489655800e+00, BM_PIO2_LO = 6.12323399573676603587e-17, BM_PI = 3.14159265358979311600e+00;

ISX_HD inline double bm_ksin(double x) {
    const double z = x * x;
    const double p = -1.66666666666666324348e-01 + (z * (8.33333333332248946124e-03 + (z * (-1.98412698298579493134e-04 + (z * (2.75573137070700676789e-06 +
                     (z * (-2.50507602534068634195e-08 + (z * 1.58969099521155010221e-10)))))))));
    return x + ((x * z) * p);
}
ISX_HD inline double bm_kcos(double x) {
    const double z = x * x;
    const double p = 4.16666666666666019037e-02 + (z * (-1.38888888888741095749e-03 + (z * (2.48015872894767294178e-05 + (z * (-2.75573143513906633035e-07 +
                     (z * (2.08757232129817482790e-09 + (z * -1.13596475577881948265e-11)))))))));
    return (1.0 - (0.5 * z)) + ((z * z) * p);
}
// x = k (pi / 2) + r with |r| <= pi / 4 (and a little); q: k modulo 4 as one of -2 .. 2
ISX_HD inline void bm_reduce(double x, double& r, double& q) {
    const double k = ((x * BM_INVPIO2) + BM_RND) - BM_RND;
    r = (x - (k * BM_PIO2_1)) - (k * BM_PIO2_1T);
    q = k - (4.0 * (((k * 0.25) + BM_RND) - BM_RND));
}
ISX_HD inline double bm_sin(double x) {
    double r, q;
    bm_reduce(x, r, q);
    if (q == 0.0) return bm_ksin(r);
    if (q == 1.0) return bm_kcos(r);
    if (q == -1.0) return -bm_kcos(r);
    return -bm_ksin(r);
}
ISX_HD inline double bm_cos(double x) {
    double r, q;
    bm_reduce(x, r, q);
    if (q == 0.0) return bm_kcos(r);
    if (q == 1.0) return -bm_ksin(r);
    if (q == -1.0) return bm_ksin(r);
    return -bm_kcos(r);
}
ISX_HD inline double bm_asin_r(double z) {                  // fdlibm's rational R(z) of asin(x) = x + x R(x^2)
    const double p = z * (1.66666666666666657415e-01 + (z * (-3.25565818622400915405e-01 + (z * (2.01212532134862925881e-01 + (z * (-4.00555345006794114027e-02 +
                     (z * (7.91534994289814532176e-04 + (z * 3.47933107596021167570e-05))))))))));
    const double q = 1.0 + (z * (-2.40339491173441421878e+00 + (z * (2.02094576023350569471e+00 + (z * (-6.88283971605453293030e-01 + (z * 7.70381505559019352791e-02)))))));
    return p / q;
}
ISX_HD inline double bm_acos(double x) {                    // x in [-1, 1]
    if (x < 0.5 && x > -0.5) return BM_PIO2_HI - (x - (BM_PIO2_LO - (x * bm_asin_r(x * x))));
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double s = sqrt(z);
        return BM_PI - (2.0 * (s + ((bm_asin_r(z) * s) - BM_PIO2_LO)));
    }
    const double z = (1.0 - x) * 0.5;
    const double s = sqrt(z);
    return 2.0 * (s + (bm_asin_r(z) * s));
}

// ---- cvRodrigues2, vector -> matrix: theta = |r|; below DBL_EPSILON the identity; else c I + (1 - c) r r^T + s [r]x with r / theta --------
ISX_HD inline void bm_rodrigues_mat(const double* rv, double* R) {
    const double theta = sqrt(((rv[0] * rv[0]) + (rv[1] * rv[1])) + (rv[2] * rv[2]));
    if (theta < DBL_EPSILON) {
        R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
        return;
    }
    const double c = bm_cos(theta), s = bm_sin(theta), c1 = 1.0 - c;
    const double x = rv[0] / theta, y = rv[1] / theta, z = rv[2] / theta;
    R[0] = (c + (c1 * (x * x)));            R[1] = ((c1 * (x * y)) + (s * (-z)));   R[2] = ((c1 * (x * z)) + (s * y));
    R[3] = ((c1 * (x * y)) + (s * z));      R[4] = (c + (c1 * (y * y)));            R[5] = ((c1 * (y * z)) + (s * (-x)));
    R[6] = ((c1 * (x * z)) + (s * (-y)));   R[7] = ((c1 * (y * z)) + (s * x));      R[8] = (c + (c1 * (z * z)));
}

// ---- cvRodrigues2, matrix -> vector, on a matrix that is already a rotation (its own SVD is not repeated) ---------------------------------
ISX_HD inline void bm_rodrigues_vec(const double* R, double* rv) {
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt((((rx * rx) + (ry * ry)) + (rz * rz)) * 0.25);
    double c = (((R[0] + R[4]) + R[8]) - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    double theta = bm_acos(c);
    if (s < 1e-5) {
        if (c > 0) {
            rx = 0.0; ry = 0.0; rz = 0.0;
        } else {
            double t = (R[0] + 1.0) * 0.5;
            rx = sqrt(t < 0.0 ? 0.0 : t);
            t = (R[4] + 1.0) * 0.5;
            ry = sqrt(t < 0.0 ? 0.0 : t) * (R[1] < 0 ? -1.0 : 1.0);
            t = (R[8] + 1.0) * 0.5;
            rz = sqrt(t < 0.0 ? 0.0 : t) * (R[2] < 0 ? -1.0 : 1.0);
            if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != ((ry * rz) > 0)) rz = -rz;
            theta = theta / sqrt(((rx * rx) + (ry * ry)) + (rz * rz));
            rx = rx * theta; ry = ry * theta; rz = rz * theta;
        }
    } else {
        const double vth = theta / (2.0 * s);
        rx = rx * vth; ry = ry * vth; rz = rz * vth;
    }
    rv[0] = rx; rv[1] = ry; rv[2] = rz;
}

// ---- JacobiImpl_ at n = 3 (homography_lm_np.jacobi_n): A's upper triangle is read and destroyed; W descending with the rows of V ----------
ISX_HD inline double bm_fabs(double v) { return fabs(v); }
ISX_HD inline float bm_fabs(float v) { return fabsf(v); }
ISX_HD inline double bm_sqrt(double v) { return sqrt(v); }
ISX_HD inline float bm_sqrt(float v) { return sqrtf(v); }
template <class T>
ISX_HD inline T bm_hypot_t(T a, T b) {
    a = bm_fabs(a); b = bm_fabs(b);
    if (a > b) { b /= a; return a * bm_sqrt(T(1) + (b * b)); }
    if (b > 0) { a /= b; return b * bm_sqrt(T(1) + (a * a)); }
    return T(0);
}
template <class T>
ISX_HD inline void bm_jacobi3_t(T* A, T* V, T* W, T eps) {
    constexpr int n = 3;
    int indR[n] = {0, 0, 0}, indC[n] = {0, 0, 0};
    for (int i = 0; i < n * n; ++i) V[i] = T(0);
    for (int i = 0; i < n; ++i) V[i * n + i] = T(1);
    for (int k = 0; k < n; ++k) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) {
            int m = k + 1;
            T mv = bm_fabs(A[n * k + m]);
            for (int i = k + 2; i < n; ++i) { const T val = bm_fabs(A[n * k + i]); if (mv < val) { mv = val; m = i; } }
            indR[k] = m;
        }
        if (k > 0) {
            int m = 0;
            T mv = bm_fabs(A[k]);
            for (int i = 1; i < k; ++i) { const T val = bm_fabs(A[n * i + k]); if (mv < val) { mv = val; m = i; } }
            indC[k] = m;
        }
    }
    for (int iters = 0; iters < n * n * 30; ++iters) {
        int k = 0;
        T mv = bm_fabs(A[indR[0]]);
        for (int i = 1; i < n - 1; ++i) { const T val = bm_fabs(A[n * i + indR[i]]); if (mv < val) { mv = val; k = i; } }
        int l = indR[k];
        for (int i = 1; i < n; ++i) { const T val = bm_fabs(A[n * indC[i] + i]); if (mv < val) { mv = val; k = indC[i]; l = i; } }
        const T p = A[n * k + l];
        if (bm_fabs(p) <= eps) break;
        const T y = (W[l] - W[k]) * T(0.5);
        T t = bm_fabs(y) + bm_hypot_t(p, y);
        T s = bm_hypot_t(p, t);
        const T c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { s = -s; t = -t; }
        A[n * k + l] = T(0);
        W[k] = W[k] - t;
        W[l] = W[l] + t;
#define BM_ROT(i0, i1, M) do { const T a0 = M[i0], b0 = M[i1]; M[i0] = (a0 * c) - (b0 * s); M[i1] = (a0 * s) + (b0 * c); } while (0)
        for (int i = 0; i < k; ++i) BM_ROT(n * i + k, n * i + l, A);
        for (int i = k + 1; i < l; ++i) BM_ROT(n * k + i, n * i + l, A);
        for (int i = l + 1; i < n; ++i) BM_ROT(n * k + i, n * l + i, A);
        for (int i = 0; i < n; ++i) BM_ROT(n * k + i, n * l + i, V);
#undef BM_ROT
        for (int j = 0; j < 2; ++j) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                int m = idx + 1;
                T mx = bm_fabs(A[n * idx + m]);
                for (int i = idx + 2; i < n; ++i) { const T val = bm_fabs(A[n * idx + i]); if (mx < val) { mx = val; m = i; } }
                indR[idx] = m;
            }
            if (idx > 0) {
                int m = 0;
                T mx = bm_fabs(A[idx]);
                for (int i = 1; i < idx; ++i) { const T val = bm_fabs(A[n * i + idx]); if (mx < val) { mx = val; m = i; } }
                indC[idx] = m;
            }
        }
    }
    for (int k = 0; k < n - 1; ++k) {
        int m = k;
        for (int i = k + 1; i < n; ++i)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            const T w = W[m]; W[m] = W[k]; W[k] = w;
            for (int i = 0; i < n; ++i) { const T v = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = v; }
        }
    }
}

ISX_HD inline void bm_jacobi3(double* A, double* V, double* W) { bm_jacobi3_t<double>(A, V, W, DBL_EPSILON); }
// cv::eigen of a CV_32F 3 x 3: the same in float32, the threshold FLT_EPSILON (waveCorrect)
ISX_HD inline void bm_jacobi3f(float* A, float* V, float* W) { bm_jacobi3_t<float>(A, V, W, FLT_EPSILON); }

// ---- svd(R); R = u * vt; if det < 0: R = -R, as the polar factor R V diag(1 / sqrt(w)) V^T of R^T R = V diag(w) V^T ------------------------
// false where R^T R is not finite or an eigenvalue is not positive: Q is then the identity.
ISX_HD inline bool bm_polar(const double* R, double* Q) {
    double A[9], V[9], W[3], M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[3 * i + j] = ((R[i] * R[j]) + (R[3 + i] * R[3 + j])) + (R[6 + i] * R[6 + j]);
    bool ok = true;
    for (int e = 0; e < 9; ++e) ok = ok && (fabs(A[e]) <= DBL_MAX);
    if (ok) {
        bm_jacobi3(A, V, W);
        for (int e = 0; e < 3; ++e) ok = ok && (W[e] > 0.0);
    }
    if (!ok) {
        Q[0] = 1.0; Q[1] = 0.0; Q[2] = 0.0; Q[3] = 0.0; Q[4] = 1.0; Q[5] = 0.0; Q[6] = 0.0; Q[7] = 0.0; Q[8] = 1.0;
        return false;
    }
    double d[3];
    for (int e = 0; e < 3; ++e) d[e] = 1.0 / sqrt(W[e]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (((V[i] * d[0]) * V[j]) + ((V[3 + i] * d[1]) * V[3 + j])) + ((V[6 + i] * d[2]) * V[6 + j]);
    es_mul3(R, M, Q);
    const double det = ((Q[0] * ((Q[4] * Q[8]) - (Q[5] * Q[7]))) - (Q[1] * ((Q[3] * Q[8]) - (Q[5] * Q[6])))) + (Q[2] * ((Q[3] * Q[7]) - (Q[4] * Q[6])));
    if (det < 0)
        for (int i = 0; i < 9; ++i) Q[i] = -Q[i];
    return true;
}

// ---- calcError's H = R * K.inv(), K = [[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], R = Rodrigues(p[1 .. 3]), f = p[0] ------------------------
ISX_HD inline void bm_cam_h(const double* p, int width, int height, double* H) {
    double R[9], K[9], Ki[9];
    bm_rodrigues_mat(p + 1, R);
    K[0] = p[0]; K[1] = 0.0; K[2] = (double)width * 0.5;
    K[3] = 0.0; K[4] = p[0]; K[5] = (double)height * 0.5;
    K[6] = 0.0; K[7] = 0.0; K[8] = 1.0;
    es_inv3(K, Ki);
    es_mul3(R, Ki, H);
}
// H (x, y, 1) divided by its length
ISX_HD inline void bm_ray(const double* H, double x, double y, double* r) {
    const double X = ((H[0] * x) + (H[1] * y)) + H[2];
    const double Y = ((H[3] * x) + (H[4] * y)) + H[5];
    const double Z = ((H[6] * x) + (H[7] * y)) + H[8];
    const double len = sqrt(((X * X) + (Y * Y)) + (Z * Z));
    r[0] = X / len; r[1] = Y / len; r[2] = Z / len;
}

// ---- BundleAdjusterReproj's calcError: p = focal, ppx, ppy, aspect, rvec[3] of a camera ------------------------------------------------------
// H = ((K2 * R2.inv()) * R1) * K1.inv(), K = [[f, 0, ppx], [0, f * aspect, ppy], [0, 0, 1]], R = Rodrigues(rvec)
ISX_HD inline void bm_reproj_k(const double* p, double* K) {
    K[0] = p[0]; K[1] = 0.0; K[2] = p[1];
    K[3] = 0.0; K[4] = p[0] * p[3]; K[5] = p[2];
    K[6] = 0.0; K[7] = 0.0; K[8] = 1.0;
}
ISX_HD inline void bm_reproj_h(const double* p1, const double* p2, double* H) {
    double K1[9], K2[9], R1[9], R2[9], K1i[9], R2i[9], A[9], B[9];
    bm_reproj_k(p1, K1);
    bm_reproj_k(p2, K2);
    bm_rodrigues_mat(p1 + 4, R1);
    bm_rodrigues_mat(p2 + 4, R2);
    es_inv3(R2, R2i);
    es_inv3(K1, K1i);
    es_mul3(K2, R2i, A);
    es_mul3(A, R1, B);
    es_mul3(B, K1i, H);
}
// the two residuals of a match: p2 - H (x1, y1, 1) dehomogenised
ISX_HD inline void bm_reproj_err(const double* H, double x1, double y1, double x2, double y2, double* e) {
    const double X = ((H[0] * x1) + (H[1] * y1)) + H[2];
    const double Y = ((H[3] * x1) + (H[4] * y1)) + H[5];
    const double Z = ((H[6] * x1) + (H[7] * y1)) + H[8];
    e[0] = x2 - (X / Z); e[1] = y2 - (Y / Z);
}

}  // namespace isxbm
