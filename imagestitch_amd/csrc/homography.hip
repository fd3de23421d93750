// homography.hip — the second half of BestOf2NearestMatcher::match on gfx950, after the reference's 计算单应性矩阵 demo (R = its
// 计算单应性矩阵.cpp, a hand-unrolled OpenCV 3.4.2 findHomography(RANSAC)):
//   isx_find_homography     R:836-909 for every pair of a matcher call: findHomography2(src, dst, RANSAC, 3, mask, 2000, 0.995) (R:602-693,
//                           RANSACPointSetRegistrator1::run R:139-233, HomographyEstimatorCallback R:253-402), the degenerate-H test,
//                           num_inliers and confidence (R:863-878), the second run on the inliers (R:881-909).  The Levenberg-Marquardt
//                           polish of R:672 is not run.
//   isx_find_homography_lm  the same with the polish (createLMSolver1(HomographyRefineCallback(src, dst), 10)->run(H8), R:404-591) over the
//                           inliers of both passes: the second instantiation of the kernel, opt-in, its OpenCV calls restated (unpinned)
//   isx_homography_release  returns the per-thread scratch
//
// The specification is tests/helpers/homography_np.py, with tests/helpers/homography_lm_np.py for the polish (DESIGN.md §8 "Homography"): float64 in + - * / sqrt only, every sum in the order of
// its loop, the float32 of computeError as written; cv::eigen (JacobiImpl_), cv::RNG, haveCollinearPoints and cvRound are restated there.
// `nmodels = cb->runKernel(ms1, ms2, model)`, which R lost between R:196 and R:197, is in place.
//
// ONE launch per call, however many pairs: k_hg_pairs, one block of one wave per pair, both passes.  The sample stream of a RANSAC run
// depends on the points alone (getSubset and checkSubset), never on the scores, so the wave works in chunks of 64 hypotheses:
//   draw     lane 0 draws the chunk's subsets in order (cv::RNG, the 10000 attempts of getSubset, checkSubset in double);
//   solve    lane h solves hypothesis h: the normalised 9 x 9 system of runKernel and its Jacobi eigen-solve.  The Jacobi state (A, V, W, the
//            pivot tables) is indexed by run-time pivots: it lives in LDS as [element][lane] - with 8-byte elements and 64 lanes the bank
//            depends on the lane alone, so pivots that differ across lanes do not conflict;
//   scan     the hypotheses in order, exactly as the sequential loop: the 64 lanes score one hypothesis against all points (a ballot
//            per 64 points), a better count replaces the model and shortens niters (RANSACUpdateNumIters1), the scan stops at niters.
// The least-squares refit over all inliers gives each of the 45 LtL[j][k] sums (and each of the 4 + 4 mean and scale sums) to a lane of its
// own that loops over the points in order: the bits of the sequential loop without a reduction tree.
#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"

#include <cfloat>

using namespace isx;
using namespace isxd;

namespace {

constexpr int HG_CHUNK = ISX_HOMOGRAPHY_CHUNK;   // hypotheses per chunk = lanes of the block
constexpr int HG_MAX_ATTEMPTS = 10000;           // getSubset(m1, m2, ms1, ms2, rng, 10000), R:189
constexpr int HG_ST_H = 1, HG_ST_PASS2 = 2, HG_ST_PASS2_FAILED = 4, HG_ST_CLAMPED = 8, HG_ST_DEGENERATE = 16;
static_assert(HG_CHUNK == WAVE, "one hypothesis per lane of one wave");

// LDS, in bytes from the start of the dynamic segment: [element][lane]
constexpr int HG_LDS_A = 0;                                  // 81 doubles a lane: the matrix (its upper triangle is what is read)
constexpr int HG_LDS_V = HG_LDS_A + 81 * WAVE * 8;           // 81 doubles: the eigenvectors, one a row
constexpr int HG_LDS_W = HG_LDS_V + 81 * WAVE * 8;           // 9 doubles: the eigenvalues
constexpr int HG_LDS_INDR = HG_LDS_W + 9 * WAVE * 8;         // 9 ints: the column of the largest element right of the diagonal, per row
constexpr int HG_LDS_INDC = HG_LDS_INDR + 9 * WAVE * 4;      // 9 ints: the row of the largest element above the diagonal, per column
constexpr int HG_LDS_SUB = HG_LDS_INDC + 9 * WAVE * 4;       // 4 ints: the subset of hypothesis h
constexpr int HG_LDS_FOUND = HG_LDS_SUB + 4 * WAVE * 4;      // 1 int: getSubset's result for hypothesis h
constexpr int HG_LDS_ATT = HG_LDS_FOUND + WAVE * 4;          // 1 int: its attempts
constexpr int HG_LDS_BYTES = HG_LDS_ATT + WAVE * 4;

struct HgPair {
    const float* points; long long points_step;   // the caller's device mat or the staged copy of a host mat
    unsigned char* mask; long long mask_step;     // the caller's device mat or its staged copy
    float* work_a; float* work_b;                 // cap x 4 floats each: the inliers of pass 1 (the input of pass 2), those of pass 2
    int cap;                                      // min(rows of points, rows of mask)
    int pad;
};

struct HgCall {
    const HgPair* pairs;
    const int* counts;
    double* H; long long H_step;
    int* stats; long long stats_step;
    double* conf;
    double thresh, confidence;
    int max_iters, thresh1, thresh2;
    int lm_max_iters;                             // k_hg_pairs<true> only: maxIters of the LM solver (10 at R:672)
};

struct HgLds {
    double* A; double* V; double* W; int* indR; int* indC; int* sub; int* found; int* att;
};

__device__ __forceinline__ double hg_det3(const double* a) {
    return (a[0] * (a[4] * a[8] - a[7] * a[5]) - a[1] * (a[3] * a[8] - a[6] * a[5])) + a[2] * (a[3] * a[7] - a[6] * a[4]);
}

// OpenCV's own hypot
__device__ __forceinline__ double hg_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1.0 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1.0 + a * a); }
    return 0.0;
}

// JacobiImpl_ on the lane's column of the LDS state, n x n (9 for runKernel, 8 for the LM solve: the elements are [r * n + c][lane]); A is
// set.  Leaves W sorted descending with the rows of V.
template <int n>
__device__ __forceinline__ void hg_jacobi(const HgLds& s, int lane) {
#define HA(r, c) s.A[((r) * n + (c)) * WAVE + lane]
#define HV(r, c) s.V[((r) * n + (c)) * WAVE + lane]
#define HW(r) s.W[(r) * WAVE + lane]
#define HR(r) s.indR[(r) * WAVE + lane]
#define HC(r) s.indC[(r) * WAVE + lane]
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) HV(i, j) = 0.0;
        HV(i, i) = 1.0;
    }
    for (int k = 0; k < n; ++k) {
        HW(k) = HA(k, k);
        if (k < n - 1) {
            int m = k + 1;
            double mv = fabs(HA(k, m));
            for (int i = k + 2; i < n; ++i) {
                const double val = fabs(HA(k, i));
                if (mv < val) { mv = val; m = i; }
            }
            HR(k) = m;
        }
        if (k > 0) {
            int m = 0;
            double mv = fabs(HA(0, k));
            for (int i = 1; i < k; ++i) {
                const double val = fabs(HA(i, k));
                if (mv < val) { mv = val; m = i; }
            }
            HC(k) = m;
        }
    }
    for (int iters = 0; iters < n * n * 30; ++iters) {
        int k = 0;
        double mv = fabs(HA(0, HR(0)));
        for (int i = 1; i < n - 1; ++i) {
            const double val = fabs(HA(i, HR(i)));
            if (mv < val) { mv = val; k = i; }
        }
        int l = HR(k);
        for (int i = 1; i < n; ++i) {
            const double val = fabs(HA(HC(i), i));
            if (mv < val) { mv = val; k = HC(i); l = i; }
        }
        const double p = HA(k, l);
        if (fabs(p) <= DBL_EPSILON) break;
        const double y = (HW(l) - HW(k)) * 0.5;
        double t = fabs(y) + hg_hypot(p, y);
        double sn = hg_hypot(p, t);
        const double c = t / sn;
        sn = p / sn; t = (p / t) * p;
        if (y < 0) { sn = -sn; t = -t; }
        HA(k, l) = 0.0;
        HW(k) -= t;
        HW(l) += t;
#define HG_ROT(v0, v1)                              \
    do {                                            \
        const double a0 = v0, b0 = v1;              \
        v0 = a0 * c - b0 * sn;                      \
        v1 = a0 * sn + b0 * c;                      \
    } while (0)
        for (int i = 0; i < k; ++i) HG_ROT(HA(i, k), HA(i, l));
        for (int i = k + 1; i < l; ++i) HG_ROT(HA(k, i), HA(i, l));
        for (int i = l + 1; i < n; ++i) HG_ROT(HA(k, i), HA(l, i));
        for (int i = 0; i < n; ++i) HG_ROT(HV(k, i), HV(l, i));
#undef HG_ROT
        for (int j = 0; j < 2; ++j) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                int m = idx + 1;
                double mx = fabs(HA(idx, m));
                for (int i = idx + 2; i < n; ++i) {
                    const double val = fabs(HA(idx, i));
                    if (mx < val) { mx = val; m = i; }
                }
                HR(idx) = m;
            }
            if (idx > 0) {
                int m = 0;
                double mx = fabs(HA(0, idx));
                for (int i = 1; i < idx; ++i) {
                    const double val = fabs(HA(i, idx));
                    if (mx < val) { mx = val; m = i; }
                }
                HC(idx) = m;
            }
        }
    }
    for (int k = 0; k < n - 1; ++k) {
        int m = k;
        for (int i = k + 1; i < n; ++i)
            if (HW(m) < HW(i)) m = i;
        if (k != m) {
            const double w = HW(m); HW(m) = HW(k); HW(k) = w;
            for (int i = 0; i < n; ++i) { const double v = HV(m, i); HV(m, i) = HV(k, i); HV(k, i) = v; }
        }
    }
#undef HA
#undef HV
#undef HW
#undef HR
#undef HC
}

// R:369-371 from row 8 of the lane's sorted V: H = (invHnorm * H0 * Hnorm2) / that(2, 2), the sums k = 0, 1, 2 left to right
__device__ __forceinline__ void hg_denormalise(const HgLds& s, int lane, const double* inv, const double* hn2, double* H) {
    double h0[9], ht[9], h2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h0[i] = s.V[(8 * 9 + i) * WAVE + lane];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) ht[3 * i + j] = (inv[3 * i] * h0[j] + inv[3 * i + 1] * h0[3 + j]) + inv[3 * i + 2] * h0[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) h2[3 * i + j] = (ht[3 * i] * hn2[j] + ht[3 * i + 1] * hn2[3 + j]) + ht[3 * i + 2] * hn2[6 + j];
    const double sc = 1.0 / h2[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = h2[i] * sc;
}

// runKernel (R:304-373) of the lane's own four correspondences q[i] = (src.x, src.y, dst.x, dst.y); false = it returned 0
__device__ bool hg_run_kernel_lane(const HgLds& s, int lane, const float (&q)[4][4], double* H) {
    constexpr int count = 4;
    double cmx = 0, cmy = 0, cMx = 0, cMy = 0;
#pragma unroll
    for (int i = 0; i < count; ++i) { cmx += q[i][2]; cmy += q[i][3]; cMx += q[i][0]; cMy += q[i][1]; }
    cmx /= count; cmy /= count; cMx /= count; cMy /= count;
    double smx = 0, smy = 0, sMx = 0, sMy = 0;
#pragma unroll
    for (int i = 0; i < count; ++i) {
        smx += fabs(q[i][2] - cmx); smy += fabs(q[i][3] - cmy);
        sMx += fabs(q[i][0] - cMx); sMy += fabs(q[i][1] - cMy);
    }
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    const double inv[9] = {1.0 / smx, 0, cmx, 0, 1.0 / smy, cmy, 0, 0, 1};
    const double hn2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    double acc[45];
#pragma unroll
    for (int e = 0; e < 45; ++e) acc[e] = 0.0;
#pragma unroll
    for (int i = 0; i < count; ++i) {
        const double x = (q[i][2] - cmx) * smx, y = (q[i][3] - cmy) * smy;
        const double X = (q[i][0] - cMx) * sMx, Y = (q[i][1] - cMy) * sMy;
        const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
        const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
        int e = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int k = j; k < 9; ++k, ++e) acc[e] = acc[e] + (Lx[j] * Lx[k] + Ly[j] * Ly[k]);
    }
    {
        int e = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int k = j; k < 9; ++k, ++e) s.A[(j * 9 + k) * WAVE + lane] = acc[e];
    }
    hg_jacobi<9>(s, lane);
    hg_denormalise(s, lane, inv, hn2, H);
    return true;
}

__device__ __forceinline__ double hg_pick(int j, double X, double Y, double x) {      // Lx[j] of R:356
    return j == 0 ? X : j == 1 ? Y : j == 2 ? 1.0 : j < 6 ? 0.0 : j == 6 ? -x * X : j == 7 ? -x * Y : -x;
}
__device__ __forceinline__ double hg_pick_y(int j, double X, double Y, double y) {    // Ly[j] of R:357
    return j < 3 ? 0.0 : j == 3 ? X : j == 4 ? Y : j == 5 ? 1.0 : j == 6 ? -y * X : j == 7 ? -y * Y : -y;
}

// runKernel over `count` dense rows by the whole wave: every sum is one lane's, looping over the rows in order.  The result is uniform.
__device__ bool hg_run_kernel_wave(const HgLds& s, int lane, const float* pts, long long step, int count, double* H) {
    const int col = (lane & 3) < 2 ? (lane & 3) + 2 : (lane & 3) - 2;      // lanes 0..3: dst.x, dst.y, src.x, src.y (cm.x, cm.y, cM.x, cM.y)
    double sum = 0.0;
    for (int i = 0; i < count; ++i) sum += row_ptr(pts, i, step)[col];
    sum /= count;
    const double cmx = __shfl(sum, 0), cmy = __shfl(sum, 1), cMx = __shfl(sum, 2), cMy = __shfl(sum, 3);
    double sa = 0.0;
    for (int i = 0; i < count; ++i) sa += fabs(row_ptr(pts, i, step)[col] - sum);
    double smx = __shfl(sa, 0), smy = __shfl(sa, 1), sMx = __shfl(sa, 2), sMy = __shfl(sa, 3);
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    const double inv[9] = {1.0 / smx, 0, cmx, 0, 1.0 / smy, cmy, 0, 0, 1};
    const double hn2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    int j = 0, k = lane < 45 ? lane : 0;                  // lane e < 45 owns LtL[j][k], j <= k, in row-major order of the upper triangle
    while (k >= 9 - j) { k -= 9 - j; ++j; }
    k += j;
    double acc = 0.0;
    for (int i = 0; i < count; ++i) {
        const float* r = row_ptr(pts, i, step);
        const double x = (r[2] - cmx) * smx, y = (r[3] - cmy) * smy;
        const double X = (r[0] - cMx) * sMx, Y = (r[1] - cMy) * sMy;
        acc = acc + (hg_pick(j, X, Y, x) * hg_pick(k, X, Y, x) + hg_pick_y(j, X, Y, y) * hg_pick_y(k, X, Y, y));
    }
    __syncthreads();
    if (lane < 45) s.A[(j * 9 + k) * WAVE + 0] = acc;     // lane 0's column
    __syncthreads();
    if (lane == 0) hg_jacobi<9>(s, 0);
    __syncthreads();
    hg_denormalise(s, 0, inv, hn2, H);
    return true;
}

// RANSACUpdateNumIters1 (R:39-59) with modelPoints = 4
__device__ int hg_update_iters(double p, double ep, int max_iters) {
    p = fmax(p, 0.0); p = fmin(p, 1.0);
    ep = fmax(ep, 0.0); ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    double denom = 1.0 - pow(1.0 - ep, 4.0);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

__device__ __forceinline__ bool hg_collinear(const float (&q)[4][4], int c) {      // haveCollinearPoints(m, 4): the last point only
    const double xi = q[3][c], yi = q[3][c + 1];
    for (int j = 0; j < 3; ++j) {
        const double dx1 = q[j][c] - xi, dy1 = q[j][c + 1] - yi;
        for (int k = 0; k < j; ++k) {
            const double dx2 = q[k][c] - xi, dy2 = q[k][c + 1] - yi;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

__device__ bool hg_check_subset(const float (&q)[4][4]) {                         // R:253-288
    if (hg_collinear(q, 0) || hg_collinear(q, 2)) return false;
    const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double a[9], b[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[3 * r] = q[tt[i][r]][0]; a[3 * r + 1] = q[tt[i][r]][1]; a[3 * r + 2] = 1.0;
            b[3 * r] = q[tt[i][r]][2]; b[3 * r + 1] = q[tt[i][r]][3]; b[3 * r + 2] = 1.0;
        }
        negative += hg_det3(a) * hg_det3(b) < 0;
    }
    return negative == 0 || negative == 4;
}

// computeError and findInliers (R:383-402, R:67-86) for one row, in float32 as written
__device__ __forceinline__ bool hg_inlier(const float* Hf, const float* r, float t) {
    const float Mx = r[0], My = r[1];
    const float ww = 1.f / ((Hf[6] * Mx + Hf[7] * My) + 1.f);
    const float dx = ((Hf[0] * Mx + Hf[1] * My) + Hf[2]) * ww - r[2];
    const float dy = ((Hf[3] * Mx + Hf[4] * My) + Hf[5]) * ww - r[3];
    return dx * dx + dy * dy <= t;
}

// rng.uniform(0, n) of cv::RNG: state = (uint64)(unsigned)state * 4294883355u + (unsigned)(state >> 32), the low word modulo n
__device__ __forceinline__ int hg_uniform(unsigned long long& state, int n) {
    state = (unsigned long long)(unsigned)state * 4294883355ull + (state >> 32);
    return (int)((unsigned)state % (unsigned)n);
}

__device__ __forceinline__ void hg_load4(const float* pts, long long step, int i0, int i1, int i2, int i3, float (&q)[4][4]) {
    const int idx[4] = {i0, i1, i2, i3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* r = row_ptr(pts, idx[i], step);
        q[i][0] = r[0]; q[i][1] = r[1]; q[i][2] = r[2]; q[i][3] = r[3];
    }
}

struct HgRun {
    bool ok;            // findHomography2's result: H is not empty
    double H[9];
    int inliers;        // rows compacted into `work`
    int iters, win, attempts;
    int lm_ret, lm_nfj; // LM only: run()'s return value and nfJ (R:580, R:491), 0 where it did not run
};

// ---- the Levenberg-Marquardt polish of R:672 (HomographyRefineCallback R:404-459, LMSolverImpl1::run R:473-581): k_hg_pairs<true> only ----
// Its state lives in the Jacobi's LDS, which no hypothesis uses by then: column 0 of A / V / W / indR / indC is the 8 x 8 Jacobi (Ap of the
// solve, A of the invert), column 1 of A is LM's A (8 x 8, mirrored), column 2 holds v, D, d, x, xd and the invert's maxval.  Nothing past
// HG_LDS_BYTES is used.
#define HG_LA(i, j) s.A[((i) * 8 + (j)) * WAVE + 1]
#define HG_LX(off, i) s.A[((off) + (i)) * WAVE + 2]
#define HG_JA(i, j) s.A[((i) * 8 + (j)) * WAVE]
#define HG_JV(i, j) s.V[((i) * 8 + (j)) * WAVE]
#define HG_JW(i) s.W[(i) * WAVE]
constexpr int HG_LM_V = 0, HG_LM_D = 8, HG_LM_DD = 16, HG_LM_X = 24, HG_LM_XD = 32, HG_LM_MAXVAL = 40;

__device__ __forceinline__ double hg_lm_jx(int i, double a, double b, double ww, double g6, double g7) {      // Jptr[i] of R:444-446
    return i == 0 ? a : i == 1 ? b : i == 2 ? ww : i < 6 ? 0.0 : i == 6 ? g6 : g7;
}
__device__ __forceinline__ double hg_lm_jy(int i, double a, double b, double ww, double g6, double g7) {      // Jptr[8 + i] of R:447-449
    return i < 3 ? 0.0 : i == 3 ? a : i == 4 ? b : i == 5 ? ww : i == 6 ? g6 : g7;
}

// compute (R:432-453) at the parameters HG_LX(xoff, .) over the m rows of `work`.  Every lane walks the rows in order and keeps
// norm(err, NORM_L2SQR) (groups of four, then one by one) and norm(err, NORM_INF): both are uniform without a broadcast.  With J, lane
// e < 36 also owns A[i][j] of mulTransposed(J, A, true) (i <= j, the upper triangle in row-major order) and lane 36 + i owns v[i] of
// gemm(J, r, GEMM_1_T): each is one lane's sum over the rows 2p, 2p + 1 in order, zero products included, from +0.0.
template <bool J>
__device__ void hg_lm_eval(const HgLds& s, int lane, const float* work, int m, int xoff, double& S, double& rinf) {
    double h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = HG_LX(xoff, i);
    const bool isA = lane < 36, isV = lane >= 36 && lane < 44;
    int i = 0, j = 0;
    if (isA) {
        j = lane;
        while (j >= 8 - i) { j -= 8 - i; ++i; }
        j += i;
    } else if (isV) {
        i = lane - 36;
    }
    double acc = 0.0, sum = 0.0, grp = 0.0, mx = 0.0;
    for (int p = 0; p < m; ++p) {
        const float* r = work + 4ll * p;
        const double Mx = r[0], My = r[1];
        double ww = (h[6] * Mx + h[7] * My) + 1.;
        ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0.;
        const double xi = ((h[0] * Mx + h[1] * My) + h[2]) * ww;
        const double yi = ((h[3] * Mx + h[4] * My) + h[5]) * ww;
        const double ex = xi - r[2], ey = yi - r[3];
        if (p & 1) {
            grp = (grp + ex * ex) + ey * ey;
            sum = sum + grp;
        } else if (p + 1 < m) {
            grp = ex * ex + ey * ey;
        } else {
            sum = sum + ex * ex;
            sum = sum + ey * ey;
        }
        if (mx < fabs(ex)) mx = fabs(ex);
        if (mx < fabs(ey)) mx = fabs(ey);
        if (J) {
            const double a = Mx * ww, b = My * ww;
            const double gx6 = (-a) * xi, gx7 = (-b) * xi, gy6 = (-a) * yi, gy7 = (-b) * yi;
            const double jx = hg_lm_jx(i, a, b, ww, gx6, gx7), jy = hg_lm_jy(i, a, b, ww, gy6, gy7);
            const double ox = isA ? hg_lm_jx(j, a, b, ww, gx6, gx7) : ex, oy = isA ? hg_lm_jy(j, a, b, ww, gy6, gy7) : ey;
            acc = acc + jx * ox;
            acc = acc + jy * oy;
        }
    }
    S = sum; rinf = mx;
    if (J) {
        __syncthreads();
        if (isA) { HG_LA(i, j) = acc; HG_LA(j, i) = acc; }
        if (isV) HG_LX(HG_LM_V, i) = acc;
        __syncthreads();
    }
}

// lane 0: Jacobi at n = 8 on HG_JA and SVBkSb's threshold (sum of W) * 2 DBL_EPSILON
__device__ __forceinline__ double hg_lm_eig(const HgLds& s) {
    hg_jacobi<8>(s, 0);
    double t = 0.0;
    for (int e = 0; e < 8; ++e) t = t + HG_JW(e);
    return t * (2.0 * DBL_EPSILON);
}

__device__ __forceinline__ double hg_lm_dot8(const double* a, const double* b) {      // a.dot(b): two groups of four
    double r = 0.0;
    r = r + (((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]);
    r = r + (((a[4] * b[4] + a[5] * b[5]) + a[6] * b[6]) + a[7] * b[7]);
    return r;
}

// LMSolverImpl1::run (R:476-580) on H[0..8) over the m rows of `work`, by the whole wave: the sums over the rows are hg_lm_eval's, the
// 8 x 8 eigen-solves run on lane 0, and every lane computes the scalars (S, Sd, R, lambda, nu) from the same LDS values, so the control
// flow is uniform without a broadcast.
__device__ void hg_lm(const HgLds& s, int lane, const float* work, int m, double* H, int max_iters, int& ret, int& nfj) {
    const double Rlo = 0.25, Rhi = 0.75, epsx = FLT_EPSILON, epsf = FLT_EPSILON;
    __syncthreads();                                                  // the refit's readers of V are done
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) HG_LX(HG_LM_X, i) = H[i];
    }
    __syncthreads();
    double S, rinf;
    hg_lm_eval<true>(s, lane, work, m, HG_LM_X, S, rinf);
    int nfJ = 2;
    if (lane < 8) HG_LX(HG_LM_D, lane) = HG_LA(lane, lane);           // D = A.diag().clone(): taken once
    __syncthreads();
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        if (lane == 0) {                                              // solve(Ap, v, d, DECOMP_EIG), xd = x - d
            for (int i = 0; i < 8; ++i)
                for (int j = 0; j < 8; ++j) HG_JA(i, j) = HG_LA(i, j);
            for (int i = 0; i < 8; ++i) HG_JA(i, i) = HG_JA(i, i) + lambda * HG_LX(HG_LM_D, i);
            const double t = hg_lm_eig(s);
            for (int j = 0; j < 8; ++j) HG_LX(HG_LM_DD, j) = 0.0;
            for (int e = 0; e < 8; ++e) {
                const double w = HG_JW(e);
                if (!(fabs(w) > t)) continue;
                double sv = 0.0;
                for (int j = 0; j < 8; ++j) sv = sv + HG_JV(e, j) * HG_LX(HG_LM_V, j);
                sv = sv * (1.0 / w);
                for (int j = 0; j < 8; ++j) HG_LX(HG_LM_DD, j) = HG_LX(HG_LM_DD, j) + sv * HG_JV(e, j);
            }
            for (int j = 0; j < 8; ++j) HG_LX(HG_LM_XD, j) = HG_LX(HG_LM_X, j) - HG_LX(HG_LM_DD, j);
        }
        __syncthreads();
        double Sd, unused;
        hg_lm_eval<false>(s, lane, work, m, HG_LM_XD, Sd, unused);
        ++nfJ;
        double d[8], v[8], td[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { d[i] = HG_LX(HG_LM_DD, i); v[i] = HG_LX(HG_LM_V, i); }
#pragma unroll
        for (int i = 0; i < 8; ++i) {                                 // gemm(A, d, -1, v, 2, temp_d)
            double sv = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) sv = sv + HG_LA(i, k) * d[k];
            td[i] = (-sv) + 2.0 * v[i];
        }
        const double dS = hg_lm_dot8(d, td);
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            const double t = hg_lm_dot8(d, v);
            double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = nu < 2. ? 2. : nu;
            nu = 10. < nu ? 10. : nu;
            if (lambda == 0) {                                        // invert(A, Ap, DECOMP_EIG): its diagonal alone is read
                __syncthreads();
                if (lane == 0) {
                    for (int i = 0; i < 8; ++i)
                        for (int j = 0; j < 8; ++j) HG_JA(i, j) = HG_LA(i, j);
                    const double th = hg_lm_eig(s);
                    double maxval = DBL_EPSILON;
                    for (int i = 0; i < 8; ++i) {
                        double sv = 0.0;
                        for (int e = 0; e < 8; ++e) {
                            const double w = HG_JW(e);
                            if (fabs(w) > th) sv = sv + HG_JV(e, i) * (HG_JV(e, i) * (1.0 / w));
                        }
                        if (maxval < fabs(sv)) maxval = fabs(sv);
                    }
                    HG_LX(HG_LM_MAXVAL, 0) = maxval;
                }
                __syncthreads();
                lambda = lc = 1. / HG_LX(HG_LM_MAXVAL, 0);
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            ++nfJ;
            S = Sd;
            __syncthreads();
            if (lane < 8) HG_LX(HG_LM_X, lane) = HG_LX(HG_LM_XD, lane);      // swap(x, xd): xd is written anew before it is read
            __syncthreads();
            hg_lm_eval<true>(s, lane, work, m, HG_LM_X, unused, rinf);
        }
        ++iter;
        double dinf = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (dinf < fabs(d[i])) dinf = fabs(d[i]);
        if (!(iter < max_iters && dinf >= epsx && rinf >= epsf)) break;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) H[i] = HG_LX(HG_LM_X, i);
    __syncthreads();                                                  // before the next user of the Jacobi's LDS
    ret = iter == max_iters ? -iter : iter;
    nfj = nfJ;
}
#undef HG_LA
#undef HG_LX
#undef HG_JA
#undef HG_JV
#undef HG_JW

// findHomography2 (R:602-693, RANSAC; R:672 with LM only) by the whole wave; every field of the result is uniform.  mask (may be null) gets
// rows [0, n); work gets the inliers in order, 4 floats a row.
template <bool LM>
__device__ void hg_find(const HgLds& s, int lane, const float* pts, long long step, int n, unsigned char* mask, long long mask_step, float* work,
                        const HgCall& c, HgRun& out) {
    out.ok = false; out.inliers = 0; out.iters = 0; out.win = -1; out.attempts = 0;
    out.lm_ret = 0; out.lm_nfj = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) out.H[i] = 0.0;
    const float t = (float)(c.thresh * c.thresh);
    const bool direct = n == 4;                                       // R:641-645: runKernel over the four rows, the mask all ones
    if (n > 4) {                                               // R:139-233
        unsigned long long rng = ~0ull;                               // RNG rng((uint64)-1): lane 0's copy is the generator
        int niters = max(c.max_iters, 1), max_good = 0, it = 0;
        bool stop = false;
        while (!stop && it < niters) {
            const int cn = min(HG_CHUNK, niters - it);
            __syncthreads();                                          // the previous chunk's readers of sub / found / att are done
            s.found[lane] = 0;                                        // hypotheses past a failed getSubset are never drawn
            s.att[lane] = 0;
            __syncthreads();
            if (lane == 0) {
                bool found = true;
                for (int h = 0; h < cn && found; ++h) {
                    int attempts = 0;
                    int i0 = 0, i1 = 0, i2 = 0, i3 = 0;
                    found = false;
                    while (attempts < HG_MAX_ATTEMPTS) {              // R:111-134: a duplicate draws again, a bad subset costs an attempt
                        i0 = hg_uniform(rng, n);
                        do i1 = hg_uniform(rng, n); while (i1 == i0);
                        do i2 = hg_uniform(rng, n); while (i2 == i0 || i2 == i1);
                        do i3 = hg_uniform(rng, n); while (i3 == i0 || i3 == i1 || i3 == i2);
                        float q[4][4];
                        hg_load4(pts, step, i0, i1, i2, i3, q);
                        ++attempts;
                        if (hg_check_subset(q)) { found = true; break; }
                    }
                    s.sub[0 * WAVE + h] = i0; s.sub[1 * WAVE + h] = i1; s.sub[2 * WAVE + h] = i2; s.sub[3 * WAVE + h] = i3;
                    s.found[h] = found ? 1 : 0;
                    s.att[h] = attempts;
                }
            }
            __syncthreads();
            bool hok = false;
            double H[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) H[i] = 0.0;
            if (lane < cn && s.found[lane]) {
                float q[4][4];
                hg_load4(pts, step, s.sub[0 * WAVE + lane], s.sub[1 * WAVE + lane], s.sub[2 * WAVE + lane], s.sub[3 * WAVE + lane], q);
                hok = hg_run_kernel_lane(s, lane, q, H);
            }
            for (int h = 0; h < cn && it < niters; ++h) {
                out.attempts += s.att[h];
                if (!s.found[h]) { stop = true; break; }              // R:190-195: at iteration 0 nothing was found, later the loop ends
                if (__shfl((int)hok, h)) {
                    double Hh[9];
                    float Hf[8];
#pragma unroll
                    for (int i = 0; i < 9; ++i) Hh[i] = __shfl(H[i], h);
#pragma unroll
                    for (int i = 0; i < 8; ++i) Hf[i] = (float)Hh[i];
                    int good = 0;
                    for (int i0 = 0; i0 < n; i0 += WAVE) {
                        const int i = i0 + lane;
                        const bool in = i < n && hg_inlier(Hf, row_ptr(pts, i, step), t);
                        good += __popcll(__ballot(in));
                    }
                    if (good > max(max_good, 3)) {                    // R:207
                        max_good = good; out.win = it;
#pragma unroll
                        for (int i = 0; i < 9; ++i) out.H[i] = Hh[i];
                        niters = hg_update_iters(c.confidence, (double)(n - good) / n, niters);
                    }
                }
                ++it;
            }
        }
        out.iters = it;
        out.ok = max_good > 0;
    }
    // the mask of the model found (R:209, R:226), or zeros (R:687), and the inliers in order (R:659-660); n == 4: every row (R:643)
    float Hf[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) Hf[i] = (float)out.H[i];
    int m = 0;
    for (int i0 = 0; i0 < n; i0 += WAVE) {
        const int i = i0 + lane;
        bool in = false;
        if (i < n) in = direct || (out.ok && hg_inlier(Hf, row_ptr(pts, i, step), t));
        const unsigned long long bal = __ballot(in);
        if (i < n && mask && !direct) mask[(long long)i * mask_step] = in ? 1 : 0;
        if (in) {
            const float* r = row_ptr(pts, i, step);
            float* o = work + 4ll * (m + __popcll(bal & ((1ull << lane) - 1ull)));
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
        }
        m += __popcll(bal);
    }
    out.inliers = m;
    __syncthreads();                                                  // the rows of `work` are written before the wave reads them
    if (direct || (out.ok && m > 0)) {                                // R:657-668: runKernel over all inliers; 0 leaves the RANSAC model
        double H[9];
        const bool ok = hg_run_kernel_wave(s, lane, work, 16, m, H);
        if (ok) {
#pragma unroll
            for (int i = 0; i < 9; ++i) out.H[i] = H[i];
        }
        if (direct) {
            out.ok = ok;
            if (!ok) out.inliers = 0;
            if (mask && lane < 4) mask[(long long)lane * mask_step] = ok ? 1 : 0;
        }
        if constexpr (LM) {                                           // R:669-672: over the inliers, from the refit or the RANSAC model it left
            if (!direct) hg_lm(s, lane, work, m, out.H, c.lm_max_iters, out.lm_ret, out.lm_nfj);
        }
    }
}

// LM = false is isx_find_homography's kernel; LM = true adds the polish and stats columns 8 - 11 (isx_find_homography_lm).  A template, so
// that the unrefined call carries none of the polish in registers or code.
template <bool LM>
__global__ __launch_bounds__(HG_CHUNK) void k_hg_pairs(HgCall c) {
    constexpr int NST = LM ? 12 : 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_smem[];
    HgLds s;
    s.A = (double*)(hg_smem + HG_LDS_A); s.V = (double*)(hg_smem + HG_LDS_V); s.W = (double*)(hg_smem + HG_LDS_W);
    s.indR = (int*)(hg_smem + HG_LDS_INDR); s.indC = (int*)(hg_smem + HG_LDS_INDC); s.sub = (int*)(hg_smem + HG_LDS_SUB);
    s.found = (int*)(hg_smem + HG_LDS_FOUND); s.att = (int*)(hg_smem + HG_LDS_ATT);
    const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
    const HgPair& P = as_global(c.pairs)[p];
    int n = as_global(c.counts)[p];
    int status = 0;
    if (n > P.cap) { n = P.cap; status |= HG_ST_CLAMPED; }
    if (n < 0) n = 0;
    double Hout[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hout[i] = 0.0;
    int st[NST] = {};
    double conf = 0.0;
    if (n >= c.thresh1) {                                             // R:836
        float* const work_a = as_global(P.work_a);
        st[3] = st[5] = -1;
        int num_inliers = 0;
        for (int pass = 0; pass < 2; ++pass) {
            HgRun r;
            if (pass == 0) hg_find<LM>(s, lane, as_global(P.points), P.points_step, n, as_global(P.mask), P.mask_step, work_a, c, r);      // R:862
            else hg_find<LM>(s, lane, work_a, 16, num_inliers, nullptr, 0, as_global(P.work_b), c, r);                                    // R:909
            st[2 + 2 * pass] = r.iters; st[3 + 2 * pass] = r.win; st[6] += r.attempts;
            if constexpr (LM) { st[8 + 2 * pass] = r.lm_ret; st[9 + 2 * pass] = r.lm_nfj; }
#pragma unroll
            for (int i = 0; i < 9; ++i) Hout[i] = r.ok ? r.H[i] : 0.0;
            if (pass == 1) {
                status |= HG_ST_PASS2;
                if (!r.ok) status = (status | HG_ST_PASS2_FAILED) & ~HG_ST_H;
                break;
            }
            if (!r.ok) break;
            status |= HG_ST_H;
            if (fabs(hg_det3(r.H)) < DBL_EPSILON) { status |= HG_ST_DEGENERATE; break; }      // R:863
            num_inliers = r.inliers;                                                          // R:867-870
            st[1] = num_inliers;
            conf = num_inliers / (8 + 0.3 * n);                                               // R:874
            conf = conf > 3. ? 0. : conf;                                                     // R:878
            if (num_inliers < c.thresh2) break;                                               // R:881
        }
    }
    st[0] = status;
    if (lane < 9) {
        double v = Hout[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) v = lane == i ? Hout[i] : v;
        row_ptr(as_global(c.H), 3ll * p + lane / 3, c.H_step)[lane % 3] = v;
    }
    if (lane < NST) {
        int v = st[0];
#pragma unroll
        for (int i = 1; i < NST; ++i) v = lane == i ? st[i] : v;
        row_ptr(as_global(c.stats), p, c.stats_step)[lane] = v;
    }
    if (lane == 0) as_global(c.conf)[p] = conf;
}

struct HgScratch : UploadScratch {       // pin: the table, host counts and the staged rows of host points mats (scratch.hpp)
    bool lds_set = false;                // both k_hg_pairs may use HG_LDS_BYTES of LDS on `device`
};

// The body of both entries.  lm: isx_find_homography_lm - k_hg_pairs<true>, 12 stats columns.
int hg_call(bool lm, int lm_max_iters, const char* who, int num_pairs, const isx_mat* points, const isx_mat* counts, double reproj_thresh, int max_iters,
            double confidence, int num_matches_thresh1, int num_matches_thresh2, isx_mat* H, isx_mat* inlier_masks, isx_mat* stats, isx_mat* conf,
            int* info, int device, void* hip_stream) {
    const int nst = lm ? 12 : 8;                                  // stats columns
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(num_pairs >= 0, ISX_ERR_INVALID, "%s: %d pairs", who, num_pairs);
    ISX_CHECK_ARG(num_pairs == 0 || (points && counts && H && inlier_masks && stats && conf), ISX_ERR_INVALID,
                  "%s: null points, counts, H, inlier_masks, stats or conf", who);
    ISX_CHECK_ARG(confidence > 0 && confidence < 1, ISX_ERR_INVALID, "%s: confidence %g is not in (0, 1)", who, confidence);        // R:156
    ISX_CHECK_ARG(max_iters >= 1, ISX_ERR_INVALID, "%s: max_iters %d", who, max_iters);
    ISX_CHECK_ARG(num_matches_thresh1 >= 0 && num_matches_thresh2 >= 0, ISX_ERR_INVALID, "%s: thresholds %d, %d", who, num_matches_thresh1, num_matches_thresh2);
    ISX_CHECK_ARG(reproj_thresh == reproj_thresh, ISX_ERR_INVALID, "%s: reproj_thresh is not a number", who);
    ISX_CHECK_ARG(!lm || (lm_max_iters >= 1 && lm_max_iters <= 1000), ISX_ERR_INVALID, "%s: lm_max_iters %d is not in [1, 1000]", who, lm_max_iters);
    if (reproj_thresh <= 0) reproj_thresh = 3;                                                                                   // R:636
    if (num_pairs > 0) {
        ISX_TRY(check_mat_holds(*counts, ISX_32SC1, 1, num_pairs, 4, STOP_NO_ROW_PRESENT, device, who, "counts", 0));
        ISX_TRY(check_mat_holds(*H, ISX_64FC1, 3ll * num_pairs, 3, 8, STOP_NO_ROW_PRESENT, device, who, "H", 0));
        ISX_TRY(check_mat_holds(*stats, ISX_32SC1, num_pairs, nst, 4, STOP_NO_ROW_PRESENT, device, who, "stats", 0));
        ISX_TRY(check_mat_holds(*conf, ISX_64FC1, 1, num_pairs, 8, STOP_NO_ROW_PRESENT, device, who, "conf", 0));
    }
    for (int p = 0; p < num_pairs; ++p) {
        ISX_CHECK_ARG(points[p].rows >= 0 && inlier_masks[p].rows >= 0, ISX_ERR_INVALID, "%s: pair %d: negative rows", who, p);
        ISX_TRY(check_mat_holds(points[p], ISX_32FC1, 0, 4, 4, STOP_NO_ROW_PRESENT, device, who, "points", p));
        ISX_TRY(check_mat_holds(inlier_masks[p], ISX_8UC1, 0, 1, 1, STOP_NO_ROW_PRESENT, device, who, "inlier_masks", p));
    }
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_TRY(refuse_capture(st, who, "the call uploads its tables and may stage host mats"));
    if (num_pairs == 0) {
        if (info) { info[0] = 0; info[1] = 0; }
        return ISX_OK;
    }

    // ---- one buffer: [upload: table | host counts | staged rows of host points] [work_a, work_b per pair] [staged host outputs] ----
    std::vector<HgPair> prs((size_t)num_pairs);
    std::vector<int> cap((size_t)num_pairs), up_rows((size_t)num_pairs, 0);
    const int* h_counts = counts->device < 0 ? (const int*)counts->data : nullptr;
    StagedMat m_counts, m_H, m_stats, m_conf;
    std::vector<StagedMat> m_pts((size_t)num_pairs), m_mask((size_t)num_pairs);
    Bump lay;
    const size_t o_prs = lay.take(prs.size() * sizeof(HgPair));
    m_counts.plan(lay, *counts, 1, (size_t)num_pairs * 4);
    std::vector<size_t> o_wa((size_t)num_pairs, 0), o_wb((size_t)num_pairs, 0);
    for (int p = 0; p < num_pairs; ++p) {
        cap[p] = std::min(points[p].rows, inlier_masks[p].rows);
        // the rows the kernel may read; of a host mat, those a host count names
        up_rows[p] = points[p].device < 0 && h_counts ? std::min(std::max(h_counts[p], 0), cap[p]) : cap[p];
        m_pts[p].plan(lay, points[p], up_rows[p], 16);
    }
    const size_t upload_bytes = lay.at;
    for (int p = 0; p < num_pairs; ++p) {
        o_wa[p] = lay.take((size_t)cap[p] * 16);
        o_wb[p] = lay.take((size_t)cap[p] * 16);
    }
    m_H.plan(lay, *H, 3ll * num_pairs, 24);
    m_stats.plan(lay, *stats, num_pairs, (size_t)4 * nst);
    m_conf.plan(lay, *conf, 1, (size_t)num_pairs * 8);
    bool any_host_mask = false;
    for (int p = 0; p < num_pairs; ++p) {
        m_mask[p].plan(lay, inlier_masks[p], cap[p], 1);
        any_host_mask |= m_mask[p].staged;
    }

    HgScratch& s = per_thread<HgScratch>();
    if (s.device != device || !s.lds_set) {                       // before begin(), so before this stream is made to wait for another
        ISX_HIP(hipFuncSetAttribute((const void*)k_hg_pairs<false>, hipFuncAttributeMaxDynamicSharedMemorySize, HG_LDS_BYTES));
        ISX_HIP(hipFuncSetAttribute((const void*)k_hg_pairs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, HG_LDS_BYTES));
        s.lds_set = true;
    }
    ISX_TRY(s.begin(device, st, lay.at, upload_bytes));
    char* const dev = (char*)s.work.p;
    char* const pin = (char*)s.pin.p;

    // ---- fill the upload ----
    for (int p = 0; p < num_pairs; ++p) {
        HgPair& P = prs[p];
        std::memset(&P, 0, sizeof(P));
        P.cap = up_rows[p];                                       // of a staged mat, the staged rows are what the kernel may read
        if (cap[p] == 0) continue;
        m_pts[p].fill(pin);
        m_pts[p].bind(dev, P.points, P.points_step);
        m_mask[p].bind(dev, P.mask, P.mask_step);
        P.work_a = (float*)(dev + o_wa[p]); P.work_b = (float*)(dev + o_wb[p]);
    }
    std::memcpy(pin + o_prs, prs.data(), prs.size() * sizeof(HgPair));
    m_counts.fill(pin);
    ISX_TRY(s.upload(st, upload_bytes));

    // ---- one launch ----
    HgCall c;
    c.pairs = (const HgPair*)(dev + o_prs);
    m_counts.bind(dev, c.counts);
    m_H.bind(dev, c.H, c.H_step);
    m_stats.bind(dev, c.stats, c.stats_step);
    m_conf.bind(dev, c.conf);
    c.thresh = reproj_thresh; c.confidence = confidence;
    c.max_iters = max_iters; c.thresh1 = num_matches_thresh1; c.thresh2 = num_matches_thresh2;
    c.lm_max_iters = lm_max_iters;
    if (lm) ISX_LAUNCH("homography_lm_pairs", (double)num_pairs * 4096.0, st, k_hg_pairs<true>, dim3((unsigned)num_pairs), dim3(HG_CHUNK), HG_LDS_BYTES, c);
    else ISX_LAUNCH("homography_pairs", (double)num_pairs * 4096.0, st, k_hg_pairs<false>, dim3((unsigned)num_pairs), dim3(HG_CHUNK), HG_LDS_BYTES, c);
    ISX_TRY(s.ran(st));

    // ---- host outputs ----
    if (m_H.staged || m_stats.staged || m_conf.staged || any_host_mask) {
        std::vector<int> cnt_tmp;
        const int* cnt = h_counts;
        if (any_host_mask && !h_counts) {
            cnt_tmp.resize((size_t)num_pairs);
            ISX_TRY(counts_to_host(cnt_tmp.data(), (const int*)counts->data, num_pairs, st));
            cnt = cnt_tmp.data();
        }
        ISX_TRY(m_H.back(dev, 3ll * num_pairs, st));
        ISX_TRY(m_stats.back(dev, num_pairs, st));
        ISX_TRY(m_conf.back(dev, 1, st));
        for (int p = 0; p < num_pairs; ++p) {
            if (!m_mask[p].staged) continue;
            const int n = std::min(std::max(cnt[p], 0), cap[p]);
            if (n < num_matches_thresh1 || n == 0) continue;      // R:836: the mask is not written
            ISX_TRY(m_mask[p].back(dev, n, st));
        }
        ISX_HIP(hipStreamSynchronize(st));
    }
    if (info) { info[0] = num_pairs; info[1] = 1; }
    return ISX_OK;
}

}  // namespace

extern "C" {

int isx_homography_release(void) ISX_ENTRY {
    clear_error();
    return per_thread<HgScratch>().release();
} ISX_EXIT("isx_homography_release")

int isx_find_homography(int num_pairs, const isx_mat* points, const isx_mat* counts, double reproj_thresh, int max_iters, double confidence,
                        int num_matches_thresh1, int num_matches_thresh2, isx_mat* H, isx_mat* inlier_masks, isx_mat* stats, isx_mat* conf,
                        int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return hg_call(false, 0, "find_homography", num_pairs, points, counts, reproj_thresh, max_iters, confidence, num_matches_thresh1,
                   num_matches_thresh2, H, inlier_masks, stats, conf, info, device, hip_stream);
} ISX_EXIT("isx_find_homography")

int isx_find_homography_lm(int num_pairs, const isx_mat* points, const isx_mat* counts, double reproj_thresh, int max_iters, double confidence,
                           int num_matches_thresh1, int num_matches_thresh2, int lm_max_iters, isx_mat* H, isx_mat* inlier_masks, isx_mat* stats,
                           isx_mat* conf, int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return hg_call(true, lm_max_iters, "find_homography_lm", num_pairs, points, counts, reproj_thresh, max_iters, confidence, num_matches_thresh1,
                   num_matches_thresh2, H, inlier_masks, stats, conf, info, device, hip_stream);
} ISX_EXIT("isx_find_homography_lm")

}  // extern "C"
