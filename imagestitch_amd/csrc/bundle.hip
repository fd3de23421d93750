// bundle.hip — detail::BundleAdjusterRay as every main of the reference calls it (W = its cylindrical-projection demo: W:183-188 converts the
// estimator's R to CV_32F, W:189-194 runs adjuster->setConfThresh(1); (*adjuster)(features, pairwise_matches, cameras)) on gfx950:
//   isx_bundle_adjust_ray      focal and rotation of every camera refined over the inlier matches of every edge, for every rig of a matcher
//                              call, reading keypoints, matches, masks, counts, conf, the estimator's rig_stats and cameras where the three
//                              earlier stages left them
//   isx_bundle_adjust_reproj   detail::BundleAdjusterReproj (commented out at W:190; cv::Stitcher's default) on the same inputs: focal, ppx,
//                              ppy, aspect and rotation over the reprojection error - k_ba_rigs compiled a second time (ReprojTr)
//   isx_wave_correct           detail::waveCorrect (commented out at W:198) for every rig: k_wave_rigs, float32 as OpenCV's is
//   isx_bundle_release         returns the per-thread scratch
//   isx_selftest_bundle_math   the host compilation of bundle_math.hpp (needs no device), and isx_selftest_bundle_math_device, the same items
//                              by the device compilation: a thread each
//
// The specification is tests/helpers/bundle_np.py (DESIGN.md §8 "Bundle adjuster"): OpenCV 3.4.2's BundleAdjusterBase::estimate,
// BundleAdjusterRay, CvLevMarq and cvRodrigues2 restated (unpinned), with three decisions of this project - a Cholesky solve with SVBkSb's
// truncation rule on the pivots, sin / cos / acos restated in + - * / sqrt (bundle_math.hpp), summation orders fixed by ISX_BUNDLE_TILE.
//
// (tests/helpers/bundle_reproj_np.py specifies the other two entries.)
//
// ONE launch per call: k_ba_rigs<Tr>, one block of Tr::THREADS (Ray 256, Reproj 512) per rig, the whole Levenberg-Marquardt loop inside.  The stage is latency-bound:
// it is on the GPU so that cameras follow the estimator in stream order without a read-back, and so that many rigs cost one.  Per rig:
//   setup   a thread per pair counts the inliers of its edge (conf > conf_thresh), one thread lays the edges out densely, a thread per pair
//           gathers the keypoints of its inliers; a thread per camera takes the polar factor of R and its Rodrigues vector;
//   J       Ray: a thread per (camera, parameter, sign): the perturbed R K^-1, kept in LDS; a thread per inlier match: the 1 + 16 rays and
//           its 3 x 8 Jacobian entries (27 doubles a match in scratch - J is never stored whole).  Reproj: two matrices x 15 variants x 64
//           cameras do not fit LDS, so a thread per (edge, variant) forms the edge's 1 + 28 matrices H in per-rig scratch (L2-resident) and
//           a thread per match does the 29 projections (30 doubles a match).  Both: a thread per (tile, entry): the 45 / 120 partial sums
//           of a tile of ISX_BUNDLE_TILE matches; a thread per entry of JtJ (scratch, L2-resident) and JtErr: the tiles in edge order;
//   solve   Cholesky, left-looking: a thread per row against the pivot row in LDS, three barriers a column; the substitutions keep a running
//           sum per row in a register, one barrier an unknown;
//   err     a thread per match, a thread per tile; the norm adds the tiles' sums in order, fetched a block at a time.
// Every loop-control decision (retry, done, the NaN exit) is made by thread 0 and broadcast through LDS; no barrier sits under a condition
// that threads can see differently.
#include "isx_device.hpp"
#include "bundle_math.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"

#include <algorithm>
#include <cfloat>

using namespace isx;
using namespace isxd;
using namespace isxbm;

namespace {

constexpr int BA_MAXN = ISX_BUNDLE_MAX_IMAGES;
constexpr int BA_TILE = ISX_BUNDLE_TILE;
static_assert(BA_MAXN == ISX_ESTIMATOR_MAX_IMAGES, "the chain never refuses what the estimator accepted");

// What k_ba_rigs takes from its traits Tr (RayTr, ReprojTr below): PC parameters a camera, RES residuals a match, STEP of the central
// differences, THREADS a block, RV where the Rodrigues vector starts among a camera's parameters, HS / FV doubles of LDS for the camera
// matrices, and the two phases cam_mats (the matrices calcError multiplies a keypoint by, plain and with one parameter moved either way) and
// matches (calcError and calcJacobian of every inlier match into jrow).  The rest follows:
template <class Tr>
struct BaK {
    static constexpr int W = 2 * Tr::PC;                     // columns of a match's Jacobian rows: the parameters of its two cameras
    static constexpr int U = W * (W + 1) / 2;                // upper entries of the W x W block
    static constexpr int ENT = U + W + 1;                    // a tile's sums: the U entries, W of J^T err, err^2 (Ray 45, Reproj 120)
    static constexpr int JROW = Tr::RES * (1 + W);           // a match in scratch: err[RES], J[RES][W] (Ray 27, Reproj 30)
    static constexpr int MAXP = Tr::PC * BA_MAXN;            // parameters a rig: a thread per row of the Cholesky
    static constexpr int PROW = Tr::THREADS;                 // prow holds one value a thread in ba_err_norm, one a parameter in ba_step
    static_assert(MAXP <= Tr::THREADS, "one parameter per thread");
};

// lambda = 10^lambdaLg10: the 33 correctly rounded literals
__constant__ double BA_LAMBDA[33] = {1e-16, 1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0,
                                     1e1,   1e2,   1e3,   1e4,   1e5,   1e6,   1e7,   1e8,  1e9,  1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16};

struct BaRig { int img_first, n, pair_first, pair_count; long long match_first, tile_first, mat_first; };
struct BaPair {                                              // the rig's pairs sorted by (from, to): the order of the edges
    const int* matches; long long matches_step;              // the caller's device mat or the staged copy of a host mat
    const unsigned char* mask; long long mask_step;
    int from, to, row, cap;                                  // local image indices; row: the pair's index in counts / conf; cap: min rows
};
struct BaImg { const float* kp; long long kp_step; int rows, pad; };

struct BaCall {
    const BaRig* rigs; const BaPair* pairs; const BaImg* imgs; const int* sizes;
    const int* counts; const double* conf;
    const int* est; long long est_step;
    const double* cin; long long cin_step;
    double* cout; long long cout_step;
    float* kr; long long kr_step;
    int* rs; long long rs_step;
    double* re; long long re_step;
    float4* pts; int* match_pair;                            // per inlier match, dense per rig: the two keypoints, the pair it belongs to
    double* jrow;                                            // JROW doubles per inlier match
    double* tiles; int* tile_pair;                           // ENT doubles per tile; the pair of a tile
    int* pair_tab;                                           // per pair: inliers, first match, first tile
    double* jtj; double* lt;                                 // per rig (PC n) x (PC n): JtJ (row-major, symmetric), L (column-major)
    double* hmat;                                            // Reproj: RP_VAR x 9 doubles per pair, the edge's H plain and moved
    double conf_thresh, eps;
    int max_iter, refine_flags;
};

enum { C_EDGES, C_M, C_T, C_STATUS, C_CENTER, C_AGAIN, C_DONE, C_LG, C_ITERS, C_JEV, C_EEV, C_KEEP, C_NAN, C_N };
enum { D_ENORM, D_PREVNORM, D_FIRST, D_THRESH, D_PIV, D_N };

struct BaCtx {                                               // what the phases share: LDS, the rig's slices of the call's scratch
    double* Hs; double* fv; double* param; double* prev; double* bvec; double* bc; double* prow; double* dctl;
    short* slot; int* ctl; unsigned char* kept;
    const BaPair* prs; const int* sizes; int* ptab; const float4* pts; const int* match_pair; double* jrow; double* tiles; const int* tile_pair;
    double* jtj; double* lt; double* hmat;
    int n, N, tid, pc, flags;
};

// ---- BundleAdjusterRay: focal and rvec a camera, the difference of two rays a match -----------------------------------------------------------
struct RayTr {
    static constexpr int PC = 4, RES = 3, THREADS = 256, RV = 1;
    static constexpr double STEP = 1e-3;
    static constexpr int HS = BA_MAXN * 81;                  // [camera][variant][9]: R K^-1, plain and with one parameter moved either way
    static constexpr int FV = BA_MAXN * 3;                   // [camera]: f, f - step, f + step
    static constexpr int HMAT = 0;                           // no per-pair matrices in scratch
    static const char* who() { return "bundle_adjust_ray"; }
    static const char* kernel() { return "bundle_rigs"; }

    __device__ static void init_param(const double* ci, double* p) { p[0] = ci[0]; }
    __device__ static void intrinsics(const double* p, const double* ci, double& focal, double& aspect, double& ppx, double& ppy) {
        focal = p[0]; aspect = ci[1]; ppx = ci[2]; ppy = ci[3];
    }

    // R K^-1 of every camera at `p`: variant 0, and with jac the 8 perturbed ones (1 + 2 q + sign; sign 0: val - step, 1: val + step)
    __device__ static void cam_mats(const BaCtx& x, const double* p, bool jac) {
        const int per = jac ? 9 : 1;
        for (int w = x.tid; w < x.n * per; w += THREADS) {
            const int cam = w / per, v = w % per;
            double p4[4] = {p[4 * cam], p[4 * cam + 1], p[4 * cam + 2], p[4 * cam + 3]};
            if (v > 0) {
                const int q = (v - 1) >> 1;
                const double val = p4[q];
                const double moved = ((v - 1) & 1) ? val + STEP : val - STEP;
#pragma unroll
                for (int e = 0; e < 4; ++e) p4[e] = e == q ? moved : p4[e];
            }
            double H[9];
            bm_cam_h(p4, x.sizes[2 * cam], x.sizes[2 * cam + 1], H);
#pragma unroll
            for (int e = 0; e < 9; ++e) x.Hs[(cam * 9 + v) * 9 + e] = H[e];
            if (v <= 2) x.fv[cam * 3 + v] = p4[0];           // f, f - step, f + step
        }
    }

    // calcError (and with jac calcJacobian) of every inlier match into jrow
    __device__ static void matches(const BaCtx& x, bool jac) {
        constexpr int BA_JROW = 27;
        const int M = x.ctl[C_M];
        const double h2 = 2.0 * STEP;
        for (int idx = x.tid; idx < M; idx += THREADS) {
            const BaPair& P = x.prs[x.match_pair[idx]];
            const int i = P.from, j = P.to;
            const float4 pt = x.pts[idx];
            const double x1 = (double)pt.x, y1 = (double)pt.y, x2 = (double)pt.z, y2 = (double)pt.w;
            const double fi = x.fv[3 * i], fj = x.fv[3 * j];
            double a[3], b[3], err[3];
            bm_ray(x.Hs + (i * 9) * 9, x1, y1, a);
            bm_ray(x.Hs + (j * 9) * 9, x2, y2, b);
            const double mult = sqrt(fi * fj);
            double* const out = x.jrow + (long long)idx * BA_JROW;
#pragma unroll
            for (int k = 0; k < 3; ++k) { err[k] = mult * (a[k] - b[k]); out[k] = err[k]; }
            if (!jac) continue;
            for (int q = 0; q < 4; ++q) {
                double e0[3], e1[3], r[3];
                for (int sg = 0; sg < 2; ++sg) {             // camera i moves
                    bm_ray(x.Hs + (i * 9 + 1 + 2 * q + sg) * 9, x1, y1, r);
                    const double mm = sqrt((q == 0 ? x.fv[3 * i + 1 + sg] : fi) * fj);
#pragma unroll
                    for (int k = 0; k < 3; ++k) (sg ? e1 : e0)[k] = mm * (r[k] - b[k]);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) out[3 + 8 * k + q] = (e1[k] - e0[k]) / h2;
                for (int sg = 0; sg < 2; ++sg) {             // camera j moves
                    bm_ray(x.Hs + (j * 9 + 1 + 2 * q + sg) * 9, x2, y2, r);
                    const double mm = sqrt(fi * (q == 0 ? x.fv[3 * j + 1 + sg] : fj));
#pragma unroll
                    for (int k = 0; k < 3; ++k) (sg ? e1 : e0)[k] = mm * (a[k] - r[k]);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) out[3 + 8 * k + 4 + q] = (e1[k] - e0[k]) / h2;
            }
        }
    }
};

// ---- BundleAdjusterReproj: focal, ppx, ppy, aspect and rvec a camera, the reprojection error of p1 in image 2 a match ------------------------
constexpr int RP_VAR = 29;                                   // an edge's H: plain, then 1 + 2 q + sign for the 14 parameters of its two cameras
struct ReprojTr {
    static constexpr int PC = 7, RES = 2, THREADS = 512, RV = 4;
    static constexpr double STEP = 1e-4;
    static constexpr int HS = BA_MAXN * 9;                   // LDS holds only the rotations of the last phase: the H live in scratch
    static constexpr int FV = 1;
    static constexpr int HMAT = RP_VAR * 9;
    static const char* who() { return "bundle_adjust_reproj"; }
    static const char* kernel() { return "bundle_reproj_rigs"; }

    __device__ static void init_param(const double* ci, double* p) { p[0] = ci[0]; p[1] = ci[2]; p[2] = ci[3]; p[3] = ci[1]; }
    __device__ static void intrinsics(const double* p, const double*, double& focal, double& aspect, double& ppx, double& ppy) {
        focal = p[0]; ppx = p[1]; ppy = p[2]; aspect = p[3];
    }
    // the bit of refine_flags that frees intrinsic q (focal, ppx, ppy, aspect): OpenCV's refinement mask (0,0), (0,2), (1,2), (1,1)
    __device__ static bool refined(int flags, int q) { return q >= 4 || (flags & (q == 0 ? 1 : (q == 1 ? 4 : (q == 2 ? 16 : 8)))) != 0; }

    // H of every edge with an inlier at `p`: variant 0, and with jac the 28 perturbed ones (columns 0 - 6 camera from, 7 - 13 camera to); a
    // column that is not refined has no H and stays zero in J
    __device__ static void cam_mats(const BaCtx& x, const double* p, bool jac) {
        const int per = jac ? RP_VAR : 1;
        for (int w = x.tid; w < x.pc * per; w += THREADS) {
            const int k = w / per, v = w % per;
            if (x.ptab[3 * k] == 0) continue;
            const BaPair& P = x.prs[k];
            double a[7], b[7];
#pragma unroll
            for (int e = 0; e < 7; ++e) { a[e] = p[7 * P.from + e]; b[e] = p[7 * P.to + e]; }
            if (v > 0) {
                const int col = (v - 1) >> 1, q = col >= 7 ? col - 7 : col;
                if (!refined(x.flags, q)) continue;
                const double val = col >= 7 ? b[q] : a[q];
                const double moved = ((v - 1) & 1) ? val + STEP : val - STEP;
#pragma unroll
                for (int e = 0; e < 7; ++e) { a[e] = (col < 7 && e == q) ? moved : a[e]; b[e] = (col >= 7 && e == q) ? moved : b[e]; }
            }
            double H[9];
            bm_reproj_h(a, b, H);
#pragma unroll
            for (int e = 0; e < 9; ++e) x.hmat[((long long)k * RP_VAR + v) * 9 + e] = H[e];
        }
    }

    __device__ static void matches(const BaCtx& x, bool jac) {
        constexpr int JROW = 30;
        const int M = x.ctl[C_M];
        const double h2 = 2.0 * STEP;
        for (int idx = x.tid; idx < M; idx += THREADS) {
            const double* const H = x.hmat + (long long)x.match_pair[idx] * (RP_VAR * 9);
            const float4 pt = x.pts[idx];
            const double x1 = (double)pt.x, y1 = (double)pt.y, x2 = (double)pt.z, y2 = (double)pt.w;
            double* const out = x.jrow + (long long)idx * JROW;
            double e[2];
            bm_reproj_err(H, x1, y1, x2, y2, e);
            out[0] = e[0]; out[1] = e[1];
            if (!jac) continue;
            for (int col = 0; col < 14; ++col) {
                double d0 = 0.0, d1 = 0.0;
                if (refined(x.flags, col >= 7 ? col - 7 : col)) {
                    double e0[2], e1[2];
                    bm_reproj_err(H + (1 + 2 * col) * 9, x1, y1, x2, y2, e0);
                    bm_reproj_err(H + (2 + 2 * col) * 9, x1, y1, x2, y2, e1);
                    d0 = (e1[0] - e0[0]) / h2; d1 = (e1[1] - e0[1]) / h2;
                }
                out[2 + col] = d0; out[2 + 14 + col] = d1;
            }
        }
    }
};
static_assert(BaK<RayTr>::ENT == 45 && BaK<RayTr>::JROW == 27 && BaK<ReprojTr>::ENT == 120 && BaK<ReprojTr>::JROW == 30, "the tiles of both adjusters");

// (a, b), a <= b, of the upper triangle of the W x W block, rows in order
template <int W>
__device__ __forceinline__ int ba_upper(int a, int b) { return W * a - (a * (a - 1)) / 2 + (b - a); }

// a tile's partial sums over its matches in order, the residuals of each in order: all ENT with jac, the sum of err^2 alone without
template <class Tr>
__device__ void ba_tiles(const BaCtx& x, bool jac) {
    constexpr int W = BaK<Tr>::W, U = BaK<Tr>::U, ENT = BaK<Tr>::ENT, JROW = BaK<Tr>::JROW, RES = Tr::RES;
    const int T = x.ctl[C_T];
    const int per = jac ? ENT : 1;
    for (int w = x.tid; w < T * per; w += Tr::THREADS) {
        const int t = w / per, ent = jac ? w % per : ENT - 1;
        const int p = x.tile_pair[t];
        const int m = x.ptab[3 * p], first = x.ptab[3 * p + 1];
        const int m0 = first + (t - x.ptab[3 * p + 2]) * BA_TILE, m1 = min(m0 + BA_TILE, first + m);
        int ca = 0, cb = 0;                                  // the two columns of a row that are multiplied (< 0: err, else a column of J)
        if (ent < U) {
            int a = 0, rest = ent;
            while (rest >= W - a) { rest -= W - a; ++a; }
            ca = a; cb = a + rest;
        } else if (ent < U + W) {
            ca = ent - U; cb = -1;
        } else {
            ca = -1; cb = -1;
        }
        double s = 0.0;
        for (int idx = m0; idx < m1; ++idx) {
            const double* row = x.jrow + (long long)idx * JROW;
#pragma unroll
            for (int k = 0; k < RES; ++k) {
                const double u = ca < 0 ? row[k] : row[RES + W * k + ca];
                const double v = cb < 0 ? row[k] : row[RES + W * k + cb];
                s = s + (u * v);
            }
        }
        x.tiles[(long long)t * ENT + ent] = s;
    }
}

// the sum over the tiles of pair p, in order, of entry `ent`, added to s
template <class Tr>
__device__ __forceinline__ double ba_add_tiles(const BaCtx& x, int p, int ent, double s) {
    const int m = x.ptab[3 * p], t0 = x.ptab[3 * p + 2], t1 = t0 + (m + BA_TILE - 1) / BA_TILE;
    for (int t = t0; t < t1; ++t) s = s + x.tiles[(long long)t * BaK<Tr>::ENT + ent];
    return s;
}

// |err| from the tiles' sums of err^2, all tiles in order, into dctl[D_ENORM]: the block fetches a thread's worth of them at a time into LDS
// (prow is free outside ba_step) and thread 0 adds them in order - one memory latency a chunk, not one a tile.  Called by every thread.
template <class Tr>
__device__ void ba_err_norm(const BaCtx& x) {
    constexpr int ENT = BaK<Tr>::ENT, THREADS = Tr::THREADS;
    const int T = x.ctl[C_T];
    double s = 0.0;
    for (int t0 = 0; t0 < T; t0 += THREADS) {
        if (t0 + x.tid < T) x.prow[x.tid] = x.tiles[(long long)(t0 + x.tid) * ENT + (ENT - 1)];
        __syncthreads();
        if (x.tid == 0) {
            const int m = min(THREADS, T - t0);
            for (int u = 0; u < m; ++u) s = s + x.prow[u];
        }
        __syncthreads();
    }
    if (x.tid == 0) x.dctl[D_ENORM] = sqrt(s);
}

// JtJ (upper triangle computed, mirrored) and JtErr from the tiles: per camera the edges that touch it in edge order
template <class Tr>
__device__ void ba_assemble(const BaCtx& x) {
    constexpr int PC = Tr::PC, W = BaK<Tr>::W, U = BaK<Tr>::U;
    const int n = x.n, N = x.N;
    for (int w = x.tid; w < N * N; w += Tr::THREADS) {
        const int A = w / N, B = w % N;
        if (A > B) continue;
        const int c = A / PC, a = A % PC, d = B / PC, b = B % PC;
        double s = 0.0;
        if (c == d) {
            for (int o = 0; o < n; ++o) {
                if (o == c) continue;
                const int p = x.slot[min(o, c) * BA_MAXN + max(o, c)];
                if (p < 0) continue;
                const int off = o < c ? PC : 0;
                s = ba_add_tiles<Tr>(x, p, ba_upper<W>(off + a, off + b), s);
            }
        } else {
            const int p = x.slot[c * BA_MAXN + d];
            if (p >= 0) s = ba_add_tiles<Tr>(x, p, ba_upper<W>(a, PC + b), s);
        }
        x.jtj[(long long)A * N + B] = s;
        x.jtj[(long long)B * N + A] = s;
    }
    if (x.tid < N) {
        const int c = x.tid / PC, a = x.tid % PC;
        double s = 0.0;
        for (int o = 0; o < n; ++o) {
            if (o == c) continue;
            const int p = x.slot[min(o, c) * BA_MAXN + max(o, c)];
            if (p < 0) continue;
            s = ba_add_tiles<Tr>(x, p, U + (o < c ? PC : 0) + a, s);
        }
        x.bvec[x.tid] = s;
    }
}

// step(): JtJN = JtJ with the diagonal times 1 + lambda; Cholesky with the trace rule; the two substitutions; param = prev - d.  Threads
// past the last row only keep the barriers.
__device__ void ba_step(const BaCtx& x, double lambda) {
    const int N = x.N, r = x.tid;
    const double scale = 1.0 + lambda;
    if (r == 0) {
        double tr = 0.0;
        for (int k = 0; k < N; ++k) tr = tr + (x.jtj[(long long)k * N + k] * scale);
        x.dctl[D_THRESH] = tr * (2.0 * DBL_EPSILON);
    }
    if (r < N) x.kept[r] = 0;
    __syncthreads();
    const double thresh = x.dctl[D_THRESH];
    double my_diag = 0.0;                                    // L[r][r]
    for (int k = 0; k < N; ++k) {
        if (r < k && x.kept[r]) x.prow[r] = x.lt[(long long)r * N + k];      // row k of L, columns < k
        __syncthreads();
        double v = 0.0;
        if (r >= k && r < N) {
            // the sum in index order; eight loads of L are issued before the first is used, so their latencies overlap (a dropped column's
            // entries are loaded and not used)
            double s = 0.0;
            int m = 0;
            for (; m + 8 <= k; m += 8) {
                double l[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) l[u] = x.lt[(long long)(m + u) * N + r];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (x.kept[m + u]) s = s + (l[u] * x.prow[m + u]);
            }
            for (; m < k; ++m)
                if (x.kept[m]) s = s + (x.lt[(long long)m * N + r] * x.prow[m]);
            const double akk = r == k ? x.jtj[(long long)k * N + k] * scale : x.jtj[(long long)r * N + k];
            v = akk - s;
            if (r == k) {
                const int keep = v > thresh ? 1 : 0;
                x.ctl[C_KEEP] = keep;
                if (keep) { my_diag = sqrt(v); x.dctl[D_PIV] = my_diag; }
                else x.ctl[C_STATUS] |= ISX_BUNDLE_DROPPED;
            }
        }
        __syncthreads();
        if (x.ctl[C_KEEP]) {
            if (r == k) { x.kept[k] = 1; x.lt[(long long)k * N + k] = my_diag; }
            else if (r > k && r < N) x.lt[(long long)k * N + r] = v / x.dctl[D_PIV];
        }
        __syncthreads();
    }
    // L y = JtErr: row r keeps its running sum; y[k] goes round through bc
    double s = 0.0, my_y = 0.0;
    for (int k = 0; k < N; ++k) {
        if (!x.kept[k]) continue;                            // uniform: kept[] is in LDS and complete
        if (r == k) { my_y = (x.bvec[k] - s) / my_diag; x.bc[k] = my_y; }
        __syncthreads();
        if (r > k && r < N) s = s + (x.lt[(long long)k * N + r] * x.bc[k]);
    }
    __syncthreads();
    // L^T d = y: the sum of row r runs over the unknowns in the order they become known, descending
    s = 0.0;
    for (int k = N - 1; k >= 0; --k) {
        if (!x.kept[k]) { if (r == k) x.bc[k] = 0.0; continue; }
        if (r == k) x.bc[k] = (my_y - s) / my_diag;
        __syncthreads();
        if (r < k) s = s + (x.lt[(long long)r * N + k] * x.bc[k]);
    }
    __syncthreads();
    if (r < N) x.param[r] = x.prev[r] - x.bc[r];
    __syncthreads();
}

__device__ void ba_passthrough(const BaCall& c, const BaRig& rig, int tid) {
    if (tid < rig.n) {
        const long long img = rig.img_first + tid;
        const double* ci = row_ptr(c.cin, img, c.cin_step);
        double* co = row_ptr(c.cout, img, c.cout_step);
        float* ko = row_ptr(c.kr, img, c.kr_step);
        double v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = ci[e];
#pragma unroll
        for (int e = 0; e < 16; ++e) co[e] = v[e];
        ko[0] = (float)v[0]; ko[1] = 0.f; ko[2] = (float)v[2];
        ko[3] = 0.f; ko[4] = (float)(v[0] * v[1]); ko[5] = (float)v[3];
        ko[6] = 0.f; ko[7] = 0.f; ko[8] = 1.f;
#pragma unroll
        for (int e = 0; e < 9; ++e) ko[9 + e] = (float)v[4 + e];
    }
}

template <class Tr>
__global__ __launch_bounds__(Tr::THREADS) void k_ba_rigs(BaCall c) {
    constexpr int BA_THREADS = Tr::THREADS, BA_MAXP = BaK<Tr>::MAXP, BA_ENT = BaK<Tr>::ENT, BA_JROW = BaK<Tr>::JROW, PC = Tr::PC;
    __shared__ double Hs[Tr::HS];                            // the camera matrices of Tr::cam_mats; the rotations of the last phase
    __shared__ double fv[Tr::FV];
    __shared__ double param[BA_MAXP], prev[BA_MAXP], bvec[BA_MAXP], bc[BA_MAXP], prow[BaK<Tr>::PROW];
    __shared__ double dctl[D_N];
    __shared__ short slot[BA_MAXN * BA_MAXN];                // [i * 64 + j], i < j: the edge's pair in the rig's table, -1 where there is none
    __shared__ int ctl[C_N];
    __shared__ unsigned char kept[BA_MAXP];

    const int tid = (int)threadIdx.x;
    const BaRig rig = c.rigs[blockIdx.x];
    const int n = rig.n, pc = rig.pair_count, N = PC * n;
    const BaImg* const imgs = c.imgs + rig.img_first;
    BaCtx x;
    x.Hs = Hs; x.fv = fv; x.param = param; x.prev = prev; x.bvec = bvec; x.bc = bc; x.prow = prow; x.dctl = dctl;
    x.slot = slot; x.ctl = ctl; x.kept = kept;
    x.prs = c.pairs + rig.pair_first; x.sizes = c.sizes + 2ll * rig.img_first; x.ptab = c.pair_tab + 3ll * rig.pair_first;
    float4* const pts = c.pts + rig.match_first;
    int* const match_pair = c.match_pair + rig.match_first;
    int* const tile_pair = c.tile_pair + rig.tile_first;
    x.pts = pts; x.match_pair = match_pair; x.jrow = c.jrow + rig.match_first * BA_JROW;
    x.tiles = c.tiles + rig.tile_first * BA_ENT; x.tile_pair = tile_pair;
    x.jtj = c.jtj + rig.mat_first; x.lt = c.lt + rig.mat_first;
    x.hmat = c.hmat + (long long)rig.pair_first * Tr::HMAT;
    x.n = n; x.N = N; x.tid = tid; x.pc = pc; x.flags = c.refine_flags;

    for (int i = tid; i < BA_MAXN * BA_MAXN; i += BA_THREADS) slot[i] = -1;
    if (tid < C_N) ctl[tid] = 0;
    if (tid < D_N) dctl[tid] = 0.0;
    __syncthreads();

    // ---- the edges: pairs in (i, j) order with confidence > conf_thresh; their inliers counted, laid out densely, gathered ----
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = tid; k < pc; k += BA_THREADS) {
            const BaPair P = x.prs[k];
            int m = 0;
            if (c.conf[P.row] > c.conf_thresh) {
                const int cnt = min(max(c.counts[P.row], 0), P.cap);     // a count above its mats' rows is clamped, a negative one is 0
                const BaImg I = imgs[P.from], J = imgs[P.to];
                const int first = pass ? x.ptab[3 * k + 1] : 0;
                for (int r = 0; r < cnt; ++r) {
                    if (row_ptr(P.mask, r, P.mask_step)[0] == 0) continue;
                    const int* mr = row_ptr(P.matches, r, P.matches_step);
                    const int q = mr[0], t = mr[1];
                    if ((unsigned)q >= (unsigned)I.rows || (unsigned)t >= (unsigned)J.rows) continue;      // outside the keypoints: no inlier
                    if (pass) {
                        const float* a = row_ptr(I.kp, q, I.kp_step);
                        const float* b = row_ptr(J.kp, t, J.kp_step);
                        pts[first + m] = make_float4(a[0], a[1], b[0], b[1]);
                        match_pair[first + m] = k;
                    }
                    ++m;
                }
                if (!pass) { slot[P.from * BA_MAXN + P.to] = (short)k; atomicAdd(&ctl[C_EDGES], 1); }
                else for (int t = 0; t < (m + BA_TILE - 1) / BA_TILE; ++t) tile_pair[x.ptab[3 * k + 2] + t] = k;
            }
            if (!pass) x.ptab[3 * k] = m;
        }
        __syncthreads();
        if (!pass && tid == 0) {
            int d = 0, t = 0;
            for (int k = 0; k < pc; ++k) {
                const int m = x.ptab[3 * k];
                x.ptab[3 * k + 1] = d; x.ptab[3 * k + 2] = t;
                d += m; t += (m + BA_TILE - 1) / BA_TILE;
            }
            ctl[C_M] = d; ctl[C_T] = t;
            const int* est = row_ptr(c.est, (long long)blockIdx.x, c.est_step);
            const int center = est[2];
            int status = 0;
            if ((est[0] & ISX_ESTIMATOR_ASSERT) || center < 0 || center >= n) status |= ISX_BUNDLE_EST_ASSERT;
            if (ctl[C_EDGES] == 0) status |= ISX_BUNDLE_NO_EDGES;
            ctl[C_STATUS] = status; ctl[C_CENTER] = center;
            ctl[C_LG] = -3;
        }
        __syncthreads();
    }

    int* const rs = row_ptr(c.rs, (long long)blockIdx.x, c.rs_step);
    double* const re = row_ptr(c.re, (long long)blockIdx.x, c.re_step);
    if (ctl[C_STATUS] != 0) {                                // the reference would have asserted: the cameras pass through
        ba_passthrough(c, rig, tid);
        if (tid < 8) rs[tid] = tid == 0 ? ctl[C_STATUS] : (tid == 5 ? ctl[C_EDGES] : (tid == 6 ? ctl[C_M] : 0));
        if (tid < 2) re[tid] = 0.0;
        return;
    }

    // ---- setUpInitialCameraParams ----
    if (tid < n) {
        const double* ci = row_ptr(c.cin, (long long)rig.img_first + tid, c.cin_step);
        double R[9], Q[9], rv[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = (double)(float)ci[4 + e];      // W:183-188
        if (!bm_polar(R, Q)) atomicOr(&ctl[C_STATUS], ISX_BUNDLE_SINGULAR_R);
        bm_rodrigues_vec(Q, rv);
        Tr::init_param(ci, param + PC * tid);
#pragma unroll
        for (int e = 0; e < 3; ++e) param[PC * tid + Tr::RV + e] = (double)(float)rv[e];
    }
    __syncthreads();

    // ---- CvLevMarq ----
    for (;;) {
        Tr::cam_mats(x, param, true);
        __syncthreads();
        Tr::matches(x, true);
        __syncthreads();
        ba_tiles<Tr>(x, true);
        __syncthreads();
        ba_assemble<Tr>(x);
        ba_err_norm<Tr>(x);
        if (tid < N) prev[tid] = param[tid];
        __syncthreads();
        if (tid == 0) {
            ++ctl[C_JEV]; ++ctl[C_EEV];
            if (ctl[C_ITERS] == 0) { dctl[D_PREVNORM] = dctl[D_ENORM]; dctl[D_FIRST] = dctl[D_ENORM]; }
        }
        for (;;) {                                           // step(), calcError, CHECK_ERR: 33 times an iteration at the most
            ba_step(x, BA_LAMBDA[ctl[C_LG] + 16]);
            Tr::cam_mats(x, param, false);
            __syncthreads();
            Tr::matches(x, false);
            __syncthreads();
            ba_tiles<Tr>(x, false);
            __syncthreads();
            ba_err_norm<Tr>(x);
            if (tid == 0) {
                ++ctl[C_EEV];
                int again = 0;
                if (dctl[D_ENORM] > dctl[D_PREVNORM]) {
                    if (++ctl[C_LG] <= 16) again = 1;
                }
                ctl[C_AGAIN] = again;
            }
            __syncthreads();
            if (!ctl[C_AGAIN]) break;
        }
        if (tid == 0) {
            ctl[C_LG] = max(ctl[C_LG] - 1, -16);
            const int iters = ++ctl[C_ITERS];
            bool nan = false;
            double dn = 0.0, pn = 0.0;
            for (int k = 0; k < N; ++k) {
                const double p = param[k], q = prev[k], d = p - q;
                nan = nan || p != p;
                dn = dn + (d * d);
                pn = pn + (q * q);
            }
            int done = iters >= c.max_iter || nan;
            if (!done && sqrt(dn) / sqrt(pn) < c.eps) done = 1;
            if (!done) dctl[D_PREVNORM] = dctl[D_ENORM];
            ctl[C_DONE] = done; ctl[C_NAN] = nan ? 1 : 0;
        }
        __syncthreads();
        if (ctl[C_DONE]) break;
    }

    // ---- the NaN check, obtainRefinedCameraParams, R_i = R_center.inv() * R_i ----
    const bool nan = ctl[C_NAN] != 0;
    if (nan) {
        ba_passthrough(c, rig, tid);
    } else {
        if (tid < n) {
            double R[9];
            bm_rodrigues_mat(param + PC * tid + Tr::RV, R);
#pragma unroll
            for (int e = 0; e < 9; ++e) Hs[9 * tid + e] = (double)(float)R[e];
        }
        __syncthreads();
        if (tid < n) {
            const long long img = rig.img_first + tid;
            const double* ci = row_ptr(c.cin, img, c.cin_step);
            double* co = row_ptr(c.cout, img, c.cout_step);
            float* ko = row_ptr(c.kr, img, c.kr_step);
            double Rc[9], Ri[9], Rinv[9], o[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) { Rc[e] = Hs[9 * ctl[C_CENTER] + e]; Ri[e] = Hs[9 * tid + e]; }
            es_inv3(Rc, Rinv);
            es_mul3(Rinv, Ri, o);
            const double t0 = ci[13], t1 = ci[14], t2 = ci[15];
            double focal, aspect, ppx, ppy;
            Tr::intrinsics(param + PC * tid, ci, focal, aspect, ppx, ppy);
            co[0] = focal; co[1] = aspect; co[2] = ppx; co[3] = ppy;
#pragma unroll
            for (int e = 0; e < 9; ++e) { const float f = (float)o[e]; co[4 + e] = (double)f; ko[9 + e] = f; }
            co[13] = t0; co[14] = t1; co[15] = t2;
            ko[0] = (float)focal; ko[1] = 0.f; ko[2] = (float)ppx;
            ko[3] = 0.f; ko[4] = (float)(focal * aspect); ko[5] = (float)ppy;
            ko[6] = 0.f; ko[7] = 0.f; ko[8] = 1.f;
        }
    }
    if (tid < 8) {
        int v = ctl[C_STATUS] | (nan ? ISX_BUNDLE_NAN : 0);
        v = tid == 1 ? ctl[C_ITERS] : v; v = tid == 2 ? ctl[C_JEV] : v; v = tid == 3 ? ctl[C_EEV] : v; v = tid == 4 ? ctl[C_LG] : v;
        v = tid == 5 ? ctl[C_EDGES] : v; v = tid == 6 ? ctl[C_M] : v; v = tid == 7 ? 0 : v;
        rs[tid] = v;
    }
    if (tid < 2) re[tid] = tid == 0 ? dctl[D_FIRST] : dctl[D_ENORM];
}

struct BaScratch : UploadScratch {};     // pin: the tables and the staged rows of host input mats (scratch.hpp)

template <class Tr>
int ba_call(int num_images, const int* image_sizes_wh, const isx_mat* keypoints, int num_pairs, const int* pairs_from_to, const isx_mat* matches,
            const isx_mat* inlier_masks, const isx_mat* counts, const isx_mat* stats, const isx_mat* conf, int num_rigs, const int* rig_first,
            const isx_mat* est_rig_stats, const isx_mat* cameras_in, double conf_thresh, int max_iter, double eps, int refine_flags,
            isx_mat* cameras_out, isx_mat* kr32_out, isx_mat* rig_stats_out, isx_mat* rig_err_out, int* info, int device, void* hip_stream) {
    constexpr int BA_THREADS = Tr::THREADS, BA_ENT = BaK<Tr>::ENT, BA_JROW = BaK<Tr>::JROW, PC = Tr::PC;
    const char* who = Tr::who();
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(image_sizes_wh && keypoints && counts && stats && conf && est_rig_stats && cameras_in && cameras_out && kr32_out && rig_stats_out && rig_err_out,
                  ISX_ERR_INVALID, "%s: null image_sizes_wh, keypoints, counts, stats, conf, est_rig_stats, cameras_in, cameras_out, kr32_out, rig_stats_out or rig_err_out", who);
    ISX_CHECK_ARG(num_pairs >= 0 && (num_pairs == 0 || (pairs_from_to && matches && inlier_masks)), ISX_ERR_INVALID,
                  "%s: %d pairs, or null pairs_from_to, matches or inlier_masks", who, num_pairs);
    ISX_CHECK_ARG(num_rigs >= 1 && (rig_first || num_rigs == 1), ISX_ERR_INVALID, "%s: %d rigs, or more than one without rig_first", who, num_rigs);
    ISX_CHECK_ARG(num_images >= 2, ISX_ERR_INVALID, "%s: %d images", who, num_images);
    ISX_CHECK_ARG(max_iter >= 1 && max_iter <= 1000, ISX_ERR_INVALID, "%s: max_iter %d is not in [1, 1000]", who, max_iter);
    ISX_CHECK_ARG(conf_thresh >= 0, ISX_ERR_INVALID, "%s: conf_thresh %g is negative or not a number (an edge must have a mask the homography stage wrote)", who, conf_thresh);
    ISX_CHECK_ARG(eps == eps, ISX_ERR_INVALID, "%s: eps is not a number", who);
    ISX_CHECK_ARG(refine_flags >= 0 && refine_flags <= 31, ISX_ERR_INVALID, "%s: refine_flags %d is not in [0, 31]", who, refine_flags);
    std::vector<int> first((size_t)num_rigs + 1);
    for (int r = 0; r <= num_rigs; ++r) first[r] = rig_first ? rig_first[r] : (r == 0 ? 0 : num_images);
    ISX_CHECK_ARG(first[0] == 0 && first[num_rigs] == num_images, ISX_ERR_INVALID, "%s: rig_first runs from %d to %d, not from 0 to %d", who, first[0],
                  first[num_rigs], num_images);
    for (int r = 0; r < num_rigs; ++r) {
        ISX_CHECK_ARG(first[r + 1] > first[r], ISX_ERR_INVALID, "%s: rig_first does not increase at rig %d", who, r);
        ISX_CHECK_ARG(first[r + 1] - first[r] >= 2, ISX_ERR_INVALID, "%s: rig %d has one image", who, r);
    }
    for (int r = 0; r < num_rigs; ++r)
        ISX_CHECK_ARG(first[r + 1] - first[r] <= BA_MAXN, ISX_ERR_UNSUPPORTED, "%s: rig %d has %d images, more than %d", who, r, first[r + 1] - first[r], BA_MAXN);
    std::vector<int> rig_of((size_t)num_images);
    for (int r = 0; r < num_rigs; ++r)
        for (int i = first[r]; i < first[r + 1]; ++i) rig_of[i] = r;
    for (int i = 0; i < num_images; ++i) ISX_CHECK_ARG(keypoints[i].rows >= 0, ISX_ERR_INVALID, "%s: keypoints %d: negative rows", who, i);
    std::vector<long long> seen((size_t)num_pairs);
    for (int p = 0; p < num_pairs; ++p) {
        const int a = pairs_from_to[2 * p], b = pairs_from_to[2 * p + 1];
        ISX_CHECK_ARG(a >= 0 && b >= 0 && a < num_images && b < num_images, ISX_ERR_INVALID, "%s: pair %d (%d, %d) is out of range", who, p, a, b);
        ISX_CHECK_ARG(a < b, ISX_ERR_INVALID, "%s: pair %d (%d, %d): from >= to", who, p, a, b);
        ISX_CHECK_ARG(rig_of[a] == rig_of[b], ISX_ERR_INVALID, "%s: pair %d (%d, %d) crosses rigs %d and %d", who, p, a, b, rig_of[a], rig_of[b]);
        ISX_CHECK_ARG(matches[p].rows >= 0 && inlier_masks[p].rows >= 0, ISX_ERR_INVALID, "%s: pair %d: negative rows", who, p);
        seen[p] = (long long)a * num_images + b;
    }
    std::vector<long long> sorted_seen(seen);
    std::sort(sorted_seen.begin(), sorted_seen.end());
    ISX_CHECK_ARG(std::adjacent_find(sorted_seen.begin(), sorted_seen.end()) == sorted_seen.end(), ISX_ERR_INVALID, "%s: a pair is listed twice", who);
    for (int i = 0; i < num_images; ++i) ISX_TRY(check_mat_holds(keypoints[i], ISX_32FC1, 0, 2, 4, STOP_NO_ROW_PRESENT, device, who, "keypoints", i));
    for (int p = 0; p < num_pairs; ++p) {
        ISX_TRY(check_mat_holds(matches[p], ISX_32SC1, 0, 3, 4, STOP_NO_ROW_PRESENT, device, who, "matches", p));
        ISX_TRY(check_mat_holds(inlier_masks[p], ISX_8UC1, 0, 1, 1, STOP_NO_ROW_PRESENT, device, who, "inlier_masks", p));
    }
    ISX_TRY(check_mat_holds(*counts, ISX_32SC1, num_pairs > 0 ? 1 : 0, num_pairs, 4, STOP_NO_ROW_WANTED, device, who, "counts", 0));
    ISX_TRY(check_mat_holds(*stats, ISX_32SC1, num_pairs, 2, 4, STOP_NO_ROW_WANTED, device, who, "stats", 0));
    ISX_TRY(check_mat_holds(*conf, ISX_64FC1, num_pairs > 0 ? 1 : 0, num_pairs, 8, STOP_NO_ROW_WANTED, device, who, "conf", 0));
    ISX_TRY(check_mat_holds(*est_rig_stats, ISX_32SC1, num_rigs, 8, 4, STOP_NO_ROW_WANTED, device, who, "est_rig_stats", 0));
    ISX_TRY(check_mat_holds(*cameras_in, ISX_64FC1, num_images, 16, 8, STOP_NO_ROW_WANTED, device, who, "cameras_in", 0));
    ISX_TRY(check_mat_holds(*cameras_out, ISX_64FC1, num_images, 16, 8, STOP_NO_ROW_WANTED, device, who, "cameras_out", 0));
    ISX_TRY(check_mat_holds(*kr32_out, ISX_32FC1, num_images, 18, 4, STOP_NO_ROW_WANTED, device, who, "kr32_out", 0));
    ISX_TRY(check_mat_holds(*rig_stats_out, ISX_32SC1, num_rigs, 8, 4, STOP_NO_ROW_WANTED, device, who, "rig_stats_out", 0));
    ISX_TRY(check_mat_holds(*rig_err_out, ISX_64FC1, num_rigs, 2, 8, STOP_NO_ROW_WANTED, device, who, "rig_err_out", 0));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_TRY(refuse_capture(st, who, "the call uploads its tables and may stage host mats"));

    // ---- the tables: per rig its pairs sorted by (from, to), the order of the edges ----
    std::vector<BaRig> rigs((size_t)num_rigs);
    std::vector<BaPair> prs((size_t)std::max(num_pairs, 1));
    std::vector<BaImg> imgs((size_t)num_images);
    std::vector<int> order((size_t)num_pairs);
    for (int p = 0; p < num_pairs; ++p) order[p] = p;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return seen[a] < seen[b]; });      // by (from, to): by rig, then index order
    for (int r = 0; r < num_rigs; ++r) rigs[r] = BaRig{first[r], first[r + 1] - first[r], 0, 0, 0, 0, 0};
    for (int p = 0; p < num_pairs; ++p) ++rigs[rig_of[pairs_from_to[2 * p]]].pair_count;
    std::vector<int> cap((size_t)std::max(num_pairs, 1), 0);
    long long match_total = 0, tile_total = 0, mat_total = 0;
    {
        int at = 0;
        for (int r = 0; r < num_rigs; ++r) {
            rigs[r].pair_first = at; rigs[r].match_first = match_total; rigs[r].tile_first = tile_total; rigs[r].mat_first = mat_total;
            for (int k = 0; k < rigs[r].pair_count; ++k, ++at) {
                const int p = order[at];
                cap[at] = std::min(matches[p].rows, inlier_masks[p].rows);
                match_total += cap[at];
                tile_total += cap[at] > 0 ? cap[at] / BA_TILE + 1 : 0;
            }
            mat_total += (long long)(PC * PC) * rigs[r].n * rigs[r].n;
        }
    }
    StagedMat m_counts, m_conf, m_est, m_cin, m_cout, m_kr, m_rs, m_re;
    std::vector<StagedMat> m_kp((size_t)num_images), m_mt((size_t)std::max(num_pairs, 1)), m_mk((size_t)std::max(num_pairs, 1));
    Bump lay;
    const size_t o_rigs = lay.take(rigs.size() * sizeof(BaRig));
    const size_t o_prs = lay.take(prs.size() * sizeof(BaPair));
    const size_t o_imgs = lay.take(imgs.size() * sizeof(BaImg));
    const size_t o_sizes = lay.take((size_t)num_images * 8);
    if (num_pairs > 0) {
        m_counts.plan(lay, *counts, 1, (size_t)num_pairs * 4);
        m_conf.plan(lay, *conf, 1, (size_t)num_pairs * 8);
    }
    m_est.plan(lay, *est_rig_stats, num_rigs, 32);
    m_cin.plan(lay, *cameras_in, num_images, 128);
    for (int i = 0; i < num_images; ++i) m_kp[i].plan(lay, keypoints[i], keypoints[i].rows, 8);
    for (int at = 0; at < num_pairs; ++at) {
        m_mt[at].plan(lay, matches[order[at]], cap[at], 12);
        m_mk[at].plan(lay, inlier_masks[order[at]], cap[at], 1);
    }
    const size_t upload_bytes = lay.at;
    const size_t o_pts = lay.take((size_t)std::max(match_total, 1ll) * 16);
    const size_t o_mpair = lay.take((size_t)std::max(match_total, 1ll) * 4);
    const size_t o_jrow = lay.take((size_t)std::max(match_total, 1ll) * BA_JROW * 8);
    const size_t o_tiles = lay.take((size_t)std::max(tile_total, 1ll) * BA_ENT * 8);
    const size_t o_tpair = lay.take((size_t)std::max(tile_total, 1ll) * 4);
    const size_t o_ptab = lay.take((size_t)std::max(num_pairs, 1) * 12);
    const size_t o_jtj = lay.take((size_t)mat_total * 8);
    const size_t o_lt = lay.take((size_t)mat_total * 8);
    const size_t o_hmat = lay.take((size_t)std::max(num_pairs, 1) * Tr::HMAT * 8);
    m_cout.plan(lay, *cameras_out, num_images, 128);
    m_kr.plan(lay, *kr32_out, num_images, 72);
    m_rs.plan(lay, *rig_stats_out, num_rigs, 32);
    m_re.plan(lay, *rig_err_out, num_rigs, 16);

    BaScratch& s = per_thread<BaScratch>();
    ISX_TRY(s.begin(device, st, lay.at, upload_bytes));
    char* const dev = (char*)s.work.p;
    char* const pin = (char*)s.pin.p;
    for (int i = 0; i < num_images; ++i) {
        BaImg& I = imgs[i];
        std::memset(&I, 0, sizeof(I));
        I.rows = keypoints[i].rows;
        if (I.rows == 0) continue;
        m_kp[i].fill(pin);
        m_kp[i].bind(dev, I.kp, I.kp_step);
    }
    for (int at = 0; at < num_pairs; ++at) {
        const int p = order[at], r = rig_of[pairs_from_to[2 * p]];
        BaPair& P = prs[at];
        std::memset(&P, 0, sizeof(P));
        P.from = pairs_from_to[2 * p] - first[r]; P.to = pairs_from_to[2 * p + 1] - first[r]; P.row = p; P.cap = cap[at];
        if (cap[at] == 0) continue;
        m_mt[at].fill(pin);
        m_mk[at].fill(pin);
        m_mt[at].bind(dev, P.matches, P.matches_step);
        m_mk[at].bind(dev, P.mask, P.mask_step);
    }
    std::memcpy(pin + o_rigs, rigs.data(), rigs.size() * sizeof(BaRig));
    std::memcpy(pin + o_prs, prs.data(), prs.size() * sizeof(BaPair));
    std::memcpy(pin + o_imgs, imgs.data(), imgs.size() * sizeof(BaImg));
    std::memcpy(pin + o_sizes, image_sizes_wh, (size_t)num_images * 8);
    m_counts.fill(pin);
    m_conf.fill(pin);
    m_est.fill(pin);
    m_cin.fill(pin);
    ISX_TRY(s.upload(st, upload_bytes));

    // ---- one launch ----
    BaCall c;
    std::memset(&c, 0, sizeof(c));
    c.rigs = (const BaRig*)(dev + o_rigs); c.pairs = (const BaPair*)(dev + o_prs); c.imgs = (const BaImg*)(dev + o_imgs); c.sizes = (const int*)(dev + o_sizes);
    if (num_pairs > 0) {
        m_counts.bind(dev, c.counts);
        m_conf.bind(dev, c.conf);
    }
    m_est.bind(dev, c.est, c.est_step);
    m_cin.bind(dev, c.cin, c.cin_step);
    m_cout.bind(dev, c.cout, c.cout_step);
    m_kr.bind(dev, c.kr, c.kr_step);
    m_rs.bind(dev, c.rs, c.rs_step);
    m_re.bind(dev, c.re, c.re_step);
    c.pts = (float4*)(dev + o_pts); c.match_pair = (int*)(dev + o_mpair); c.jrow = (double*)(dev + o_jrow);
    c.tiles = (double*)(dev + o_tiles); c.tile_pair = (int*)(dev + o_tpair); c.pair_tab = (int*)(dev + o_ptab);
    c.jtj = (double*)(dev + o_jtj); c.lt = (double*)(dev + o_lt); c.hmat = (double*)(dev + o_hmat);
    c.conf_thresh = conf_thresh; c.eps = eps; c.max_iter = max_iter; c.refine_flags = refine_flags;
    ISX_LAUNCH(Tr::kernel(), (double)match_total * 24.0 + (double)num_images * 272.0, st, k_ba_rigs<Tr>, dim3((unsigned)num_rigs), dim3(BA_THREADS), 0, c);
    ISX_TRY(s.ran(st));

    // ---- host outputs ----
    if (m_cout.staged || m_kr.staged || m_rs.staged || m_re.staged) {
        ISX_TRY(m_cout.back(dev, num_images, st));
        ISX_TRY(m_kr.back(dev, num_images, st));
        ISX_TRY(m_rs.back(dev, num_rigs, st));
        ISX_TRY(m_re.back(dev, num_rigs, st));
        ISX_HIP(hipStreamSynchronize(st));
    }
    if (info) { info[0] = num_rigs; info[1] = 1; }
    return ISX_OK;
}

// ---- waveCorrect: one block a rig; thread 0 finds the correction (sums in image order, a 3 x 3 Jacobi), a thread per image applies it --------
struct WvCall {
    const int* first;
    const double* cin; long long cin_step;
    double* cout; long long cout_step;
    float* kr; long long kr_step;
    int* rs; long long rs_step;
    int kind;
};
constexpr int WV_THREADS = 64;

__device__ __forceinline__ float wv_r(const WvCall& c, long long img, int e) { return (float)row_ptr(c.cin, img, c.cin_step)[4 + e]; }

__global__ __launch_bounds__(WV_THREADS) void k_wave_rigs(WvCall c) {
    __shared__ float Rw[9];
    __shared__ int status;
    const int tid = (int)threadIdx.x;
    const long long i0 = c.first[blockIdx.x];
    const int n = c.first[blockIdx.x + 1] - c.first[blockIdx.x];
    if (tid == 0) {
        int st = n <= 1 ? ISX_WAVE_SINGLE : 0;
        if (st == 0) {
            float moment[9], V[9], Wv[3], k[3] = {0.f, 0.f, 0.f};
            for (int e = 0; e < 9; ++e) moment[e] = 0.f;
            for (int i = 0; i < n; ++i) {
                const float col[3] = {wv_r(c, i0 + i, 0), wv_r(c, i0 + i, 3), wv_r(c, i0 + i, 6)};
                for (int r = 0; r < 3; ++r)
                    for (int q = 0; q < 3; ++q) moment[3 * r + q] = moment[3 * r + q] + (col[r] * col[q]);
                k[0] = k[0] + wv_r(c, i0 + i, 2); k[1] = k[1] + wv_r(c, i0 + i, 5); k[2] = k[2] + wv_r(c, i0 + i, 8);
            }
            bm_jacobi3f(moment, V, Wv);
            const int row = c.kind == ISX_WAVE_CORRECT_HORIZ ? 2 : 0;
            float rg1[3] = {V[3 * row], V[3 * row + 1], V[3 * row + 2]};
            float rg0[3] = {(rg1[1] * k[2]) - (rg1[2] * k[1]), (rg1[2] * k[0]) - (rg1[0] * k[2]), (rg1[0] * k[1]) - (rg1[1] * k[0])};
            const float nrm = sqrtf(((rg0[0] * rg0[0]) + (rg0[1] * rg0[1])) + (rg0[2] * rg0[2]));
            if ((double)nrm <= DBL_MIN) {
                st = ISX_WAVE_DEGENERATE;
            } else {
                for (int e = 0; e < 3; ++e) rg0[e] = rg0[e] / nrm;
                const float rg2[3] = {(rg0[1] * rg1[2]) - (rg0[2] * rg1[1]), (rg0[2] * rg1[0]) - (rg0[0] * rg1[2]), (rg0[0] * rg1[1]) - (rg0[1] * rg1[0])};
                const float* const rg = c.kind == ISX_WAVE_CORRECT_HORIZ ? rg0 : rg1;
                float conf = 0.f;
                for (int i = 0; i < n; ++i) {
                    const float d = ((rg[0] * wv_r(c, i0 + i, 0)) + (rg[1] * wv_r(c, i0 + i, 3))) + (rg[2] * wv_r(c, i0 + i, 6));
                    conf = c.kind == ISX_WAVE_CORRECT_HORIZ ? conf + d : conf - d;
                }
                if (conf < 0.f)
                    for (int e = 0; e < 3; ++e) { rg0[e] = -rg0[e]; rg1[e] = -rg1[e]; }
                for (int e = 0; e < 3; ++e) { Rw[e] = rg0[e]; Rw[3 + e] = rg1[e]; Rw[6 + e] = rg2[e]; }
            }
        }
        status = st;
        int* const rs = row_ptr(c.rs, (long long)blockIdx.x, c.rs_step);
        rs[0] = st; rs[1] = n;
    }
    __syncthreads();
    const bool pass = status != 0;
    for (int i = tid; i < n; i += WV_THREADS) {
        const double* ci = row_ptr(c.cin, i0 + i, c.cin_step);
        double* co = row_ptr(c.cout, i0 + i, c.cout_step);
        float* ko = row_ptr(c.kr, i0 + i, c.kr_step);
        double v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = ci[e];
        float R[9], o[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = (float)v[4 + e];
        if (pass) {
#pragma unroll
            for (int e = 0; e < 9; ++e) o[e] = R[e];
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) o[3 * r + q] = ((Rw[3 * r] * R[q]) + (Rw[3 * r + 1] * R[3 + q])) + (Rw[3 * r + 2] * R[6 + q]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) co[e] = v[e];
#pragma unroll
        for (int e = 0; e < 9; ++e) { co[4 + e] = pass ? v[4 + e] : (double)o[e]; ko[9 + e] = o[e]; }
#pragma unroll
        for (int e = 13; e < 16; ++e) co[e] = v[e];
        ko[0] = (float)v[0]; ko[1] = 0.f; ko[2] = (float)v[2];
        ko[3] = 0.f; ko[4] = (float)(v[0] * v[1]); ko[5] = (float)v[3];
        ko[6] = 0.f; ko[7] = 0.f; ko[8] = 1.f;
    }
}

int wv_call(int num_images, int num_rigs, const int* rig_first, const isx_mat* cameras_in, int kind, isx_mat* cameras_out, isx_mat* kr32_out,
            isx_mat* rig_stats_out, int* info, int device, void* hip_stream) {
    const char* who = "wave_correct";
    ISX_CHECK_ARG(cameras_in && cameras_out && kr32_out && rig_stats_out, ISX_ERR_INVALID, "%s: null cameras_in, cameras_out, kr32_out or rig_stats_out", who);
    ISX_CHECK_ARG(num_rigs >= 1 && (rig_first || num_rigs == 1), ISX_ERR_INVALID, "%s: %d rigs, or more than one without rig_first", who, num_rigs);
    ISX_CHECK_ARG(num_images >= 1, ISX_ERR_INVALID, "%s: %d images", who, num_images);
    ISX_CHECK_ARG(kind == ISX_WAVE_CORRECT_HORIZ || kind == ISX_WAVE_CORRECT_VERT, ISX_ERR_INVALID, "%s: kind %d is neither horizontal (0) nor vertical (1)", who, kind);
    std::vector<int> first((size_t)num_rigs + 1);
    for (int r = 0; r <= num_rigs; ++r) first[r] = rig_first ? rig_first[r] : (r == 0 ? 0 : num_images);
    ISX_CHECK_ARG(first[0] == 0 && first[num_rigs] == num_images, ISX_ERR_INVALID, "%s: rig_first runs from %d to %d, not from 0 to %d", who, first[0],
                  first[num_rigs], num_images);
    for (int r = 0; r < num_rigs; ++r) ISX_CHECK_ARG(first[r + 1] > first[r], ISX_ERR_INVALID, "%s: rig_first does not increase at rig %d", who, r);
    ISX_TRY(check_mat_holds(*cameras_in, ISX_64FC1, num_images, 16, 8, STOP_NO_ROW_WANTED, device, who, "cameras_in", 0));
    ISX_TRY(check_mat_holds(*cameras_out, ISX_64FC1, num_images, 16, 8, STOP_NO_ROW_WANTED, device, who, "cameras_out", 0));
    ISX_TRY(check_mat_holds(*kr32_out, ISX_32FC1, num_images, 18, 4, STOP_NO_ROW_WANTED, device, who, "kr32_out", 0));
    ISX_TRY(check_mat_holds(*rig_stats_out, ISX_32SC1, num_rigs, 2, 4, STOP_NO_ROW_WANTED, device, who, "rig_stats_out", 0));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_TRY(refuse_capture(st, who, "the call uploads its table and may stage host mats"));

    StagedMat m_cin, m_cout, m_kr, m_rs;
    Bump lay;
    const size_t o_first = lay.take(first.size() * 4);
    m_cin.plan(lay, *cameras_in, num_images, 128);
    const size_t upload_bytes = lay.at;
    m_cout.plan(lay, *cameras_out, num_images, 128);
    m_kr.plan(lay, *kr32_out, num_images, 72);
    m_rs.plan(lay, *rig_stats_out, num_rigs, 8);
    BaScratch& s = per_thread<BaScratch>();
    ISX_TRY(s.begin(device, st, lay.at, upload_bytes));
    char* const dev = (char*)s.work.p;
    char* const pin = (char*)s.pin.p;
    std::memcpy(pin + o_first, first.data(), first.size() * 4);
    m_cin.fill(pin);
    ISX_TRY(s.upload(st, upload_bytes));

    WvCall c;
    std::memset(&c, 0, sizeof(c));
    c.first = (const int*)(dev + o_first);
    m_cin.bind(dev, c.cin, c.cin_step);
    m_cout.bind(dev, c.cout, c.cout_step);
    m_kr.bind(dev, c.kr, c.kr_step);
    m_rs.bind(dev, c.rs, c.rs_step);
    c.kind = kind;
    ISX_LAUNCH("wave_rigs", (double)num_images * 328.0, st, k_wave_rigs, dim3((unsigned)num_rigs), dim3(WV_THREADS), 0, c);
    ISX_TRY(s.ran(st));
    if (m_cout.staged || m_kr.staged || m_rs.staged) {
        ISX_TRY(m_cout.back(dev, num_images, st));
        ISX_TRY(m_kr.back(dev, num_images, st));
        ISX_TRY(m_rs.back(dev, num_rigs, st));
        ISX_HIP(hipStreamSynchronize(st));
    }
    if (info) { info[0] = num_rigs; info[1] = 1; }
    return ISX_OK;
}

// ---- the self-tests of bundle_math.hpp: one item of function fn, by the host's loop and by a thread of k_selftest_bundle_math --------------
constexpr int BM_FNS = 12;
ISX_HD inline int bm_fn_in(int fn) {                         // doubles an item reads
    constexpr int w[BM_FNS] = {1, 1, 1, 3, 9, 9, 6, 11, 9, 9, 14, 13};
    return w[fn];
}
ISX_HD inline int bm_fn_out(int fn) {                        // doubles an item writes
    constexpr int w[BM_FNS] = {1, 1, 1, 9, 3, 10, 9, 3, 12, 12, 9, 2};
    return w[fn];
}

ISX_HD inline void bm_selftest_item(int fn, const double* in, double* out) {
    switch (fn) {
    case 0: out[0] = bm_sin(in[0]); break;
    case 1: out[0] = bm_cos(in[0]); break;
    case 2: out[0] = bm_acos(in[0]); break;
    case 3: bm_rodrigues_mat(in, out); break;                                        // 3 in, 9 out
    case 4: bm_rodrigues_vec(in, out); break;                                        // 9 in, 3 out
    case 5: out[9] = bm_polar(in, out) ? 1.0 : 0.0; break;                           // 9 in, 9 + ok out
    case 6: bm_cam_h(in, (int)in[4], (int)in[5], out); break;                        // f, rvec, width, height in, 9 out
    case 7: bm_ray(in, in[9], in[10], out); break;                                   // H, x, y in, 3 out
    case 8: {                                                                        // A (float32 values) in, V and W out
        float A[9], V[9], W[3];
        for (int e = 0; e < 9; ++e) A[e] = (float)in[e];
        bm_jacobi3f(A, V, W);
        for (int e = 0; e < 9; ++e) out[e] = (double)V[e];
        for (int e = 0; e < 3; ++e) out[9 + e] = (double)W[e];
        break;
    }
    case 9: {                                                                        // A in, V and W out
        double A[9];
        for (int e = 0; e < 9; ++e) A[e] = in[e];
        bm_jacobi3(A, out, out + 9);
        break;
    }
    case 10: bm_reproj_h(in, in + 7, out); break;                                    // p1[7], p2[7] in, 9 out
    default: bm_reproj_err(in, in[9], in[10], in[11], in[12], out); break;           // H, x1, y1, x2, y2 in, 2 out
    }
}

__global__ void __launch_bounds__(256) k_selftest_bundle_math(int fn, int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    bm_selftest_item(fn, in + (size_t)bm_fn_in(fn) * i, out + (size_t)bm_fn_out(fn) * i);
}

}  // namespace

extern "C" {

int isx_bundle_release(void) ISX_ENTRY {
    clear_error();
    return per_thread<BaScratch>().release();
} ISX_EXIT("isx_bundle_release")

int isx_bundle_adjust_ray(int num_images, const int* image_sizes_wh, const isx_mat* keypoints, int num_pairs, const int* pairs_from_to,
                          const isx_mat* matches, const isx_mat* inlier_masks, const isx_mat* counts, const isx_mat* stats, const isx_mat* conf,
                          int num_rigs, const int* rig_first, const isx_mat* est_rig_stats, const isx_mat* cameras_in, double conf_thresh, int max_iter,
                          double eps, isx_mat* cameras_out, isx_mat* kr32_out, isx_mat* rig_stats_out, isx_mat* rig_err_out, int* info, int device,
                          void* hip_stream) ISX_ENTRY {
    clear_error();
    return ba_call<RayTr>(num_images, image_sizes_wh, keypoints, num_pairs, pairs_from_to, matches, inlier_masks, counts, stats, conf, num_rigs, rig_first,
                          est_rig_stats, cameras_in, conf_thresh, max_iter, eps, 0, cameras_out, kr32_out, rig_stats_out, rig_err_out, info, device, hip_stream);
} ISX_EXIT("isx_bundle_adjust_ray")

int isx_bundle_adjust_reproj(int num_images, const int* image_sizes_wh, const isx_mat* keypoints, int num_pairs, const int* pairs_from_to,
                             const isx_mat* matches, const isx_mat* inlier_masks, const isx_mat* counts, const isx_mat* stats, const isx_mat* conf,
                             int num_rigs, const int* rig_first, const isx_mat* est_rig_stats, const isx_mat* cameras_in, double conf_thresh,
                             int max_iter, double eps, int refine_flags, isx_mat* cameras_out, isx_mat* kr32_out, isx_mat* rig_stats_out,
                             isx_mat* rig_err_out, int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return ba_call<ReprojTr>(num_images, image_sizes_wh, keypoints, num_pairs, pairs_from_to, matches, inlier_masks, counts, stats, conf, num_rigs,
                             rig_first, est_rig_stats, cameras_in, conf_thresh, max_iter, eps, refine_flags, cameras_out, kr32_out, rig_stats_out,
                             rig_err_out, info, device, hip_stream);
} ISX_EXIT("isx_bundle_adjust_reproj")

int isx_wave_correct(int num_images, int num_rigs, const int* rig_first, const isx_mat* cameras_in, int kind, isx_mat* cameras_out, isx_mat* kr32_out,
                     isx_mat* rig_stats_out, int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return wv_call(num_images, num_rigs, rig_first, cameras_in, kind, cameras_out, kr32_out, rig_stats_out, info, device, hip_stream);
} ISX_EXIT("isx_wave_correct")

int isx_selftest_bundle_math(int fn, int n, const double* in, double* out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 0 && (n == 0 || (in && out)), ISX_ERR_INVALID, "selftest_bundle_math: n %d, or null in / out", n);
    ISX_CHECK_ARG(fn >= 0 && fn < BM_FNS, ISX_ERR_INVALID, "selftest_bundle_math: fn %d", fn);
    for (int i = 0; i < n; ++i) bm_selftest_item(fn, in + (size_t)bm_fn_in(fn) * i, out + (size_t)bm_fn_out(fn) * i);
    return ISX_OK;
} ISX_EXIT("isx_selftest_bundle_math")

int isx_selftest_bundle_math_device(int fn, int n, const double* in, double* out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 0 && (n == 0 || (in && out)), ISX_ERR_INVALID, "selftest_bundle_math_device: n %d, or null in / out", n);
    ISX_CHECK_ARG(fn >= 0 && fn < BM_FNS, ISX_ERR_INVALID, "selftest_bundle_math_device: fn %d", fn);
    if (n == 0) return ISX_OK;
    hipStream_t st = nullptr;
    const size_t in_bytes = (size_t)n * bm_fn_in(fn) * sizeof(double), out_bytes = (size_t)n * bm_fn_out(fn) * sizeof(double);
    DevBuf din, dout;
    ISX_TRY(din.reserve(in_bytes));
    ISX_TRY(dout.reserve(out_bytes));
    ISX_HIP(hipMemcpyAsync(din.p, in, in_bytes, hipMemcpyHostToDevice, st));
    ISX_LAUNCH("selftest_bundle_math", (double)(in_bytes + out_bytes), st, k_selftest_bundle_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fn, n,
               (const double*)din.p, (double*)dout.p);
    ISX_HIP(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));
    return ISX_OK;
} ISX_EXIT("isx_selftest_bundle_math_device")

}  // extern "C"
