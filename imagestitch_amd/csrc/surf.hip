// surf.hip — cv::detail::SurfFeaturesFinder (OpenCV 3.4.2: stitching/src/matchers.cpp on xfeatures2d/src/surf.cpp), the finder every main
// of the reference comments out, on gfx950:
//   isx_surf_find      SURF::detectAndCompute with extended = false, upright = false: 64 floats a keypoint
//   isx_surf_reserve   sizes the per-thread scratch ahead of a capture
//   isx_surf_release   returns it
//   isx_surf_default_params   host code
//
// The specification (DESIGN.md §8 "Features finder, SURF"; tests/helpers/surf_np.py, matched bit for bit; OpenCV parity is unpinned): every
// float operation is rounded on its own in the order the model writes it, the trigonometry is proj_math.hpp's, the two Gaussian tables are
// surf_tables.hpp's literals.
//
// The launches (their number depends on num_octaves alone):
//   k_surf_rows      gray and the row prefix sums of the integral image, a workgroup a row (uint32, wrapping)
//   k_surf_cols      the column prefix sums, a thread a column
//   k_surf_hessian   det and trace of every layer of one octave                                                  (num_octaves launches)
//   k_surf_maxima    <false> a workgroup takes 256 consecutive positions of the scan order (octave, layer, y, x), tests the 26 neighbours,
//                    runs interpolateKeypoint and counts what it accepts; <true> does the same again and writes each candidate at the
//                    prefix of the counts: the candidates lie in scan order whatever the scheduling
//   k_surf_prefix    one workgroup: the exclusive prefix of the workgroups' counts, the number of candidates, the overflow bit
//   k_surf_rank      every candidate counts the candidates before it in the total order (LDS tiles): order[rank] = candidate
//   k_surf_orient    a workgroup a ranked candidate: the 113 Haar samples, the 72 windows, the angle, or "removed"
//   k_surf_compact   one workgroup: the output row of every kept keypoint, the count and the status
//   k_surf_describe  a workgroup a keypoint, a work item a cell of the 21 x 21 patch walking its samples of the rotated window in the
//                    model's order; gradients and cell sums through LDS; one work item the double-precision norm
// No float atomics, no atomics at all; nothing read back on device mats.
#include "isx_device.hpp"
#include "block_scan.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"
#include "proj_math.hpp"
#include "surf_tables.hpp"

#include <cmath>

using namespace isx;
using namespace isxd;

namespace {

constexpr int SF_OCT = ISX_SURF_MAX_OCTAVES, SF_MID = ISX_SURF_MAX_LAYERS, SF_LAY = ISX_SURF_MAX_LAYERS + 2;
constexpr int SF_MAX = ISX_SURF_MAX_CANDIDATES;
constexpr int SF_ORI_NT = 256, SF_ORI_POINTS = 113, SF_ORI_WINDOWS = 72;
constexpr int SF_PATCH = 21, SF_CELLS = SF_PATCH * SF_PATCH, SF_DESC_NT = 448;
constexpr int SF_SCAN_NT = 1024;
static_assert(SF_MAX % SF_SCAN_NT == 0, "a thread of the compaction owns a whole stride of the candidates");
static_assert(SF_CELLS <= SF_DESC_NT, "a work item a patch cell");

struct SfBox { int x1, y1, x2, y2; float w; };

// one octave's layers as k_surf_hessian is told them, by value
struct SfOctave {
    int rows, cols, step, map_cols;
    int size[SF_LAY], present[SF_LAY];
    long long off[SF_LAY];                   // of the layer's maps, in floats
    SfBox dx[SF_LAY][3], dy[SF_LAY][3], dxy[SF_LAY][4];
};

// what the other kernels are told
struct SfPlan {
    int rows, cols, noct, nlay;
    float thresh;
    int size[SF_OCT][SF_LAY], present[SF_OCT][SF_LAY];
    long long off[SF_OCT][SF_LAY];
    int blk_off[SF_OCT * SF_MID + 1];        // the search workgroups of (o, l) are blk_off[o * nlay + l - 1] .. blk_off[o * nlay + l]
    int nblocks;
    long long map_floats;
};

// the search region of middle layer l of octave o
struct SfSearch { int ok, step, R, C, m, nr, nc; };
__host__ __device__ inline SfSearch sf_search(const SfPlan& P, int o, int l) {
    SfSearch s;
    s.step = 1 << o; s.R = P.rows >> o; s.C = P.cols >> o;
    s.m = (P.size[o][l + 1] / 2) / s.step + 1;
    s.nr = s.R - 2 * s.m; s.nc = s.C - 2 * s.m;
    s.ok = P.present[o][l - 1] && P.present[o][l] && P.present[o][l + 1] && s.nr > 0 && s.nc > 0;
    return s;
}

struct SfOut {
    float* kp; long long kp_step;
    float* meta; long long meta_step;
    float* desc; long long desc_step;
    int* count_status;
    int cap;
};

// calcHaarPattern: the box sums as signed 32-bit differences of the wrapping integral, each times its weight in float32, added in double
__device__ __forceinline__ float sf_haar(const unsigned* __restrict__ o, int SW, const SfBox* b, int n) {
    double d = 0.0;
    for (int k = 0; k < n; ++k) {
        const unsigned v = o[b[k].y1 * SW + b[k].x1] + o[b[k].y2 * SW + b[k].x2] - o[b[k].y2 * SW + b[k].x1] - o[b[k].y1 * SW + b[k].x2];
        const float p = (float)(int)v * b[k].w;
        d += (double)p;
    }
    return (float)d;
}

// resizeHaarPattern for one box
__host__ __device__ inline SfBox sf_resize_box(int x1, int y1, int x2, int y2, int w, float ratio) {
    SfBox b;
    b.x1 = (int)rintf(ratio * (float)x1); b.y1 = (int)rintf(ratio * (float)y1);
    b.x2 = (int)rintf(ratio * (float)x2); b.y2 = (int)rintf(ratio * (float)y2);
    b.w = (float)w / ((float)(b.x2 - b.x1) * (float)(b.y2 - b.y1));
    return b;
}

template <int CN>
__global__ __launch_bounds__(256) void k_surf_rows(const unsigned char* __restrict__ src, long long sstep, int W, int H, unsigned char* __restrict__ gray,
                                                   unsigned* __restrict__ S) {
    __shared__ unsigned s_tot[2][256 / WAVE];
    const int y = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE, SW = W + 1;
    unsigned* out = S + (long long)(y + 1) * SW;
    if (y == 0)
        for (int x = t; x < SW; x += 256) S[x] = 0u;
    if (t == 0) out[0] = 0u;
    unsigned carry = 0u;
    int flip = 0;
    for (int x0 = 0; x0 < W; x0 += 256, flip ^= 1) {
        const int x = x0 + t;
        unsigned v = 0u;
        if (x < W) {
            const unsigned char* p = src + (long long)y * sstep + (long long)x * CN;
            if constexpr (CN == 1) v = p[0];
            else v = (unsigned)(((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + 8192) >> 14);
            gray[(long long)y * W + x] = (unsigned char)v;
        }
        unsigned upto = v;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) { const unsigned n = __shfl_up(upto, o, WAVE); upto += lane >= o ? n : 0u; }
        if (lane == WAVE - 1) s_tot[flip][wv] = upto;
        __syncthreads();
        unsigned before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < 256 / WAVE; ++w) { const unsigned c = s_tot[flip][w]; before += w < wv ? c : 0u; all += c; }
        if (x < W) out[x + 1] = carry + before + upto;
        carry += all;
    }
}

__global__ __launch_bounds__(WAVE) void k_surf_cols(int W, int H, unsigned* __restrict__ S) {
    const int x = (int)(blockIdx.x * WAVE + threadIdx.x);
    if (x >= W) return;
    unsigned* p = S + (W + 1) + x + 1;
    unsigned acc = 0u;
    for (int y = 0; y < H; ++y, p += W + 1) { acc += *p; *p = acc; }
}

// calcLayerDetAndTrace for every layer of an octave: blockIdx.z = layer, 64 x 4 samples a workgroup
__global__ __launch_bounds__(256) void k_surf_hessian(SfOctave Q, const unsigned* __restrict__ S, float* __restrict__ det, float* __restrict__ trace) {
    const int l = (int)blockIdx.z;
    if (!Q.present[l]) return;
    const int size = Q.size[l];
    const int ni = 1 + (Q.rows - size) / Q.step, nj = 1 + (Q.cols - size) / Q.step, margin = (size / 2) / Q.step;
    const int j = (int)(blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1))), i = (int)(blockIdx.y * 4 + threadIdx.x / WAVE);
    if (i >= ni || j >= nj) return;
    const int SW = Q.cols + 1;
    const unsigned* o = S + (long long)(i * Q.step) * SW + j * Q.step;
    const float dx = sf_haar(o, SW, Q.dx[l], 3), dy = sf_haar(o, SW, Q.dy[l], 3), dxy = sf_haar(o, SW, Q.dxy[l], 4);
    const long long at = Q.off[l] + (long long)(i + margin) * Q.map_cols + (j + margin);
    det[at] = dx * dy - 0.81f * dxy * dxy;
    trace[at] = dx + dy;
}

// candidates: six rows of SF_MAX floats: pt.x, pt.y, size, response, octave, laplacian
template <bool WRITE>
__global__ __launch_bounds__(256) void k_surf_maxima(SfPlan P, const float* __restrict__ det, const float* __restrict__ trace, int* __restrict__ blk_count,
                                                     const int* __restrict__ blk_base, float* __restrict__ cand) {
    __shared__ int s_cnt[256 / WAVE];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    if (blk >= P.nblocks) return;
    int idx = 0;
    while (blk >= P.blk_off[idx + 1]) ++idx;
    const int o = idx / P.nlay, l = idx % P.nlay + 1;
    const SfSearch G = sf_search(P, o, l);
    const long long p = (long long)(blk - P.blk_off[idx]) * 256 + t;
    bool keep = false;
    float px = 0.f, py = 0.f, psize = 0.f, resp = 0.f, lap = 0.f;
    if (p < (long long)G.nr * G.nc) {
        const int i = (int)(p / G.nc) + G.m, j = (int)(p % G.nc) + G.m;
        const float* d1 = det + P.off[o][l] + (long long)i * G.C + j;
        const float v = d1[0];
        if (v > P.thresh) {
            const float* d0 = det + P.off[o][l - 1] + (long long)i * G.C + j;
            const float* d2 = det + P.off[o][l + 1] + (long long)i * G.C + j;
            float N0[9], N1[9], N2[9];
            bool top = true;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const int at = (a - 1) * G.C + (b - 1);
                    N0[a * 3 + b] = d0[at]; N1[a * 3 + b] = d1[at]; N2[a * 3 + b] = d2[at];
                    top = top && v > N0[a * 3 + b] && v > N2[a * 3 + b] && (a * 3 + b == 4 || v > N1[a * 3 + b]);
                }
            if (top) {
                const int size = P.size[o][l], ds = size - P.size[o][l - 1], half = (size / 2) / G.step;
                const float cx = (float)(G.step * (j - half)) + (float)(size - 1) * 0.5f, cy = (float)(G.step * (i - half)) + (float)(size - 1) * 0.5f;
                const float b0 = -(N1[5] - N1[3]) / 2.f, b1 = -(N1[7] - N1[1]) / 2.f, b2 = -(N2[4] - N0[4]) / 2.f;
                const float a01 = (N1[8] - N1[6] - N1[2] + N1[0]) / 4.f, a02 = (N2[5] - N2[3] - N0[5] + N0[3]) / 4.f, a12 = (N2[7] - N2[1] - N0[7] + N0[1]) / 4.f;
                const float a00 = N1[3] - 2.f * N1[4] + N1[5], a11 = N1[1] - 2.f * N1[4] + N1[7], a22 = N0[4] - 2.f * N1[4] + N2[4];
                float x0, x1, x2;
                if (fast_solve3(a00, a01, a02, a01, a11, a12, a02, a12, a22, b0, b1, b2, x0, x1, x2) && (x0 != 0.f || x1 != 0.f || x2 != 0.f) && fabsf(x0) <= 1.f &&
                    fabsf(x1) <= 1.f && fabsf(x2) <= 1.f) {
                    keep = true;
                    px = cx + x0 * (float)G.step; py = cy + x1 * (float)G.step;
                    psize = rintf((float)size + x2 * (float)ds);
                    resp = v;
                    const float tr = trace[P.off[o][l] + (long long)i * G.C + j];
                    lap = tr > 0.f ? 1.f : (tr < 0.f ? -1.f : 0.f);
                }
            }
        }
    }
    int total;
    const int before = block_count_before<256>(keep, s_cnt, total);
    if constexpr (!WRITE) {
        if (t == 0) blk_count[blk] = total;
    } else {
        const long long at = (long long)blk_base[blk] + before;
        if (keep && at < SF_MAX) {
            cand[at] = px; cand[SF_MAX + at] = py; cand[2 * SF_MAX + at] = psize; cand[3 * SF_MAX + at] = resp; cand[4 * SF_MAX + at] = (float)o;
            cand[5 * SF_MAX + at] = lap;
        }
    }
}

__global__ __launch_bounds__(SF_SCAN_NT) void k_surf_prefix(int n, const int* __restrict__ cnt, int* __restrict__ base, int* __restrict__ ncand_status) {
    __shared__ int s_tot[SF_SCAN_NT / WAVE];
    const int t = (int)threadIdx.x, chunk = (n + SF_SCAN_NT - 1) / SF_SCAN_NT;
    const long long lo = (long long)t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    long long mine = 0;
    for (long long i = lo; i < hi; ++i) mine += cnt[i];
    // (a count that passes 2^31 cannot occur: there are fewer search positions than ISX_SURF_MAX_PIXELS * 4 / 3 * 4 < 2^27)
    int total;
    int run = block_sum_before<SF_SCAN_NT>((int)mine, s_tot, total);
    for (long long i = lo; i < hi; ++i) { base[i] = run; run += cnt[i]; }
    if (t == 0) {
        ncand_status[0] = total < SF_MAX ? total : SF_MAX;
        ncand_status[1] = total > SF_MAX ? (int)ISX_SURF_CANDIDATES_DROPPED : 0;
    }
}

// rank of candidate i = the candidates before it: response, size, octave, pt.y, pt.x descending, then the scan index ascending
__global__ __launch_bounds__(256) void k_surf_rank(const float* __restrict__ cand, const int* __restrict__ ncand_status, int* __restrict__ order) {
    __shared__ float s_k[5][256];
    const int n = ncand_status[0], t = (int)threadIdx.x, i = (int)blockIdx.x * 256 + t;
    if ((int)blockIdx.x * 256 >= n) return;
    const bool live = i < n;
    const int ii = live ? i : 0;
    const float r = cand[3 * SF_MAX + ii], s = cand[2 * SF_MAX + ii], o = cand[4 * SF_MAX + ii], y = cand[SF_MAX + ii], x = cand[ii];
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        if (j0 + t < n) {
            s_k[0][t] = cand[3 * SF_MAX + j0 + t]; s_k[1][t] = cand[2 * SF_MAX + j0 + t]; s_k[2][t] = cand[4 * SF_MAX + j0 + t];
            s_k[3][t] = cand[SF_MAX + j0 + t]; s_k[4][t] = cand[j0 + t];
        }
        __syncthreads();
        const int m = n - j0 < 256 ? n - j0 : 256;
        for (int jj = 0; jj < m; ++jj) {
            const float rj = s_k[0][jj], sj = s_k[1][jj], oj = s_k[2][jj], yj = s_k[3][jj], xj = s_k[4][jj];
            const bool before = rj > r || (rj == r && (sj > s || (sj == s && (oj > o || (oj == o && (yj > y || (yj == y && (xj > x || (xj == x && j0 + jj < i)))))))));
            rank += before ? 1 : 0;
        }
    }
    if (live) order[rank] = i;
}

__device__ __forceinline__ float sf_atan2deg(float y, float x) {
    float a = isxpm::pm_atan2f(y, x) * (float)(180.0 / 3.14159265358979323846);
    if (a < 0.f) a = a + 360.f;
    if (a >= 360.f) a = a - 360.f;
    return a;
}

// the orientation of ranked candidate r = blockIdx.x: angle[r], valid[r]
__global__ __launch_bounds__(SF_ORI_NT) void k_surf_orient(int rows, int cols, const unsigned* __restrict__ S, const float* __restrict__ cand, const int* __restrict__ ncand_status,
                                                           const int* __restrict__ order, float* __restrict__ angle, int* __restrict__ valid) {
    __shared__ int s_cnt[SF_ORI_NT / WAVE], s_pi[SF_ORI_POINTS], s_pj[SF_ORI_POINTS], s_use[SF_ORI_POINTS], s_ang[SF_ORI_POINTS];
    __shared__ float s_X[SF_ORI_POINTS], s_Y[SF_ORI_POINTS], s_sx[SF_ORI_WINDOWS], s_sy[SF_ORI_WINDOWS];
    const int r = (int)blockIdx.x, t = (int)threadIdx.x;
    if (r >= ncand_status[0]) return;
    const int c = order[r];
    const float ptx = cand[c], pty = cand[SF_MAX + c], size = cand[2 * SF_MAX + c];
    const float s = size * 1.2f / 9.0f;
    const int g = 2 * cvround_x86(2.f * s);
    if (rows + 1 < g || cols + 1 < g) {
        if (t == 0) { valid[r] = 0; angle[r] = 0.f; }
        return;
    }
    // the disc's points in row-major order
    const int di = t / 13 - 6, dj = t % 13 - 6;
    const bool in_disc = t < 169 && di * di + dj * dj <= 36;
    int total;
    const int at = block_count_before<SF_ORI_NT>(in_disc, s_cnt, total);
    if (in_disc && at < SF_ORI_POINTS) { s_pi[at] = di; s_pj[at] = dj; }      // (the disc has exactly SF_ORI_POINTS points)
    __syncthreads();
    bool use = false;
    if (t < SF_ORI_POINTS) {
        const int i = s_pi[t], j = s_pj[t];
        const float half = (float)(g - 1) / 2.f;
        const int x = cvround_x86(ptx + (float)j * s - half), y = cvround_x86(pty + (float)i * s - half);
        use = y >= 0 && y < rows + 1 - g && x >= 0 && x < cols + 1 - g;
        float vx = 0.f, vy = 0.f;
        int ai = 0;
        if (use) {
            const float ratio = (float)g / 4.f;
            const SfBox bx[2] = {sf_resize_box(0, 0, 2, 4, -1, ratio), sf_resize_box(2, 0, 4, 4, 1, ratio)};
            const SfBox by[2] = {sf_resize_box(0, 0, 4, 2, 1, ratio), sf_resize_box(0, 2, 4, 4, -1, ratio)};
            const int SW = cols + 1;
            const unsigned* o = S + (long long)y * SW + x;
            const float w = isxsf::surf_g13(i + 6) * isxsf::surf_g13(j + 6);
            vx = sf_haar(o, SW, bx, 2) * w;
            vy = sf_haar(o, SW, by, 2) * w;
            ai = cvround_x86(sf_atan2deg(vy, vx));
        }
        s_use[t] = use ? 1 : 0; s_X[t] = vx; s_Y[t] = vy; s_ang[t] = ai;
    }
    const int nkept = __syncthreads_count(use);
    if (nkept == 0) {
        if (t == 0) { valid[r] = 0; angle[r] = 0.f; }
        return;
    }
    if (t < SF_ORI_WINDOWS) {
        const int a = 5 * t;
        float sx = 0.f, sy = 0.f;
        for (int k = 0; k < SF_ORI_POINTS; ++k) {
            const int d = abs(s_ang[k] - a);
            if (s_use[k] && (d < 30 || d > 330)) { sx += s_X[k]; sy += s_Y[k]; }
        }
        s_sx[t] = sx; s_sy[t] = sy;
    }
    __syncthreads();
    if (t == 0) {
        float best = 0.f, bx = 0.f, by = 0.f;
        for (int k = 0; k < SF_ORI_WINDOWS; ++k) {
            const float m = s_sx[k] * s_sx[k] + s_sy[k] * s_sy[k];
            if (m > best) { best = m; bx = s_sx[k]; by = s_sy[k]; }
        }
        angle[r] = sf_atan2deg(-by, bx);
        valid[r] = 1;
    }
}

// the output row of every ranked candidate (-1: removed), the count and the status
__global__ __launch_bounds__(SF_SCAN_NT) void k_surf_compact(const int* __restrict__ ncand_status, const int* __restrict__ valid, int* __restrict__ slot, SfOut O) {
    __shared__ int s_tot[SF_SCAN_NT / WAVE];
    const int n = ncand_status[0], t = (int)threadIdx.x, chunk = SF_MAX / SF_SCAN_NT;
    const int lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += valid[i];
    int total;
    int run = block_sum_before<SF_SCAN_NT>(mine, s_tot, total);
    for (int i = lo; i < hi; ++i) {
        const int v = valid[i];
        slot[i] = v ? run : -1;
        run += v;
    }
    if (t == 0) {
        O.count_status[0] = total < O.cap ? total : O.cap;
        O.count_status[1] = ncand_status[1] | (total > O.cap ? (int)ISX_SURF_TRUNCATED : 0);
    }
}

// computeResizeAreaTab's entries of destination cell d: sources first .. first + cnt - 1, the first weighs `head` if has_head, the last `tail`
// if has_tail, the others `mid`
struct SfSpan { int first, cnt, has_head, has_tail; float head, mid, tail; };
__device__ __forceinline__ SfSpan sf_span(int d, int ssize, double scale) {
    const double fsx1 = (double)d * scale, fsx2 = fsx1 + scale;
    const double rest = (double)ssize - fsx1, cell = scale < rest ? scale : rest;
    int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
    sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
    sx1 = sx1 < sx2 ? sx1 : sx2;
    SfSpan s;
    s.has_head = (double)sx1 - fsx1 > 1e-3;
    s.head = (float)(((double)sx1 - fsx1) / cell);
    s.mid = (float)(1.0 / cell);
    s.has_tail = fsx2 - (double)sx2 > 1e-3;
    double tl = fsx2 - (double)sx2;
    tl = tl < 1.0 ? tl : 1.0;
    tl = tl < cell ? tl : cell;
    s.tail = (float)(tl / cell);
    s.first = s.has_head ? sx1 - 1 : sx1;
    s.cnt = s.has_head + (sx2 - sx1) + s.has_tail;
    return s;
}
__device__ __forceinline__ float sf_weight(const SfSpan& s, int e) { return (s.has_head && e == 0) ? s.head : ((s.has_tail && e == s.cnt - 1) ? s.tail : s.mid); }

__global__ __launch_bounds__(SF_DESC_NT) void k_surf_describe(int rows, int cols, const unsigned char* __restrict__ gray, const float* __restrict__ cand,
                                                              const int* __restrict__ ncand_status, const int* __restrict__ order, const float* __restrict__ angle,
                                                              const int* __restrict__ slot, SfOut O) {
    __shared__ int s_P[SF_CELLS];
    __shared__ float s_dx[400], s_dy[400], s_vec[64], s_g20[20], s_scale;
    const int r = (int)blockIdx.x, t = (int)threadIdx.x;
    if (r >= ncand_status[0]) return;
    const int row = slot[r];
    if (row < 0 || row >= O.cap) return;
    const int c = order[r];
    const float ptx = cand[c], pty = cand[SF_MAX + c], size = cand[2 * SF_MAX + c], ang = angle[r];
    if (t < 20) s_g20[t] = isxsf::surf_g20(t);
    const float s = size * 1.2f / 9.0f;
    const int win = (int)(21.f * s);
    if (t < SF_CELLS) {
        float sn, cs;
        isxpm::pm_sincosf(ang * (float)(3.14159265358979323846 / 180.0), sn, cs);
        const float sin_dir = -sn, cos_dir = cs;
        const float off = -(float)(win - 1) / 2.f;
        float sx = ptx + off * cos_dir + off * sin_dir, sy = pty - off * sin_dir + off * cos_dir;
        const double scale = (double)win / (double)SF_PATCH;
        const SfSpan ys = sf_span(t / SF_PATCH, win, scale), xs = sf_span(t % SF_PATCH, win, scale);
        for (int i = 0; i < ys.first; ++i) { sx += sin_dir; sy += cos_dir; }
        const double dc = (double)cos_dir, dsn = (double)sin_dir;
        float acc = 0.f;
        for (int ey = 0; ey < ys.cnt; ++ey) {
            double px = (double)sx, py = (double)sy;
            for (int j = 0; j < xs.first; ++j) { px += dc; py -= dsn; }
            float buf = 0.f;
            for (int ex = 0; ex < xs.cnt; ++ex) {
                const int ix = (int)floor(px), iy = (int)floor(py);
                int v;
                if ((unsigned)ix < (unsigned)(cols - 1) && (unsigned)iy < (unsigned)(rows - 1)) {
                    const float a = (float)(px - (double)ix), b = (float)(py - (double)iy);
                    const unsigned char* q = gray + (long long)iy * cols + ix;
                    v = cvround_x86((float)q[0] * (1.f - a) * (1.f - b) + (float)q[1] * a * (1.f - b) + (float)q[cols] * (1.f - a) * b + (float)q[cols + 1] * a * b) & 255;
                } else {
                    int nx = __double2int_rn(px), ny = __double2int_rn(py);
                    nx = nx < 0 ? 0 : (nx > cols - 1 ? cols - 1 : nx);
                    ny = ny < 0 ? 0 : (ny > rows - 1 ? rows - 1 : ny);
                    v = gray[(long long)ny * cols + nx];
                }
                const float term = (float)v * sf_weight(xs, ex);
                buf = ex == 0 ? term : buf + term;
                px += dc; py -= dsn;
            }
            const float term = buf * sf_weight(ys, ey);
            acc = ey == 0 ? term : acc + term;
            sx += sin_dir; sy += cos_dir;
        }
        const int q = cvround_x86(acc);
        s_P[t] = q < 0 ? 0 : (q > 255 ? 255 : q);
    }
    __syncthreads();
    if (t < 400) {
        const int i = t / 20, j = t % 20;
        const float dw = s_g20[i] * s_g20[j];
        const int p00 = s_P[i * SF_PATCH + j], p01 = s_P[i * SF_PATCH + j + 1], p10 = s_P[(i + 1) * SF_PATCH + j], p11 = s_P[(i + 1) * SF_PATCH + j + 1];
        s_dx[t] = (float)(p01 - p00 + p11 - p10) * dw;
        s_dy[t] = (float)(p10 - p00 + p11 - p01) * dw;
    }
    __syncthreads();
    if (t < 64) {
        // work item t = cell (t / 16, t / 4 % 4), component t % 4: sum dx, sum dy, sum |dx|, sum |dy| in y, x order
        const int ci = t / 16, cj = (t / 4) % 4, k = t % 4;
        const float* src = (k & 1) ? s_dy : s_dx;
        float v = 0.f;
        for (int y = ci * 5; y < ci * 5 + 5; ++y)
            for (int x = cj * 5; x < cj * 5 + 5; ++x) {
                const float g = src[y * 20 + x];
                v += k >= 2 ? fabsf(g) : g;
            }
        s_vec[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double mag = 0.0;
        for (int k = 0; k < 64; ++k) { const float p = s_vec[k] * s_vec[k]; mag += (double)p; }
        s_scale = (float)(1.0 / (sqrt(mag) + (double)1.1920928955078125e-7f));
        float* kp = (float*)((char*)O.kp + (long long)row * O.kp_step);
        float* mt = (float*)((char*)O.meta + (long long)row * O.meta_step);
        kp[0] = ptx; kp[1] = pty;
        mt[0] = size; mt[1] = ang; mt[2] = cand[3 * SF_MAX + c]; mt[3] = cand[4 * SF_MAX + c]; mt[4] = cand[5 * SF_MAX + c];
    }
    __syncthreads();
    if (t < 64) ((float*)((char*)O.desc + (long long)row * O.desc_step))[t] = s_vec[t] * s_scale;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
void default_params(isx_surf_params& p) {
    p.hess_thresh = 300.0; p.num_octaves = 3; p.num_layers = 4; p.num_octaves_descr = 3; p.num_layers_descr = 4; p.extended = 0; p.upright = 0;
}

int check_params(const isx_surf_params* q, const char* who) {
    ISX_CHECK_ARG(q != nullptr, ISX_ERR_INVALID, "%s: null params", who);
    ISX_CHECK_ARG(q->hess_thresh >= 0.0 && q->hess_thresh <= 3.0e38, ISX_ERR_INVALID, "%s: hess_thresh %g is not in [0, 3e38]", who, q->hess_thresh);
    ISX_CHECK_ARG(q->num_octaves >= 1 && q->num_octaves <= ISX_SURF_MAX_OCTAVES, ISX_ERR_INVALID, "%s: num_octaves %d is not in [1, %d]", who, q->num_octaves,
                  ISX_SURF_MAX_OCTAVES);
    ISX_CHECK_ARG(q->num_layers >= 1 && q->num_layers <= ISX_SURF_MAX_LAYERS, ISX_ERR_INVALID, "%s: num_layers %d is not in [1, %d]", who, q->num_layers,
                  ISX_SURF_MAX_LAYERS);
    ISX_CHECK_ARG(q->num_octaves_descr == q->num_octaves && q->num_layers_descr == q->num_layers, ISX_ERR_UNSUPPORTED,
                  "%s: descriptor octaves / layers %d / %d differ from the detector's %d / %d (one detectAndCompute only)", who, q->num_octaves_descr,
                  q->num_layers_descr, q->num_octaves, q->num_layers);
    ISX_CHECK_ARG(q->extended == 0, ISX_ERR_UNSUPPORTED, "%s: extended descriptors (64 floats only)", who);
    ISX_CHECK_ARG(q->upright == 0, ISX_ERR_UNSUPPORTED, "%s: upright keypoints (oriented only)", who);
    return ISX_OK;
}

// the geometry of a W x H image under the parameters: which layers exist, where their maps lie, the search workgroups
int plan_image(const isx_surf_params& q, int W, int H, const char* who, SfPlan& P) {
    ISX_CHECK_ARG(W <= ISX_SURF_MAX_SIDE && H <= ISX_SURF_MAX_SIDE, ISX_ERR_UNSUPPORTED, "%s: an image of %d x %d (at most %d a side)", who, W, H, ISX_SURF_MAX_SIDE);
    ISX_CHECK_ARG((long long)W * H <= ISX_SURF_MAX_PIXELS, ISX_ERR_UNSUPPORTED, "%s: an image of %d x %d (at most %d pixels)", who, W, H, ISX_SURF_MAX_PIXELS);
    std::memset(&P, 0, sizeof(P));
    P.rows = H; P.cols = W; P.noct = q.num_octaves; P.nlay = q.num_layers; P.thresh = (float)q.hess_thresh;
    long long at = 0;
    for (int o = 0; o < P.noct; ++o)
        for (int l = 0; l < P.nlay + 2; ++l) {
            P.size[o][l] = (9 + 6 * l) << o;
            P.present[o][l] = P.size[o][l] <= H && P.size[o][l] <= W;
            P.off[o][l] = at;
            if (P.present[o][l]) at += (long long)(H >> o) * (W >> o);
        }
    P.map_floats = at;
    long long blocks = 0;
    for (int o = 0; o < P.noct; ++o)
        for (int l = 1; l <= P.nlay; ++l) {
            P.blk_off[o * P.nlay + l - 1] = (int)blocks;
            const SfSearch G = sf_search(P, o, l);
            if (G.ok) blocks += ((long long)G.nr * G.nc + 255) / 256;
        }
    P.blk_off[P.noct * P.nlay] = (int)blocks;
    for (int k = P.noct * P.nlay + 1; k <= SF_OCT * SF_MID; ++k) P.blk_off[k] = (int)blocks;
    P.nblocks = (int)blocks;
    return ISX_OK;
}

void plan_octave(const SfPlan& P, int o, SfOctave& Q) {
    static const int DX[3][5] = {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1}};
    static const int DY[3][5] = {{2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1}};
    static const int DXY[4][5] = {{1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}};
    std::memset(&Q, 0, sizeof(Q));
    Q.rows = P.rows; Q.cols = P.cols; Q.step = 1 << o; Q.map_cols = P.cols >> o;
    for (int l = 0; l < P.nlay + 2; ++l) {
        Q.size[l] = P.size[o][l]; Q.present[l] = P.present[o][l]; Q.off[l] = P.off[o][l];
        const float ratio = (float)Q.size[l] / 9.f;
        for (int k = 0; k < 3; ++k) {
            Q.dx[l][k] = sf_resize_box(DX[k][0], DX[k][1], DX[k][2], DX[k][3], DX[k][4], ratio);
            Q.dy[l][k] = sf_resize_box(DY[k][0], DY[k][1], DY[k][2], DY[k][3], DY[k][4], ratio);
        }
        for (int k = 0; k < 4; ++k) Q.dxy[l][k] = sf_resize_box(DXY[k][0], DXY[k][1], DXY[k][2], DXY[k][3], DXY[k][4], ratio);
    }
}

// one buffer: [staged host image] [gray] [integral] [det] [trace] [workgroup counts | bases] [ncand, status] [candidates] [order | angle | valid | slot]
// [staged host outputs]
struct SfLayout { size_t o_image, upload_bytes, o_gray, o_sum, o_det, o_trace, o_blk_count, o_blk_base, o_ncand, o_cand, o_order, o_angle, o_valid, o_slot; };
void lay_out(Bump& lay, const SfPlan& P, size_t image_bytes, SfLayout& o) {
    o.o_image = lay.take(image_bytes);
    o.upload_bytes = lay.at;
    o.o_gray = lay.take((size_t)P.rows * P.cols);
    o.o_sum = lay.take((size_t)(P.rows + 1) * (P.cols + 1) * 4);
    o.o_det = lay.take((size_t)P.map_floats * 4); o.o_trace = lay.take((size_t)P.map_floats * 4);
    const size_t blocks = (size_t)std::max(P.nblocks, 1);
    o.o_blk_count = lay.take(blocks * 4); o.o_blk_base = lay.take(blocks * 4);
    o.o_ncand = lay.take(8);
    o.o_cand = lay.take((size_t)6 * SF_MAX * 4);
    o.o_order = lay.take((size_t)SF_MAX * 4); o.o_angle = lay.take((size_t)SF_MAX * 4); o.o_valid = lay.take((size_t)SF_MAX * 4); o.o_slot = lay.take((size_t)SF_MAX * 4);
}

struct SfScratch : UploadScratch {};

}  // namespace

extern "C" {

int isx_surf_default_params(isx_surf_params* params) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(params != nullptr, ISX_ERR_INVALID, "surf_default_params: null params");
    default_params(*params);
    return ISX_OK;
} ISX_EXIT("isx_surf_default_params")

int isx_surf_release(void) ISX_ENTRY {
    clear_error();
    return per_thread<SfScratch>().release();
} ISX_EXIT("isx_surf_release")

int isx_surf_reserve(const isx_surf_params* params, int width, int height, int cap, int device) ISX_ENTRY {
    clear_error();
    const char* who = "surf_reserve";
    ISX_TRY(check_params(params, who));
    ISX_CHECK_ARG(width >= 1 && height >= 1, ISX_ERR_SIZE, "%s: an image of %d x %d", who, width, height);
    ISX_CHECK_ARG(cap >= 1, ISX_ERR_SIZE, "%s: outputs of %d rows", who, cap);
    SfPlan P;
    ISX_TRY(plan_image(*params, width, height, who, P));
    Bump lay;
    SfLayout o;
    lay_out(lay, P, 0, o);
    ISX_HIP(hipSetDevice(device));
    SfScratch& s = per_thread<SfScratch>();
    ISX_TRY(s.begin(device, nullptr, std::max(lay.at, s.work.cap), 0));
    return ISX_OK;
} ISX_EXIT("isx_surf_reserve")

int isx_surf_find(const isx_mat* image, const isx_surf_params* params, isx_mat* keypoints, isx_mat* meta, isx_mat* descriptors, isx_mat* count_status,
                  int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "surf_find";
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(image && keypoints && meta && descriptors && count_status, ISX_ERR_INVALID, "%s: null image, keypoints, meta, descriptors or count_status", who);
    ISX_TRY(check_params(params, who));
    ISX_CHECK_ARG(image->type == ISX_8UC1 || image->type == ISX_8UC3 || image->type == ISX_8UC4, ISX_ERR_TYPE, "%s: the image is %s (CV_8UC1, CV_8UC3 or CV_8UC4)", who,
                  type_name(image->type));
    ISX_CHECK_ARG(image->rows >= 1 && image->cols >= 1, ISX_ERR_SIZE, "%s: an image of %d x %d", who, image->cols, image->rows);
    const int cn = mat_cn(image->type), W = image->cols, H = image->rows;
    SfPlan P;
    ISX_TRY(plan_image(*params, W, H, who, P));
    ISX_CHECK_ARG(image->data != nullptr, ISX_ERR_INVALID, "%s: the image has a null data pointer", who);
    ISX_CHECK_ARG(image->step >= (size_t)W * cn || H == 1, ISX_ERR_INVALID, "%s: the image's step %zu is smaller than a row", who, image->step);
    ISX_CHECK_ARG(image->device < 0 || image->device == device, ISX_ERR_INVALID, "%s: the image lives on device %d, the call runs on %d", who, image->device, device);
    ISX_CHECK_ARG(keypoints->type == ISX_32FC1 && meta->type == ISX_32FC1 && descriptors->type == ISX_32FC1, ISX_ERR_TYPE,
                  "%s: keypoints, meta and descriptors are %s, %s and %s (CV_32FC1)", who, type_name(keypoints->type), type_name(meta->type), type_name(descriptors->type));
    const int cap = std::min(keypoints->rows, std::min(meta->rows, descriptors->rows));
    ISX_CHECK_ARG(cap >= 1, ISX_ERR_SIZE, "%s: keypoints, meta and descriptors have %d, %d and %d rows (at least 1 each)", who, keypoints->rows, meta->rows,
                  descriptors->rows);
    ISX_TRY(check_mat_holds(*keypoints, ISX_32FC1, cap, 2, 4, STOP_NO_ROW_WANTED, device, who, "keypoints", 0));
    ISX_TRY(check_mat_holds(*meta, ISX_32FC1, cap, 5, 4, STOP_NO_ROW_WANTED, device, who, "meta", 0));
    ISX_TRY(check_mat_holds(*descriptors, ISX_32FC1, cap, 64, 4, STOP_NO_ROW_WANTED, device, who, "descriptors", 0));
    ISX_TRY(check_mat_holds(*count_status, ISX_32SC1, 1, 2, 4, STOP_NO_ROW_WANTED, device, who, "count_status", 0));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    bool capturing = false;
    ISX_TRY(is_capturing(st, capturing));
    const bool any_host = image->device < 0 || keypoints->device < 0 || meta->device < 0 || descriptors->device < 0 || count_status->device < 0;
    ISX_CHECK_ARG(!capturing || !any_host, ISX_ERR_STATE, "%s: the stream is capturing and a mat is a host mat (staging it synchronises)", who);

    Bump lay;
    SfLayout o;
    const size_t image_bytes = image->device < 0 ? (size_t)H * W * cn : 0;
    lay_out(lay, P, image_bytes, o);
    StagedMat m_kp, m_meta, m_desc, m_cs;
    m_kp.plan(lay, *keypoints, cap, 8);
    m_meta.plan(lay, *meta, cap, 20);
    m_desc.plan(lay, *descriptors, cap, 256);
    m_cs.plan(lay, *count_status, 1, 8);

    SfScratch& s = per_thread<SfScratch>();
    if (capturing) {
        // nothing may be allocated, uploaded or fenced inside a capture: the scratch holds the call as it is, or the call is refused
        ISX_CHECK_ARG(s.device == device && s.work.p != nullptr && s.work.cap >= lay.at, ISX_ERR_STATE,
                      "%s: the stream is capturing and the scratch would have to grow (isx_surf_reserve first)", who);
    } else {
        ISX_TRY(s.begin(device, st, lay.at, o.upload_bytes));
        if (image->device < 0) {
            char* const pin = (char*)s.pin.p;
            for (int r = 0; r < H; ++r) std::memcpy(pin + o.o_image + (size_t)r * W * cn, (const char*)image->data + (size_t)r * image->step, (size_t)W * cn);
            ISX_TRY(s.upload(st, o.upload_bytes));
        }
    }
    char* const dev = (char*)s.work.p;

    const unsigned char* d_img = image->device < 0 ? (const unsigned char*)(dev + o.o_image) : (const unsigned char*)image->data;
    const long long img_step = image->device < 0 ? (long long)W * cn : (long long)image->step;
    unsigned char* const d_gray = (unsigned char*)(dev + o.o_gray);
    unsigned* const d_sum = (unsigned*)(dev + o.o_sum);
    float* const d_det = (float*)(dev + o.o_det);
    float* const d_trace = (float*)(dev + o.o_trace);
    int* const d_blk_count = (int*)(dev + o.o_blk_count);
    int* const d_blk_base = (int*)(dev + o.o_blk_base);
    int* const d_ncand = (int*)(dev + o.o_ncand);
    float* const d_cand = (float*)(dev + o.o_cand);
    int* const d_order = (int*)(dev + o.o_order);
    float* const d_angle = (float*)(dev + o.o_angle);
    int* const d_valid = (int*)(dev + o.o_valid);
    int* const d_slot = (int*)(dev + o.o_slot);
    SfOut O;
    m_kp.bind(dev, O.kp, O.kp_step);
    m_meta.bind(dev, O.meta, O.meta_step);
    m_desc.bind(dev, O.desc, O.desc_step);
    m_cs.bind(dev, O.count_status);
    O.cap = cap;

    // ---- the launches ----
    const double px = (double)W * H;
    if (cn == 1) ISX_LAUNCH("surf_rows", px * 6, st, k_surf_rows<1>, dim3(H), dim3(256), 0, d_img, img_step, W, H, d_gray, d_sum);
    else if (cn == 3) ISX_LAUNCH("surf_rows", px * 8, st, k_surf_rows<3>, dim3(H), dim3(256), 0, d_img, img_step, W, H, d_gray, d_sum);
    else ISX_LAUNCH("surf_rows", px * 9, st, k_surf_rows<4>, dim3(H), dim3(256), 0, d_img, img_step, W, H, d_gray, d_sum);
    ISX_LAUNCH("surf_cols", px * 8, st, k_surf_cols, dim3(cdiv(W, WAVE)), dim3(WAVE), 0, W, H, d_sum);
    for (int oc = 0; oc < P.noct; ++oc) {
        SfOctave Q;
        plan_octave(P, oc, Q);
        const int step = 1 << oc, s0 = P.size[oc][0];
        const int ni = P.present[oc][0] ? 1 + (H - s0) / step : 1, nj = P.present[oc][0] ? 1 + (W - s0) / step : 1;
        ISX_LAUNCH("surf_hessian", px * 8 * (P.nlay + 2) / (step * step), st, k_surf_hessian, dim3(cdiv(nj, WAVE), cdiv(ni, 4), P.nlay + 2), dim3(256), 0, Q,
                   (const unsigned*)d_sum, d_det, d_trace);
    }
    const dim3 search_grid(std::max(P.nblocks, 1));
    ISX_LAUNCH("surf_maxima_count", (double)P.nblocks * 1024, st, k_surf_maxima<false>, search_grid, dim3(256), 0, P, (const float*)d_det, (const float*)d_trace,
               d_blk_count, (const int*)d_blk_base, d_cand);
    ISX_LAUNCH("surf_prefix", (double)P.nblocks * 12, st, k_surf_prefix, dim3(1), dim3(SF_SCAN_NT), 0, P.nblocks, (const int*)d_blk_count, d_blk_base, d_ncand);
    ISX_LAUNCH("surf_maxima_write", (double)P.nblocks * 1024, st, k_surf_maxima<true>, search_grid, dim3(256), 0, P, (const float*)d_det, (const float*)d_trace,
               d_blk_count, (const int*)d_blk_base, d_cand);
    ISX_LAUNCH("surf_rank", (double)SF_MAX * 24, st, k_surf_rank, dim3(SF_MAX / 256), dim3(256), 0, (const float*)d_cand, (const int*)d_ncand, d_order);
    ISX_LAUNCH("surf_orient", (double)SF_MAX * SF_ORI_POINTS * 32, st, k_surf_orient, dim3(SF_MAX), dim3(SF_ORI_NT), 0, H, W, (const unsigned*)d_sum, (const float*)d_cand,
               (const int*)d_ncand, (const int*)d_order, d_angle, d_valid);
    ISX_LAUNCH("surf_compact", (double)SF_MAX * 8, st, k_surf_compact, dim3(1), dim3(SF_SCAN_NT), 0, (const int*)d_ncand, (const int*)d_valid, d_slot, O);
    ISX_LAUNCH("surf_describe", (double)cap * 4096, st, k_surf_describe, dim3(SF_MAX), dim3(SF_DESC_NT), 0, H, W, (const unsigned char*)d_gray, (const float*)d_cand,
               (const int*)d_ncand, (const int*)d_order, (const float*)d_angle, (const int*)d_slot, O);
    if (!capturing) ISX_TRY(s.ran(st));

    // ---- host outputs: the count first, then the rows it names ----
    if (m_kp.staged || m_meta.staged || m_desc.staged || m_cs.staged) {
        int cs[2] = {0, 0};
        ISX_TRY(counts_to_host(cs, O.count_status, 2, st));
        if (m_cs.staged) std::memcpy(count_status->data, cs, 8);
        ISX_TRY(m_kp.back(dev, cs[0], st));
        ISX_TRY(m_meta.back(dev, cs[0], st));
        ISX_TRY(m_desc.back(dev, cs[0], st));
        ISX_HIP(hipStreamSynchronize(st));
    }
    return ISX_OK;
} ISX_EXIT("isx_surf_find")

}  // extern "C"
