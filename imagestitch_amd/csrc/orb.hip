// orb.hip — the features finder of the F demo (the reference's 特征点检测/特征点检测/特征点检测.cpp) on gfx950:
//   isx_orb_find       OrbFeaturesFinder::find F:948-1017 = per grid cell detectAndCompute F:727-946 (computeKeyPoints F:56-191,
//                      HarrisResponses F:204-246, ICAngles F:250-283, computeOrbDescriptors F:287-353)
//   isx_orb_reserve    sizes the per-thread scratch and uploads the default pattern ahead of a capture
//   isx_orb_release    returns it
//   isx_orb_capacity, isx_orb_default_params, isx_orb_default_pattern   host code
//
// The specification (DESIGN.md §8 "Features finder"; tests/helpers/orb_np.py, matched bit for bit): what F writes is followed operation for
// operation; FAST, the blur, cv::RNG and the trigonometry are restated; the pyramid is resize.hip's INTER_LINEAR (resize_taps.hpp); no
// border is built, because no reader leaves its layer.
//
// Every launch covers all cells and levels of the image (blockIdx.z or blockIdx.y is the layer = cell * nlevels + level), so the launch
// count depends on nlevels alone:
//   k_orb_gray       the gray image (level 0 of a cell is a window of it); it also clears the histograms and the status word
//   k_orb_resize     level l of every cell from its level l - 1                                                    (nlevels - 1 launches)
//   k_orb_fast       the FAST-9/16 score map (0: no corner)
//   k_orb_nms        scores that beat their 8 neighbours, inside runByImageBorder(31), and their 256-bin histogram per layer (int atomics)
//   k_orb_first_cut  one workgroup per layer: the cut score from the histogram, then the kept map in row-major order, 8 pixels a thread,
//                    compacted by prefix counts: the candidates come out in canonical order whatever the scheduling
//   k_orb_harris     a thread per candidate
//   k_orb_final_cut  one workgroup per layer: every candidate counts the responses above it and the equal ones before it (LDS), then the
//                    same ordered compaction
//   k_orb_blur       7 x 7, sigma 2 in Q8 integers
//   k_orb_describe   a wave per keypoint: the moments by a wave reduction, the angle, 8 pattern points per lane, and the output rows at
//                    the prefix sum of the layers' counts; block (0, 0) writes count and status
// No float atomics, nothing read back on device mats.  The plan (geometry, per-level counts and offsets) travels in the kernel arguments:
// nothing is uploaded but the pattern, so a call on device mats can be captured once the scratch is reserved.
#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"
#include "resize_taps.hpp"
#include "proj_math.hpp"

#include <cmath>

using namespace isx;
using namespace isxd;

namespace {

constexpr int OB_LEVELS = ISX_ORB_MAX_LEVELS;
constexpr int OB_EDGE = 31, OB_PATCH = 31, OB_HALF = 15, OB_HARRIS = 7;
constexpr int OB_PATTERN_POINTS = 512, OB_PATTERN_BYTES = OB_PATTERN_POINTS * 2 * 4;
constexpr int OB_CUT_NT = 1024;              // threads of the two cut kernels
constexpr int OB_CUT_PX = 8;                 // pixels a thread of the first cut takes per step
static_assert(OB_CUT_NT * OB_CUT_PX < (1 << 16), "the two counts of a step share a word");
constexpr int OB_DESC_NT = 256;              // k_orb_describe: 4 waves, a keypoint each
static_assert(ISX_ORB_MAX_CANDIDATES % OB_CUT_NT == 0, "a thread of the final cut owns whole strides of the candidates");

// What every kernel is told, by value.  A pyramid is W * H bytes of level 0 (the cells are windows of it) and, per level l >= 1, one slot of
// pitch[l] x slot_rows[l] bytes per cell.  Cell sizes take two values a direction (cw0 or cw0 + 1 columns), so do the layers'.
struct OrbPlan {
    int W, H, gx, gy, nlevels, fast_threshold;
    int cw0, ch0;                            // the smaller cell width and height
    int lw[OB_LEVELS][2], lh[OB_LEVELS][2];  // layer size for a cell of cw0 (+ 1) columns, ch0 (+ 1) rows
    int pitch[OB_LEVELS];
    long long lvl_off[OB_LEVELS], slot[OB_LEVELS];
    float scale[OB_LEVELS], inv_scale[OB_LEVELS];
    int n[OB_LEVELS];                        // F:72-82
    int cand_cap[OB_LEVELS], cand_off[OB_LEVELS], cand_sum;      // per cell: level l's candidates start at cand_off[l]; cand_sum in all
    int keep_cap[OB_LEVELS], keep_off[OB_LEVELS], keep_sum;
    int umax[OB_HALF + 1];                   // F:88-103
    float harris_scale;                      // scale_sq_sq of F:216-217
};
struct OrbLayer { int w, h, pitch, xl, yl; long long off; };

__host__ __device__ inline OrbLayer orb_layer(const OrbPlan& P, int cell, int l) {
    const int c = cell % P.gx, r = cell / P.gx;
    const int xl = c * P.W / P.gx, xr = (c + 1) * P.W / P.gx, yl = r * P.H / P.gy, yr = (r + 1) * P.H / P.gy;      // F:984-987
    OrbLayer L;
    L.xl = xl; L.yl = yl;
    if (l == 0) { L.w = xr - xl; L.h = yr - yl; L.pitch = P.W; L.off = (long long)yl * P.W + xl; }
    else {
        L.w = P.lw[l][(xr - xl) - P.cw0]; L.h = P.lh[l][(yr - yl) - P.ch0];
        L.pitch = P.pitch[l]; L.off = P.lvl_off[l] + (long long)cell * P.slot[l];
    }
    if (L.w <= 0 || L.h <= 0) L.w = L.h = 0;
    return L;
}

struct OrbOut {
    float* kp; long long kp_step;
    float* meta; long long meta_step;
    unsigned char* desc; long long desc_step;
    int* count_status;
};

template <int CN>
__global__ __launch_bounds__(256) void k_orb_gray(const unsigned char* __restrict__ src, long long sstep, int W, int H, unsigned char* __restrict__ gray,
                                                  int* __restrict__ zero, int zero_words) {
    const int x = (int)(blockIdx.x * 256 + threadIdx.x), y = (int)blockIdx.y;
    // the histograms and the status word start every call at zero (no memset: the call is nothing but its kernels)
    const long long nthreads = (long long)gridDim.x * gridDim.y * 256;
    for (long long i = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < zero_words; i += nthreads) zero[i] = 0;
    if (x >= W) return;
    const unsigned char* p = src + (long long)y * sstep + (long long)x * CN;
    int v;
    if constexpr (CN == 1) v = p[0];
    else v = ((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + 8192) >> 14;
    gray[(long long)y * W + x] = (unsigned char)v;
}

// level l of every cell from its level l - 1: resize.hip's INTER_LINEAR on CV_8U, the 2 x 2 area rule where both sides halve
__global__ __launch_bounds__(256) void k_orb_resize(OrbPlan P, int l, unsigned char* __restrict__ pyr) {
    const int cell = (int)blockIdx.z;
    const OrbLayer S = orb_layer(P, cell, l - 1), D = orb_layer(P, cell, l);
    const int x = (int)(blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1))), y = (int)(blockIdx.y * 4 + threadIdx.x / WAVE);
    if (x >= D.w || y >= D.h || S.w <= 0) return;
    const unsigned char* s = pyr + S.off;
    int v;
    if (S.w == 2 * D.w && S.h == 2 * D.h) {
        const unsigned char* r0 = s + (long long)(2 * y) * S.pitch + 2 * x;
        v = ((int)r0[0] + (int)r0[1] + (int)r0[S.pitch] + (int)r0[S.pitch + 1] + 2) >> 2;
    } else {
        const double scale_x = 1.0 / ((double)D.w / S.w), scale_y = 1.0 / ((double)D.h / S.h);      // resize_scale
        const ColTap ct = col_tap(x, scale_x, S.w);
        const RowTap rt = row_tap(y, scale_y, S.h);
        const int sx1 = min(ct.sx + 1, S.w - 1);
        const int a0 = resize_coef(1.f - ct.a1), a1 = resize_coef(ct.a1), b0 = resize_coef(1.f - rt.fy), b1 = resize_coef(rt.fy);
        const unsigned char* r0 = s + (long long)rt.sy0 * S.pitch;
        const unsigned char* r1 = s + (long long)rt.sy1 * S.pitch;
        v = resize_vert_u8((int)r0[ct.sx] * a0 + (int)r0[sx1] * a1, (int)r1[ct.sx] * a0 + (int)r1[sx1] * a1, b0, b1);
    }
    pyr[D.off + (long long)y * D.pitch + x] = (unsigned char)v;
}

// the layer, pixel and row pointer of a thread of the per-pixel kernels: 64 x 4 pixels a block, blockIdx.z = layer
#define OB_PIXEL_THREAD()                                                                                                         \
    const int layer = (int)blockIdx.z;                                                                                            \
    const OrbLayer L = orb_layer(P, layer / P.nlevels, layer % P.nlevels);                                                        \
    const int x = (int)(blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1))), y = (int)(blockIdx.y * 4 + threadIdx.x / WAVE);          \
    if (x >= L.w || y >= L.h) return

// FAST-9/16: d_k = I(p + o_k) - I(p); a = max over the 16 arcs of 9 of min d, b = min over the arcs of max d; score = max(a, -b) - 1
__global__ __launch_bounds__(256) void k_orb_fast(OrbPlan P, const unsigned char* __restrict__ pyr, unsigned char* __restrict__ score) {
    OB_PIXEL_THREAD();
    int out = 0;
    if (x >= 3 && y >= 3 && x < L.w - 3 && y < L.h - 3) {
        const unsigned char* c = pyr + L.off + (long long)y * L.pitch + x;
        const int p = L.pitch, v = c[0];
        const int o[16] = {3 * p, 3 * p + 1, 2 * p + 2, p + 3, 3, -p + 3, -2 * p + 2, -3 * p + 1, -3 * p, -3 * p - 1, -2 * p - 2, -p - 3, -3, p - 3, 2 * p - 2, 3 * p - 1};
        int d[16], lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) d[k] = (int)c[o[k]] - v;
#pragma unroll
        for (int k = 0; k < 16; ++k) { lo2[k] = min(d[k], d[(k + 1) & 15]); hi2[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
        for (int k = 0; k < 16; ++k) { lo4[k] = min(lo2[k], lo2[(k + 2) & 15]); hi4[k] = max(hi2[k], hi2[(k + 2) & 15]); }
        int a = INT_MIN, b = INT_MAX;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            a = max(a, min(min(lo4[k], lo4[(k + 4) & 15]), d[(k + 8) & 15]));
            b = min(b, max(max(hi4[k], hi4[(k + 4) & 15]), d[(k + 8) & 15]));
        }
        const int s = max(a, -b) - 1;
        out = s >= P.fast_threshold ? s : 0;
    }
    score[L.off + (long long)y * L.pitch + x] = (unsigned char)out;
}

// a corner stays where its score is strictly greater than its 8 neighbours' (F:118: nonmaxSuppression = true) and it lies inside
// runByImageBorder(31) (F:123); the histogram of the scores that stay feeds the first cut
__global__ __launch_bounds__(256) void k_orb_nms(OrbPlan P, const unsigned char* __restrict__ score, unsigned char* __restrict__ kept, int* __restrict__ hist) {
    OB_PIXEL_THREAD();
    if (x < OB_EDGE || y < OB_EDGE || x >= L.w - OB_EDGE || y >= L.h - OB_EDGE) return;
    const unsigned char* c = score + L.off + (long long)y * L.pitch + x;
    const int p = L.pitch, s = c[0];
    const int m = max(max(max((int)c[-p - 1], (int)c[-p]), max((int)c[-p + 1], (int)c[-1])), max(max((int)c[1], (int)c[p - 1]), max((int)c[p], (int)c[p + 1])));
    const int out = s > m ? s : 0;           // (s > m >= 0: a corner)
    kept[L.off + (long long)y * L.pitch + x] = (unsigned char)out;
    if (out) atomicAdd(hist + layer * 256 + out, 1);
}

// The exclusive count of `flag` over the block's threads in thread order, and the block's total: ballot inside a wave, the waves' counts
// through LDS.  `cnt` is this call's own LDS row (the caller alternates two, so one barrier a call is enough).
template <int NT>
__device__ __forceinline__ int block_count_before(bool flag, int* cnt, int& total) {
    const int lane = (int)(threadIdx.x & (WAVE - 1)), wv = (int)(threadIdx.x / WAVE);
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) cnt[wv] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int i = 0; i < NT / WAVE; ++i) { const int c = cnt[i]; before += i < wv ? c : 0; total += c; }
    return before;
}

// retainBest(2 n_l) by FAST score (F:126) with the capacity rule.  above[s] = kept points with a score > s.  The cut T is the smallest score
// with above[T] < 2 n: every point above T is kept, the points at T are the ties: the first `room` = cand_cap - above[T] of them in
// row-major order.  A kept point's row is the number of kept points before it.
__global__ __launch_bounds__(OB_CUT_NT) void k_orb_first_cut(OrbPlan P, const unsigned char* __restrict__ kept, const int* __restrict__ hist, int* __restrict__ cand_xy,
                                                             int* __restrict__ cand_count, int* __restrict__ status) {
    __shared__ int s_hist[256], s_above[256], s_cnt[2][OB_CUT_NT / WAVE], s_cut;
    const int layer = (int)blockIdx.x, cell = layer / P.nlevels, l = layer % P.nlevels, t = (int)threadIdx.x;
    const OrbLayer L = orb_layer(P, cell, l);
    if (t < 256) s_hist[t] = hist[layer * 256 + t];
    __syncthreads();
    if (t < 256) {
        int a = 0;
        for (int s = t + 1; s < 256; ++s) a += s_hist[s];
        s_above[t] = a;
    }
    __syncthreads();
    const int want = 2 * P.n[l];
    if (t == 0) {
        int T = 256;                         // 256: nothing is kept (n_l == 0)
        for (int s = 255; s >= 1 && s_above[s] < want; --s) T = s;
        s_cut = T;
    }
    __syncthreads();
    const int T = s_cut;
    const int room = T < 256 ? P.cand_cap[l] - s_above[T] : 0;
    const int rw = L.w - 2 * OB_EDGE, rh = L.h - 2 * OB_EDGE;
    const int total = rw > 0 && rh > 0 ? rw * rh : 0;
    const unsigned char* img = kept + L.off;
    int* out = cand_xy + (long long)cell * P.cand_sum + P.cand_off[l];
    // a thread owns OB_CUT_PX consecutive pixels of the region's row-major order and counts its points above the cut and at it; the
    // two counts ride in one word (a step holds 8192 pixels) through a shuffle scan inside the wave and the waves' totals in LDS
    const int lane = t & (WAVE - 1), wv = t / WAVE;
    int above_before = 0, ties_before = 0, flip = 0;
    for (int i0 = 0; i0 < total; i0 += OB_CUT_NT * OB_CUT_PX, flip ^= 1) {
        const int i = i0 + t * OB_CUT_PX;
        int py = 0, px = 0;
        if (i < total) { py = i / rw; px = i - py * rw; }
        int sc[OB_CUT_PX];
        unsigned mine = 0;
        {
            int qx = px, qy = py;
#pragma unroll
            for (int k = 0; k < OB_CUT_PX; ++k) {
                int s = 0;
                if (i + k < total) {
                    s = img[(long long)(qy + OB_EDGE) * L.pitch + (qx + OB_EDGE)];
                    if (++qx == rw) { qx = 0; ++qy; }
                }
                sc[k] = s;
                mine += (s > T ? 1u : 0u) + (s == T ? 0x10000u : 0u);
            }
        }
        unsigned upto = mine;                // inclusive over the wave's lanes
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) { const unsigned v = __shfl_up(upto, o, WAVE); upto += lane >= o ? v : 0u; }
        if (lane == WAVE - 1) s_cnt[flip][wv] = (int)upto;
        __syncthreads();
        unsigned before = upto - mine, all = 0;
#pragma unroll
        for (int w = 0; w < OB_CUT_NT / WAVE; ++w) { const unsigned c = (unsigned)s_cnt[flip][w]; before += w < wv ? c : 0u; all += c; }
        int ab = above_before + (int)(before & 0xFFFFu), tb = ties_before + (int)(before >> 16);
        int qx = px, qy = py;
#pragma unroll
        for (int k = 0; k < OB_CUT_PX; ++k) {
            if (i + k >= total) break;
            const int s = sc[k], xy = ((qy + OB_EDGE) << 16) | (qx + OB_EDGE);
            if (s > T) { out[ab + min(tb, room)] = xy; ++ab; }
            else if (s == T) { if (tb < room) out[ab + tb] = xy; ++tb; }
            if (++qx == rw) { qx = 0; ++qy; }
        }
        above_before += (int)(all & 0xFFFFu); ties_before += (int)(all >> 16);
    }
    if (t == 0) {
        cand_count[layer] = above_before + min(ties_before, room);
        if (ties_before > room) atomicOr(status, (int)ISX_ORB_TRUNCATED);
    }
}

// HarrisResponses (F:204-246), blockSize 7: int sums, then F:243-244's float expression in its written order
__global__ __launch_bounds__(256) void k_orb_harris(OrbPlan P, const unsigned char* __restrict__ pyr, const int* __restrict__ cand_xy, const int* __restrict__ cand_count,
                                                    float* __restrict__ cand_resp) {
    const int layer = (int)blockIdx.y, cell = layer / P.nlevels, l = layer % P.nlevels;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= cand_count[layer]) return;
    const OrbLayer L = orb_layer(P, cell, l);
    const long long at = (long long)cell * P.cand_sum + P.cand_off[l] + i;
    const int xy = cand_xy[at], x0 = xy & 0xFFFF, y0 = xy >> 16, p = L.pitch;
    const unsigned char* c0 = pyr + L.off + (long long)(y0 - OB_HARRIS / 2) * p + (x0 - OB_HARRIS / 2);
    int a = 0, b = 0, c = 0;
    for (int i2 = 0; i2 < OB_HARRIS; ++i2)
#pragma unroll
        for (int j = 0; j < OB_HARRIS; ++j) {
            const unsigned char* q = c0 + i2 * p + j;
            const int Ix = ((int)q[1] - (int)q[-1]) * 2 + ((int)q[-p + 1] - (int)q[-p - 1]) + ((int)q[p + 1] - (int)q[p - 1]);
            const int Iy = ((int)q[p] - (int)q[-p]) * 2 + ((int)q[p - 1] - (int)q[-p - 1]) + ((int)q[p + 1] - (int)q[-p + 1]);
            a += Ix * Ix; b += Iy * Iy; c += Ix * Iy;
        }
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    cand_resp[at] = (fa * fb - fc * fc - 0.04f * (fa + fb) * (fa + fb)) * P.harris_scale;
}

// retainBest(n_l) by Harris response (F:172) with the capacity rule: candidate i is wanted when fewer than n responses are greater, and kept
// when the greater ones and the equal ones before it leave it a row (greater + equal_before < keep_cap).  Kept points stay in canonical order.
__global__ __launch_bounds__(OB_CUT_NT) void k_orb_final_cut(OrbPlan P, const int* __restrict__ cand_xy, const float* __restrict__ cand_resp, const int* __restrict__ cand_count,
                                                             int* __restrict__ keep_xy, float* __restrict__ keep_resp, int* __restrict__ keep_count, int* __restrict__ status) {
    __shared__ float s_resp[ISX_ORB_MAX_CANDIDATES];
    __shared__ int s_cnt[2][OB_CUT_NT / WAVE], s_dropped;
    const int layer = (int)blockIdx.x, cell = layer / P.nlevels, l = layer % P.nlevels, t = (int)threadIdx.x;
    const int m = cand_count[layer], n = P.n[l], cap = P.keep_cap[l];
    const long long cbase = (long long)cell * P.cand_sum + P.cand_off[l], kbase = (long long)cell * P.keep_sum + P.keep_off[l];
    if (t == 0) s_dropped = 0;
    for (int i = t; i < m; i += OB_CUT_NT) s_resp[i] = cand_resp[cbase + i];
    __syncthreads();
    int base = 0, flip = 0;
    bool dropped = false;
    for (int i0 = 0; i0 < m; i0 += OB_CUT_NT, flip ^= 1) {
        const int i = i0 + t;
        bool keep = false;
        if (i < m) {
            const float r = s_resp[i];
            int greater = 0, equal_before = 0;
            for (int j = 0; j < m; ++j) {
                const float q = s_resp[j];
                greater += q > r;
                equal_before += (q == r) & (j < i);
            }
            const bool wanted = greater < n;
            keep = wanted && greater + equal_before < cap;
            dropped |= wanted && !keep;
        }
        int total;
        const int pos = base + block_count_before<OB_CUT_NT>(keep, s_cnt[flip], total);
        if (keep) { keep_xy[kbase + pos] = cand_xy[cbase + i]; keep_resp[kbase + pos] = s_resp[i]; }
        base += total;
    }
    if (dropped) s_dropped = 1;
    __syncthreads();
    if (t == 0) {
        keep_count[layer] = base;
        if (s_dropped) atomicOr(status, (int)ISX_ORB_TRUNCATED);
    }
}

// GaussianBlur(7 x 7, sigma 2) (F:936) in exact integers where the window lies inside the layer; the 3-px rim is never read
__global__ __launch_bounds__(256) void k_orb_blur(OrbPlan P, const unsigned char* __restrict__ pyr, unsigned char* __restrict__ blurred) {
    OB_PIXEL_THREAD();
    if (x < 3 || y < 3 || x >= L.w - 3 || y >= L.h - 3) return;
    const unsigned char* c = pyr + L.off + (long long)(y - 3) * L.pitch + (x - 3);
    const int OB_BLUR[7] = {18, 34, 49, 54, 49, 34, 18};      // getGaussianKernel(7, 2) in Q8, the residual in the centre tap
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const unsigned char* r = c + i * L.pitch;
        int h = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) h += OB_BLUR[j] * (int)r[j];
        acc += OB_BLUR[i] * h;
    }
    blurred[L.off + (long long)y * L.pitch + x] = (unsigned char)((acc + (1 << 15)) >> 16);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// ICAngles (F:250-283), pt *= scale (F:189), computeOrbDescriptors (F:287-353) and the output rows.  blockIdx.y = layer, a wave per keypoint.
__global__ __launch_bounds__(OB_DESC_NT) void k_orb_describe(OrbPlan P, const unsigned char* __restrict__ pyr, const unsigned char* __restrict__ blurred,
                                                             const unsigned char* __restrict__ pattern, long long pattern_step, const int* __restrict__ keep_xy,
                                                             const float* __restrict__ keep_resp, const int* __restrict__ keep_count, const int* __restrict__ status, OrbOut O) {
    __shared__ int s_pat[2 * OB_PATTERN_POINTS], s_sum[2][OB_DESC_NT / WAVE];
    const int layer = (int)blockIdx.y, cell = layer / P.nlevels, l = layer % P.nlevels, nlayers = P.gx * P.gy * P.nlevels;
    const int t = (int)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    bool bad = false;
    for (int i = t; i < OB_PATTERN_POINTS; i += OB_DESC_NT) {
        const int* row = (const int*)(pattern + (long long)i * pattern_step);
        const int px = row[0], py = row[1];
        bad |= px < -OB_HALF || px > OB_HALF || py < -OB_HALF || py > OB_HALF;
        s_pat[2 * i] = px; s_pat[2 * i + 1] = py;
    }
    int before = 0, all = 0;                  // keypoints of the layers before this one, and of all
    for (int i = t; i < nlayers; i += OB_DESC_NT) { const int c = keep_count[i]; all += c; before += i < layer ? c : 0; }
    before = wave_sum(before); all = wave_sum(all);
    if (lane == 0) { s_sum[0][wv] = before; s_sum[1][wv] = all; }
    bad = __syncthreads_or(bad);
    before = all = 0;
#pragma unroll
    for (int i = 0; i < OB_DESC_NT / WAVE; ++i) { before += s_sum[0][i]; all += s_sum[1][i]; }
    if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
        O.count_status[0] = bad ? 0 : all;
        O.count_status[1] = *status | (bad ? (int)ISX_ORB_BAD_PATTERN : 0);
    }
    const int k = (int)blockIdx.x * (OB_DESC_NT / WAVE) + wv;
    if (bad || k >= keep_count[layer]) return;
    const OrbLayer L = orb_layer(P, cell, l);
    const long long kat = (long long)cell * P.keep_sum + P.keep_off[l] + k;
    const int xy = keep_xy[kat], x = xy & 0xFFFF, y = xy >> 16, p = L.pitch;
    // the moments: lanes 0 - 31 take row y + v, lanes 32 - 63 row y - v, u = (lane & 31) - 15 inside umax[v]
    const unsigned char* c = pyr + L.off + (long long)y * p + x;
    const int u = (lane & 31) - OB_HALF, up = lane < 32;
    int m01 = 0, m10 = 0;
    for (int v = 0; v <= OB_HALF; ++v) {
        const int d = P.umax[v];
        if (u >= -d && u <= d && (v > 0 || up)) {
            const int val = c[(up ? v : -v) * p + u];
            m10 += u * val;
            m01 += (up ? v : -v) * val;
        }
    }
    m01 = wave_sum(m01); m10 = wave_sum(m10);
    float angle = isxpm::pm_atan2f((float)m01, (float)m10) * (float)(180.0 / 3.14159265358979323846);
    if (angle < 0.f) angle = angle + 360.f;
    if (angle >= 360.f) angle = angle - 360.f;
    const float scale = P.scale[l], inv = P.inv_scale[l];
    const float ptx = (float)x * scale, pty = (float)y * scale;
    const int cx = cvround_x86(ptx * inv), cy = cvround_x86(pty * inv);                       // F:305-306
    float b, a;
    isxpm::pm_sincosf(angle * (float)(3.14159265358979323846 / 180.0), b, a);                 // F:302-303
    const unsigned char* bc = blurred + L.off + (long long)cy * p + cx;
    int nib = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int tv[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = 8 * lane + 2 * j + e;
            const float fx = (float)s_pat[2 * idx], fy = (float)s_pat[2 * idx + 1];
            const int ix = cvround_x86(fx * a - fy * b), iy = cvround_x86(fx * b + fy * a);   // GET_VALUE, F:313-318
            tv[e] = bc[iy * p + ix];
        }
        nib |= (tv[0] < tv[1]) << j;
    }
    const int other = __shfl_xor(nib, 1, WAVE);
    const long long row = (long long)before + k;
    if ((lane & 1) == 0) O.desc[row * O.desc_step + (lane >> 1)] = (unsigned char)(nib | (other << 4));
    if (lane == 0) {
        float* kp = (float*)((char*)O.kp + row * O.kp_step);
        float* mt = (float*)((char*)O.meta + row * O.meta_step);
        kp[0] = ptx + (float)L.xl; kp[1] = pty + (float)L.yl;                                 // F:1006-1007
        mt[0] = (float)OB_PATCH * scale; mt[1] = angle; mt[2] = keep_resp[kat]; mt[3] = (float)l;      // F:135, F:281, F:243, F:134
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
int cv_round(float v) { return (int)std::rint(v); }

void default_params(isx_orb_params& p) {
    p.grid_width = 3; p.grid_height = 1; p.n_features = 1500; p.scale_factor = 1.3f; p.nlevels = 5; p.edge_threshold = OB_EDGE; p.first_level = 0; p.wta_k = 2;
    p.score_type = ISX_ORB_HARRIS_SCORE; p.patch_size = OB_PATCH; p.fast_threshold = 20;
}

// F:72-82
void features_per_level(int nfeatures, double scale_factor, int nlevels, int* n) {
    const float factor = (float)(1.0 / scale_factor);
    float wanted = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        n[l] = cv_round(wanted);
        sum += n[l];
        wanted *= factor;
    }
    n[nlevels - 1] = std::max(nfeatures - sum, 0);
}

// the checks of the parameters, and what follows from them alone
int plan_params(const isx_orb_params* q, const char* who, OrbPlan& P, int& capacity) {
    ISX_CHECK_ARG(q != nullptr, ISX_ERR_INVALID, "%s: null params", who);
    ISX_CHECK_ARG(q->grid_width >= 1 && q->grid_height >= 1 && q->grid_width <= ISX_ORB_MAX_LAYERS && q->grid_height <= ISX_ORB_MAX_LAYERS, ISX_ERR_INVALID,
                  "%s: a grid of %d x %d cells", who, q->grid_width, q->grid_height);
    ISX_CHECK_ARG(q->n_features >= 0 && q->n_features <= (1 << 24), ISX_ERR_INVALID, "%s: n_features %d is not in [0, 2^24]", who, q->n_features);
    ISX_CHECK_ARG(q->scale_factor > 1.f && q->scale_factor <= 16.f, ISX_ERR_INVALID, "%s: scale_factor %g is not in (1, 16]", who, (double)q->scale_factor);
    ISX_CHECK_ARG(q->nlevels >= 1 && q->nlevels <= ISX_ORB_MAX_LEVELS, ISX_ERR_INVALID, "%s: nlevels %d is not in [1, %d]", who, q->nlevels, ISX_ORB_MAX_LEVELS);
    ISX_CHECK_ARG(q->fast_threshold >= 1 && q->fast_threshold <= 254, ISX_ERR_INVALID, "%s: fast_threshold %d is not in [1, 254]", who, q->fast_threshold);
    ISX_CHECK_ARG(q->patch_size == OB_PATCH && q->edge_threshold == OB_EDGE, ISX_ERR_UNSUPPORTED, "%s: patch_size %d, edge_threshold %d (31 and 31 only)", who,
                  q->patch_size, q->edge_threshold);
    ISX_CHECK_ARG(q->wta_k == 2, ISX_ERR_UNSUPPORTED, "%s: WTA_K %d (2 only)", who, q->wta_k);
    ISX_CHECK_ARG(q->first_level == 0, ISX_ERR_UNSUPPORTED, "%s: firstLevel %d (0 only)", who, q->first_level);
    ISX_CHECK_ARG(q->score_type == ISX_ORB_HARRIS_SCORE, ISX_ERR_UNSUPPORTED, "%s: score type %d (HARRIS_SCORE only)", who, q->score_type);
    const long long cells = (long long)q->grid_width * q->grid_height;
    ISX_CHECK_ARG(cells * q->nlevels <= ISX_ORB_MAX_LAYERS, ISX_ERR_UNSUPPORTED, "%s: %lld cells x %d levels (at most %d layers)", who, cells, q->nlevels, ISX_ORB_MAX_LAYERS);
    std::memset(&P, 0, sizeof(P));
    P.gx = q->grid_width; P.gy = q->grid_height; P.nlevels = q->nlevels; P.fast_threshold = q->fast_threshold;
    const double scale_factor = (double)q->scale_factor;                                  // F:45
    const int area = (int)cells;
    const int per_cell = (int)((long long)q->n_features * (99 + area) / 100 / area);        // F:43
    features_per_level(per_cell, scale_factor, P.nlevels, P.n);
    ISX_CHECK_ARG(2LL * P.n[0] + ISX_ORB_CAND_TIE_ROOM <= ISX_ORB_MAX_CANDIDATES && 2LL * P.n[P.nlevels - 1] + ISX_ORB_CAND_TIE_ROOM <= ISX_ORB_MAX_CANDIDATES,
                  ISX_ERR_UNSUPPORTED, "%s: %d features on a level of a cell (2 n + %d candidates, at most %d)", who, std::max(P.n[0], P.n[P.nlevels - 1]),
                  ISX_ORB_CAND_TIE_ROOM, ISX_ORB_MAX_CANDIDATES);
    for (int l = 0; l < P.nlevels; ++l) {
        P.scale[l] = (float)std::pow(scale_factor, (double)l);                           // F:721-724
        P.inv_scale[l] = 1.f / P.scale[l];                                               // F:299
        P.cand_cap[l] = 2 * P.n[l] + ISX_ORB_CAND_TIE_ROOM; P.cand_off[l] = P.cand_sum; P.cand_sum += P.cand_cap[l];
        P.keep_cap[l] = P.n[l] + ISX_ORB_KEEP_TIE_ROOM; P.keep_off[l] = P.keep_sum; P.keep_sum += P.keep_cap[l];
    }
    capacity = (int)(cells * P.keep_sum);
    // F:88-103
    int umax[OB_HALF + 2] = {0};
    const int vmax = (int)std::floor(OB_HALF * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(OB_HALF * std::sqrt(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) umax[v] = (int)std::rint(std::sqrt((double)OB_HALF * OB_HALF - v * v));
    for (int v = OB_HALF, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
    for (int v = 0; v <= OB_HALF; ++v) P.umax[v] = umax[v];
    const float scale = 1.f / ((1 << 2) * OB_HARRIS * 255.f);                              // F:216-217
    P.harris_scale = scale * scale * scale * scale;
    return ISX_OK;
}

// the geometry of a W x H image under the plan: layer sizes, pitches and the pyramid's bytes
int plan_image(int W, int H, const char* who, OrbPlan& P, long long& pyramid_bytes, int& max_w, int& max_h) {
    ISX_CHECK_ARG(W <= ISX_ORB_MAX_SIDE && H <= ISX_ORB_MAX_SIDE, ISX_ERR_UNSUPPORTED, "%s: an image of %d x %d (at most %d a side)", who, W, H, ISX_ORB_MAX_SIDE);
    ISX_CHECK_ARG(P.gx <= W && P.gy <= H, ISX_ERR_INVALID, "%s: a grid of %d x %d cells on an image of %d x %d", who, P.gx, P.gy, W, H);
    P.W = W; P.H = H; P.cw0 = W / P.gx; P.ch0 = H / P.gy;
    const long long cells = (long long)P.gx * P.gy;
    long long at = (long long)W * H;
    max_w = P.cw0 + 1; max_h = P.ch0 + 1;
    for (int l = 1; l < P.nlevels; ++l) {
        for (int e = 0; e < 2; ++e) {
            P.lw[l][e] = cv_round((float)(P.cw0 + e) / P.scale[l]);                      // F:794
            P.lh[l][e] = cv_round((float)(P.ch0 + e) / P.scale[l]);
        }
        P.pitch[l] = (std::max(P.lw[l][1], 1) + 3) & ~3;
        P.slot[l] = (long long)P.pitch[l] * std::max(P.lh[l][1], 1);
        P.lvl_off[l] = at;
        at += cells * P.slot[l];
    }
    pyramid_bytes = at;
    return ISX_OK;
}

void default_pattern(int* xy) {
    unsigned long long state = 0x34985739ull;                                              // F:711
    auto uniform = [&](int a, int b) {
        state = (unsigned long long)(unsigned)state * 4294883355ull + (state >> 32);
        return a + (int)((unsigned)state % (unsigned)(b - a));
    };
    for (int i = 0; i < OB_PATTERN_POINTS; ++i) {
        xy[2 * i] = uniform(-OB_PATCH / 2, OB_PATCH / 2 + 1);                              // F:715-716
        xy[2 * i + 1] = uniform(-OB_PATCH / 2, OB_PATCH / 2 + 1);
    }
}

// pin / the head of work: the default pattern, then the caller's host pattern; then a staged host image (scratch.hpp has the two ordering rules)
struct ObScratch : UploadScratch {
    void* resident = nullptr;                // where the default pattern has been uploaded: work.p then
};

struct ObLayout {
    size_t o_default, o_user, o_image, upload_bytes, o_pyr, o_score, o_kept, o_blur, o_hist, o_status, o_cand_count, o_keep_count, o_cand_xy, o_cand_resp, o_keep_xy, o_keep_resp;
    size_t zero_bytes;                       // hist and status, cleared by k_orb_gray
};
void lay_out(Bump& lay, const OrbPlan& P, long long pyramid_bytes, size_t image_bytes, ObLayout& o) {
    const size_t layers = (size_t)P.gx * P.gy * P.nlevels, cells = (size_t)P.gx * P.gy;
    o.o_default = lay.take(OB_PATTERN_BYTES); o.o_user = lay.take(OB_PATTERN_BYTES);
    o.o_image = lay.take(image_bytes);
    o.upload_bytes = lay.at;
    o.o_pyr = lay.take((size_t)pyramid_bytes); o.o_score = lay.take((size_t)pyramid_bytes); o.o_kept = lay.take((size_t)pyramid_bytes); o.o_blur = lay.take((size_t)pyramid_bytes);
    o.o_hist = lay.take(layers * 256 * 4);
    o.o_status = lay.take(4);
    o.zero_bytes = lay.at - o.o_hist;
    o.o_cand_count = lay.take(layers * 4); o.o_keep_count = lay.take(layers * 4);
    o.o_cand_xy = lay.take(cells * P.cand_sum * 4); o.o_cand_resp = lay.take(cells * P.cand_sum * 4);
    o.o_keep_xy = lay.take(cells * P.keep_sum * 4); o.o_keep_resp = lay.take(cells * P.keep_sum * 4);
}

}  // namespace

extern "C" {

int isx_orb_default_params(isx_orb_params* params) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(params != nullptr, ISX_ERR_INVALID, "orb_default_params: null params");
    default_params(*params);
    return ISX_OK;
} ISX_EXIT("isx_orb_default_params")

int isx_orb_capacity(const isx_orb_params* params, int* capacity) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(capacity != nullptr, ISX_ERR_INVALID, "orb_capacity: null capacity");
    OrbPlan P;
    int cap = 0;
    ISX_TRY(plan_params(params, "orb_capacity", P, cap));
    *capacity = cap;
    return ISX_OK;
} ISX_EXIT("isx_orb_capacity")

int isx_orb_default_pattern(isx_mat* pattern) ISX_ENTRY {
    clear_error();
    const char* who = "orb_default_pattern";
    ISX_CHECK_ARG(pattern != nullptr, ISX_ERR_INVALID, "%s: null pattern", who);
    ISX_CHECK_ARG(pattern->device < 0, ISX_ERR_INVALID, "%s: the pattern is a device mat (host code: pass a host mat)", who);
    ISX_TRY(check_mat_holds(*pattern, ISX_32SC1, OB_PATTERN_POINTS, 2, 4, STOP_NO_ROW_WANTED, -1, who, "pattern", 0));
    int xy[2 * OB_PATTERN_POINTS];
    default_pattern(xy);
    for (int i = 0; i < OB_PATTERN_POINTS; ++i) std::memcpy((char*)pattern->data + (size_t)i * pattern->step, xy + 2 * i, 8);
    return ISX_OK;
} ISX_EXIT("isx_orb_default_pattern")

int isx_orb_release(void) ISX_ENTRY {
    clear_error();
    ObScratch& s = per_thread<ObScratch>();
    s.resident = nullptr;
    return s.release();
} ISX_EXIT("isx_orb_release")

int isx_orb_reserve(const isx_orb_params* params, int width, int height, int device) ISX_ENTRY {
    clear_error();
    const char* who = "orb_reserve";
    OrbPlan P;
    int cap = 0, max_w = 0, max_h = 0;
    long long pyramid_bytes = 0;
    ISX_TRY(plan_params(params, who, P, cap));
    ISX_CHECK_ARG(width >= 1 && height >= 1, ISX_ERR_SIZE, "%s: an image of %d x %d", who, width, height);
    ISX_TRY(plan_image(width, height, who, P, pyramid_bytes, max_w, max_h));
    Bump lay;
    ObLayout o;
    lay_out(lay, P, pyramid_bytes, 0, o);
    ISX_HIP(hipSetDevice(device));
    ObScratch& s = per_thread<ObScratch>();
    ISX_TRY(s.begin(device, nullptr, std::max(lay.at, s.work.cap), o.upload_bytes));
    std::memset(s.pin.p, 0, o.upload_bytes);
    default_pattern((int*)((char*)s.pin.p + o.o_default));
    ISX_TRY(s.upload(nullptr, o.upload_bytes));
    ISX_TRY(s.wait_upload());
    s.resident = s.work.p;
    return ISX_OK;
} ISX_EXIT("isx_orb_reserve")

int isx_orb_find(const isx_mat* image, const isx_orb_params* params, const isx_mat* pattern, isx_mat* keypoints, isx_mat* meta,
                 isx_mat* descriptors, isx_mat* count_status, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "orb_find";
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(image && keypoints && meta && descriptors && count_status, ISX_ERR_INVALID, "%s: null image, keypoints, meta, descriptors or count_status", who);
    OrbPlan P;
    int cap = 0, max_w = 0, max_h = 0;
    long long pyramid_bytes = 0;
    ISX_TRY(plan_params(params, who, P, cap));
    ISX_CHECK_ARG(image->type == ISX_8UC1 || image->type == ISX_8UC3 || image->type == ISX_8UC4, ISX_ERR_TYPE, "%s: the image is %s (CV_8UC1, CV_8UC3 or CV_8UC4)", who,
                  type_name(image->type));
    ISX_CHECK_ARG(image->rows >= 1 && image->cols >= 1, ISX_ERR_SIZE, "%s: an image of %d x %d", who, image->cols, image->rows);
    const int cn = mat_cn(image->type), W = image->cols, H = image->rows;
    ISX_TRY(plan_image(W, H, who, P, pyramid_bytes, max_w, max_h));
    ISX_CHECK_ARG(image->data != nullptr, ISX_ERR_INVALID, "%s: the image has a null data pointer", who);
    ISX_CHECK_ARG(image->step >= (size_t)W * cn || H == 1, ISX_ERR_INVALID, "%s: the image's step %zu is smaller than a row", who, image->step);
    ISX_CHECK_ARG(image->device < 0 || image->device == device, ISX_ERR_INVALID, "%s: the image lives on device %d, the call runs on %d", who, image->device, device);
    if (pattern) {
        ISX_CHECK_ARG(pattern->type == ISX_32SC1, ISX_ERR_TYPE, "%s: the pattern is %s (CV_32SC1)", who, type_name(pattern->type));
        ISX_CHECK_ARG(pattern->rows == OB_PATTERN_POINTS && pattern->cols == 2, ISX_ERR_SIZE, "%s: the pattern is %d x %d (512 x 2)", who, pattern->rows, pattern->cols);
        ISX_TRY(check_mat_holds(*pattern, ISX_32SC1, OB_PATTERN_POINTS, 2, 4, STOP_NO_ROW_WANTED, device, who, "pattern", 0));
        if (pattern->device < 0)
            for (int i = 0; i < OB_PATTERN_POINTS; ++i) {
                const int* r = (const int*)((const char*)pattern->data + (size_t)i * pattern->step);
                ISX_CHECK_ARG(r[0] >= -OB_HALF && r[0] <= OB_HALF && r[1] >= -OB_HALF && r[1] <= OB_HALF, ISX_ERR_INVALID,
                              "%s: pattern point %d is (%d, %d): outside the 31 x 31 patch", who, i, r[0], r[1]);
            }
    }
    ISX_TRY(check_mat_holds(*keypoints, ISX_32FC1, cap, 2, 4, STOP_NO_ROW_WANTED, device, who, "keypoints", 0));
    ISX_TRY(check_mat_holds(*meta, ISX_32FC1, cap, 4, 4, STOP_NO_ROW_WANTED, device, who, "meta", 0));
    ISX_TRY(check_mat_holds(*descriptors, ISX_8UC1, cap, 32, 1, STOP_NO_ROW_WANTED, device, who, "descriptors", 0));
    ISX_TRY(check_mat_holds(*count_status, ISX_32SC1, 1, 2, 4, STOP_NO_ROW_WANTED, device, who, "count_status", 0));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    bool capturing = false;
    ISX_TRY(is_capturing(st, capturing));
    const bool host_pattern = pattern && pattern->device < 0;
    const bool any_host = image->device < 0 || host_pattern || keypoints->device < 0 || meta->device < 0 || descriptors->device < 0 || count_status->device < 0;
    ISX_CHECK_ARG(!capturing || !any_host, ISX_ERR_STATE, "%s: the stream is capturing and a mat is a host mat (staging it synchronises)", who);

    // ---- one buffer: [upload: default pattern | host pattern | staged host image] [4 pyramids] [hist | status] [counts] [candidates] [kept]
    //      [staged host outputs]
    Bump lay;
    ObLayout o;
    const size_t image_bytes = image->device < 0 ? (size_t)H * W * cn : 0;
    lay_out(lay, P, pyramid_bytes, image_bytes, o);
    StagedMat m_kp, m_meta, m_desc, m_cs;
    m_kp.plan(lay, *keypoints, cap, 8);
    m_meta.plan(lay, *meta, cap, 16);
    m_desc.plan(lay, *descriptors, cap, 32);
    m_cs.plan(lay, *count_status, 1, 8);

    ObScratch& s = per_thread<ObScratch>();
    if (capturing) {
        // nothing may be allocated, uploaded or fenced inside a capture: the scratch holds the call as it is, or the call is refused
        ISX_CHECK_ARG(s.device == device && s.work.cap >= lay.at && s.resident != nullptr && s.resident == s.work.p, ISX_ERR_STATE,
                      "%s: the stream is capturing and the scratch would have to grow (isx_orb_reserve first)", who);
    } else {
        ISX_TRY(s.begin(device, st, lay.at, o.upload_bytes));
        char* const pin = (char*)s.pin.p;
        default_pattern((int*)(pin + o.o_default));
        if (host_pattern)
            for (int i = 0; i < OB_PATTERN_POINTS; ++i) std::memcpy(pin + o.o_user + 8 * i, (const char*)pattern->data + (size_t)i * pattern->step, 8);
        else std::memset(pin + o.o_user, 0, OB_PATTERN_BYTES);
        if (image->device < 0)
            for (int r = 0; r < H; ++r) std::memcpy(pin + o.o_image + (size_t)r * W * cn, (const char*)image->data + (size_t)r * image->step, (size_t)W * cn);
        ISX_TRY(s.upload(st, o.upload_bytes));
        s.resident = s.work.p;
    }
    char* const dev = (char*)s.work.p;

    const unsigned char* d_img = image->device < 0 ? (const unsigned char*)(dev + o.o_image) : (const unsigned char*)image->data;
    const long long img_step = image->device < 0 ? (long long)W * cn : (long long)image->step;
    const unsigned char* d_pat = !pattern ? (const unsigned char*)(dev + o.o_default) : host_pattern ? (const unsigned char*)(dev + o.o_user) : (const unsigned char*)pattern->data;
    const long long pat_step = pattern && !host_pattern ? (long long)pattern->step : 8;
    unsigned char* const d_pyr = (unsigned char*)(dev + o.o_pyr);
    unsigned char* const d_score = (unsigned char*)(dev + o.o_score);
    unsigned char* const d_kept = (unsigned char*)(dev + o.o_kept);
    unsigned char* const d_blur = (unsigned char*)(dev + o.o_blur);
    int* const d_hist = (int*)(dev + o.o_hist);
    int* const d_status = (int*)(dev + o.o_status);
    int* const d_cand_count = (int*)(dev + o.o_cand_count);
    int* const d_keep_count = (int*)(dev + o.o_keep_count);
    int* const d_cand_xy = (int*)(dev + o.o_cand_xy);
    float* const d_cand_resp = (float*)(dev + o.o_cand_resp);
    int* const d_keep_xy = (int*)(dev + o.o_keep_xy);
    float* const d_keep_resp = (float*)(dev + o.o_keep_resp);
    OrbOut O;
    m_kp.bind(dev, O.kp, O.kp_step);
    m_meta.bind(dev, O.meta, O.meta_step);
    m_desc.bind(dev, O.desc, O.desc_step);
    m_cs.bind(dev, O.count_status);

    // ---- the launches ----
    const int cells = P.gx * P.gy, layers = cells * P.nlevels;
    int max_cand = 0, max_keep = 0;
    for (int l = 0; l < P.nlevels; ++l) { max_cand = std::max(max_cand, P.cand_cap[l]); max_keep = std::max(max_keep, P.keep_cap[l]); }
    const double px = (double)W * H;
    const dim3 pixel_grid(cdiv(max_w, WAVE), cdiv(max_h, 4), layers);
    const dim3 gray_grid(cdiv(W, 256), H);
    const int zero_words = (int)(o.zero_bytes / 4);
    if (cn == 1) ISX_LAUNCH("orb_gray", px * 2, st, k_orb_gray<1>, gray_grid, dim3(256), 0, d_img, img_step, W, H, d_pyr, d_hist, zero_words);
    else if (cn == 3) ISX_LAUNCH("orb_gray", px * 4, st, k_orb_gray<3>, gray_grid, dim3(256), 0, d_img, img_step, W, H, d_pyr, d_hist, zero_words);
    else ISX_LAUNCH("orb_gray", px * 5, st, k_orb_gray<4>, gray_grid, dim3(256), 0, d_img, img_step, W, H, d_pyr, d_hist, zero_words);
    for (int l = 1; l < P.nlevels; ++l) {
        if (P.lw[l][1] <= 0 || P.lh[l][1] <= 0) break;       // no cell has pixels on this level, nor on those above
        ISX_LAUNCH("orb_resize", px, st, k_orb_resize, dim3(cdiv(P.lw[l][1], WAVE), cdiv(P.lh[l][1], 4), cells), dim3(256), 0, P, l, d_pyr);
    }
    ISX_LAUNCH("orb_fast", px * 2, st, k_orb_fast, pixel_grid, dim3(256), 0, P, (const unsigned char*)d_pyr, d_score);
    ISX_LAUNCH("orb_nms", px * 2, st, k_orb_nms, pixel_grid, dim3(256), 0, P, (const unsigned char*)d_score, d_kept, d_hist);
    ISX_LAUNCH("orb_first_cut", px, st, k_orb_first_cut, dim3(layers), dim3(OB_CUT_NT), 0, P, (const unsigned char*)d_kept, (const int*)d_hist, d_cand_xy, d_cand_count,
               d_status);
    ISX_LAUNCH("orb_harris", (double)layers * max_cand * 81, st, k_orb_harris, dim3(cdiv(max_cand, 256), layers), dim3(256), 0, P, (const unsigned char*)d_pyr,
               (const int*)d_cand_xy, (const int*)d_cand_count, d_cand_resp);
    ISX_LAUNCH("orb_final_cut", (double)layers * max_cand * 8, st, k_orb_final_cut, dim3(layers), dim3(OB_CUT_NT), 0, P, (const int*)d_cand_xy, (const float*)d_cand_resp,
               (const int*)d_cand_count, d_keep_xy, d_keep_resp, d_keep_count, d_status);
    ISX_LAUNCH("orb_blur", px * 2, st, k_orb_blur, pixel_grid, dim3(256), 0, P, (const unsigned char*)d_pyr, d_blur);
    ISX_LAUNCH("orb_describe", (double)layers * max_keep * 1024, st, k_orb_describe, dim3(cdiv(max_keep, OB_DESC_NT / WAVE), layers), dim3(OB_DESC_NT), 0, P,
               (const unsigned char*)d_pyr, (const unsigned char*)d_blur, d_pat, pat_step, (const int*)d_keep_xy, (const float*)d_keep_resp, (const int*)d_keep_count,
               (const int*)d_status, O);
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
} ISX_EXIT("isx_orb_find")

}  // extern "C"
