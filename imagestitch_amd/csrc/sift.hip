// sift.hip — SIFT::detectAndCompute(image, noArray()) of OpenCV 4.x (features2d/src/sift.dispatch.cpp on sift.simd.hpp, float DoG), the finder
// cv::Stitcher and stitching_detailed --features sift offer beside ORB and SURF, on gfx950:
//   isx_sift_find      128 floats a keypoint
//   isx_sift_reserve   sizes the per-thread scratch ahead of a capture
//   isx_sift_release   returns it
//   isx_sift_default_params, isx_selftest_sift_math   host code
//
// The specification (DESIGN.md §8 "Features finder, SIFT"; tests/helpers/sift_np.py, matched bit for bit; OpenCV parity is unpinned): every
// float operation is rounded on its own in the order the model writes it, exp and exp2 are sift_math.hpp's, the trigonometry is
// proj_math.hpp's, the six blur kernels are sift_tables.hpp's literals.
//
// The launches, 10 + 11 n - (n > 0) for n built octaves (n depends on the image size alone):
//   k_sift_base      gray, the 2 x INTER_LINEAR upsample in float32                                              (1)
//   k_sift_blur      <false> the row pass, <true> the column pass of one blur and the DoG of the layer it completes; a work item a pixel
//                    (2 for the base image, 10 an octave)
//   k_sift_half      layer 0 of the next octave from layer 3 at (2 x, 2 y)                                      (n - 1)
//   k_sift_extrema   <false> a workgroup takes 256 consecutive positions of the scan order (octave, layer, r, c), tests the 26 neighbours,
//                    runs adjustLocalExtrema and counts what survives; <true> does the same again and writes each candidate at the prefix
//                    of the counts: the candidates lie in scan order whatever the scheduling                     (2)
//   k_sift_prefix    one workgroup: the exclusive prefix of the workgroups' counts, the number of candidates, the overflow bit
//   k_sift_rank      every candidate counts the candidates before it in the total order and looks for an earlier candidate with its final
//                    (octave, layer, r, c) (LDS tiles): order[rank] = candidate, dup[candidate]
//   k_sift_orient    a workgroup a ranked candidate: every sample's (bin, value) into LDS in parallel, then a work item a bin walks the
//                    list in sample order; smoothing, the peaks in bin order
//   k_sift_compact   one workgroup: the first output row of every ranked candidate, the count and the status
//   k_sift_describe  a workgroup a keypoint: 512 samples at a time into LDS, then a work item a cell of the 6 x 6 x 10 histogram walks them
//                    in sample order; the fold, the two norms, the rounding
// No float atomics, no atomics at all; nothing read back on device mats.
#include "isx_device.hpp"
#include "block_scan.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"
#include "resize_taps.hpp"
#include "sift_math.hpp"
#include "sift_tables.hpp"

#include <cfloat>
#include <cmath>

using namespace isx;
using namespace isxd;

namespace {

constexpr int SI_OCT = 12, SI_LAYERS = 3, SI_G = SI_LAYERS + 3, SI_D = SI_LAYERS + 2, SI_BORDER = 5, SI_STEPS = 5;
constexpr int SI_MAX = ISX_SIFT_MAX_CANDIDATES;
constexpr int SI_ORI_NT = 256, SI_ORI_BINS = 36, SI_ORI_RMAX = 16, SI_ORI_LEN = (2 * SI_ORI_RMAX + 1) * (2 * SI_ORI_RMAX + 1), SI_PEAKS = 18;
constexpr int SI_DESC_NT = 512, SI_HIST = 6 * 6 * 10;
constexpr int SI_SCAN_NT = 1024;
static_assert(SI_MAX % SI_SCAN_NT == 0, "a thread of the compaction owns a whole stride of the candidates");
static_assert(SI_HIST <= SI_DESC_NT, "a work item a histogram cell");
static_assert((ISX_SIFT_MAX_SIDE * 2) >> (SI_OCT - 1) < 2 * SI_BORDER + 1, "every octave that can be built has a slot");

// what the kernels are told: the built octaves, where their layers lie (floats from the pyramid's base; layer l of octave o is
// goff[o] + l * rows[o] * cols[o], a DoG layer doff[o] + l * rows[o] * cols[o]), the search workgroups
struct SiPlan {
    int W, H, noct;
    int rows[SI_OCT], cols[SI_OCT];
    long long goff[SI_OCT], doff[SI_OCT];
    int blk_off[SI_OCT * SI_LAYERS + 1];      // the search workgroups of (o, l) are blk_off[o * 3 + l - 1] .. blk_off[o * 3 + l]
    int nblocks, nfeatures;
    float thr, ct, et;
    long long pyr_floats, tmp_floats;
};

struct SiOut {
    float* kp; long long kp_step;
    float* meta; long long meta_step;
    float* desc; long long desc_step;
    int* count_status;
    int cap;
};

// gray as isx_orb_find makes it, then cv::resize(Size(2 W, 2 H), INTER_LINEAR) on CV_32F with resize_taps.hpp's taps: 64 x 4 pixels a workgroup
template <int CN>
__global__ __launch_bounds__(256) void k_sift_base(const unsigned char* __restrict__ src, long long sstep, int W, int H, double scale_x, double scale_y,
                                                   float* __restrict__ dst) {
    const int x = (int)(blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1))), y = (int)(blockIdx.y * 4 + threadIdx.x / WAVE);
    if (x >= 2 * W || y >= 2 * H) return;
    const ColTap ct = col_tap(x, scale_x, W);
    const RowTap rt = row_tap(y, scale_y, H);
    const bool two = ct.sx + 1 < W;
    const float a0 = 1.f - ct.a1, b0 = 1.f - rt.fy;
    float h[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned char* p = src + (long long)(k ? rt.sy1 : rt.sy0) * sstep + (long long)ct.sx * CN;
        float g0, g1 = 0.f;
        if constexpr (CN == 1) {
            g0 = (float)p[0];
            if (two) g1 = (float)p[1];
        } else {
            g0 = (float)(((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + 8192) >> 14);
            if (two) g1 = (float)(((int)p[CN] * 1868 + (int)p[CN + 1] * 9617 + (int)p[CN + 2] * 4899 + 8192) >> 14);
        }
        h[k] = two ? g0 * a0 + g1 * ct.a1 : g0;
    }
    dst[y * (2 * W) + x] = h[0] * b0 + h[1] * rt.fy;
}

// One pass of GaussianBlur with kernel `kern` of sift_tables.hpp: t[h] a[0], then t[h + j] (a[+j] + a[-j]) for j = 1 .. h.  COLS: down the
// columns, and dog = dst - prev where dog is given.  Offsets inside a layer are 32-bit; the layers' bases are the caller's pointers.
template <bool COLS>
__global__ __launch_bounds__(256) void k_sift_blur(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ prev, float* __restrict__ dog,
                                                   int rows, int cols, int kern) {
    const int x = (int)(blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1))), y = (int)(blockIdx.y * 4 + threadIdx.x / WAVE);
    if (x >= cols || y >= rows) return;
    const int first = isxsi::sift_tap_first(kern), h = isxsi::sift_tap_width(kern) / 2;
    const int n = COLS ? rows : cols, pos = COLS ? y : x, stride = COLS ? cols : 1;
    const float* line = COLS ? src + x : src + y * cols;
    float acc = line[pos * stride] * isxsi::sift_tap(first + h);
    for (int j = 1; j <= h; ++j) {
        const float pair = line[reflect101(pos + j, n) * stride] + line[reflect101(pos - j, n) * stride];
        acc = acc + isxsi::sift_tap(first + h + j) * pair;
    }
    const int at = y * cols + x;
    dst[at] = acc;
    if (COLS && dog) dog[at] = acc - prev[at];
}

// resize(layer 3, Size(cols / 2, rows / 2), INTER_NEAREST): the pixel at (2 x, 2 y)
__global__ __launch_bounds__(256) void k_sift_half(const float* __restrict__ src, int scols, float* __restrict__ dst, int rows, int cols) {
    const int x = (int)(blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1))), y = (int)(blockIdx.y * 4 + threadIdx.x / WAVE);
    if (x >= cols || y >= rows) return;
    dst[y * cols + x] = src[(2 * y) * scols + 2 * x];
}

struct SiDeriv { float dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys; };
// the derivatives of adjustLocalExtrema at p = &dog(layer, r, c); LS is a layer's floats
__device__ __forceinline__ SiDeriv si_derivs(const float* __restrict__ p, int LS, int cols) {
    const float img_scale = 1.f / 255.f, deriv_scale = img_scale * 0.5f, second_deriv_scale = img_scale, cross_deriv_scale = img_scale * 0.25f;
    SiDeriv d;
    d.dx = (p[1] - p[-1]) * deriv_scale;
    d.dy = (p[cols] - p[-cols]) * deriv_scale;
    d.ds = (p[LS] - p[-LS]) * deriv_scale;
    const float v2 = p[0] * 2.f;
    d.dxx = (p[1] + p[-1] - v2) * second_deriv_scale;
    d.dyy = (p[cols] + p[-cols] - v2) * second_deriv_scale;
    d.dss = (p[LS] + p[-LS] - v2) * second_deriv_scale;
    d.dxy = (p[cols + 1] - p[cols - 1] - p[-cols + 1] + p[-cols - 1]) * cross_deriv_scale;
    d.dxs = (p[LS + 1] - p[LS - 1] - p[-LS + 1] + p[-LS - 1]) * cross_deriv_scale;
    d.dys = (p[LS + cols] - p[LS - cols] - p[-LS + cols] + p[-LS - cols]) * cross_deriv_scale;
    return d;
}

struct SiCand { float x, y, size, response; int layer, r, c; };
// adjustLocalExtrema from the starting pixel (l, r, c) of octave o, whose DoG layers start at D
__device__ bool si_adjust(const float* __restrict__ D, int rows, int cols, int o, int l, int r, int c, float ct, float et, SiCand& out) {
    const int LS = rows * cols;
    const float huge = (float)(INT_MAX / 3);
    float xi = 0.f, xr = 0.f, xc = 0.f;
    int i = 0;
    for (; i < SI_STEPS; ++i) {
        const SiDeriv d = si_derivs(D + (long long)l * LS + r * cols + c, LS, cols);
        float x0 = 0.f, x1 = 0.f, x2 = 0.f;      // Matx::solve gives zeros where the solve fails
        fast_solve3(d.dxx, d.dxy, d.dxs, d.dxy, d.dyy, d.dys, d.dxs, d.dys, d.dss, d.dx, d.dy, d.ds, x0, x1, x2);
        xi = -x2; xr = -x1; xc = -x0;
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        if (fabsf(xi) > huge || fabsf(xr) > huge || fabsf(xc) > huge) return false;
        // (a NaN passes both tests and rounds to INT_MIN as cvRound does: the sums below wrap to a negative index and the candidate leaves)
        c = (int)((unsigned)c + (unsigned)cvround_x86(xc));
        r = (int)((unsigned)r + (unsigned)cvround_x86(xr));
        l = (int)((unsigned)l + (unsigned)cvround_x86(xi));
        if (l < 1 || l > SI_LAYERS || c < SI_BORDER || c >= cols - SI_BORDER || r < SI_BORDER || r >= rows - SI_BORDER) return false;
    }
    if (i >= SI_STEPS) return false;
    const float* p = D + (long long)l * LS + r * cols + c;
    const SiDeriv d = si_derivs(p, LS, cols);
    const float t = d.dx * xc + d.dy * xr + d.ds * xi;
    const float contr = p[0] * (1.f / 255.f) + t * 0.5f;
    if (fabsf(contr) * (float)SI_LAYERS < ct) return false;
    const float tr = d.dxx + d.dyy, det = d.dxx * d.dyy - d.dxy * d.dxy;
    if (det <= 0.f || tr * tr * et >= (et + 1.f) * (et + 1.f) * det) return false;
    const float two_o = (float)(1 << o);
    out.x = ((float)c + xc) * two_o;
    out.y = ((float)r + xr) * two_o;
    out.size = 1.6f * isxpm::pm_exp2f(((float)l + xi) / (float)SI_LAYERS) * two_o * 2.f;
    out.response = fabsf(contr);
    out.layer = l; out.r = r; out.c = c;
    return true;
}

// candidates: four rows of SI_MAX floats (pt.x, pt.y, size before the halving, response) and two of ints (octave * 4 + layer, r << 16 | c)
template <bool WRITE>
__global__ __launch_bounds__(256) void k_sift_extrema(SiPlan P, const float* __restrict__ pyr, int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                                      float* __restrict__ cand, int* __restrict__ cand_i) {
    __shared__ int s_cnt[256 / WAVE];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    if (blk >= P.nblocks) return;
    int idx = 0;
    while (blk >= P.blk_off[idx + 1]) ++idx;
    const int o = idx / SI_LAYERS, l = idx % SI_LAYERS + 1;
    const int rows = P.rows[o], cols = P.cols[o], nr = rows - 2 * SI_BORDER, nc = cols - 2 * SI_BORDER, LS = rows * cols;
    const long long p = (long long)(blk - P.blk_off[idx]) * 256 + t;
    bool keep = false;
    SiCand K;
    if (p < (long long)nr * nc) {
        const int r = (int)(p / nc) + SI_BORDER, c = (int)(p % nc) + SI_BORDER;
        const float* D = pyr + P.doff[o];
        const float* d1 = D + (long long)l * LS + r * cols + c;
        const float v = d1[0];
        if (fabsf(v) > P.thr && v != 0.f) {
            bool ge = true, le = true;
#pragma unroll
            for (int k = -1; k <= 1; ++k)
#pragma unroll
                for (int a = -1; a <= 1; ++a)
#pragma unroll
                    for (int b = -1; b <= 1; ++b) {
                        const float w = d1[k * LS + a * cols + b];
                        ge = ge && v >= w; le = le && v <= w;
                    }
            if (v > 0.f ? ge : le) keep = si_adjust(D, rows, cols, o, l, r, c, P.ct, P.et, K);
        }
    }
    int total;
    const int before = block_count_before<256>(keep, s_cnt, total);
    if constexpr (!WRITE) {
        if (t == 0) blk_count[blk] = total;
    } else {
        const long long at = (long long)blk_base[blk] + before;
        if (keep && at < SI_MAX) {
            cand[at] = K.x; cand[SI_MAX + at] = K.y; cand[2 * SI_MAX + at] = K.size; cand[3 * SI_MAX + at] = K.response;
            cand_i[at] = o * 4 + K.layer; cand_i[SI_MAX + at] = (K.r << 16) | K.c;
        }
    }
}

__global__ __launch_bounds__(SI_SCAN_NT) void k_sift_prefix(int n, const int* __restrict__ cnt, int* __restrict__ base, int* __restrict__ ncand_status) {
    __shared__ int s_tot[SI_SCAN_NT / WAVE];
    const int t = (int)threadIdx.x, chunk = (n + SI_SCAN_NT - 1) / SI_SCAN_NT;
    const long long lo = (long long)t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    long long mine = 0;
    for (long long i = lo; i < hi; ++i) mine += cnt[i];
    // (a count that passes 2^31 cannot occur: there are fewer search positions than ISX_SIFT_MAX_PIXELS * 4 * 4 / 3 * 3 = 2^27)
    int total;
    int run = block_sum_before<SI_SCAN_NT>((int)mine, s_tot, total);
    for (long long i = lo; i < hi; ++i) { base[i] = run; run += cnt[i]; }
    if (t == 0) {
        ncand_status[0] = total < SI_MAX ? total : SI_MAX;
        ncand_status[1] = total > SI_MAX ? (int)ISX_SIFT_CANDIDATES_DROPPED : 0;
    }
}

// rank of candidate i = the candidates before it: response, size, octave, pt.y, pt.x descending, then the scan index ascending;
// dup[i] = an earlier candidate in scan order has the same final (octave, layer, r, c)
__global__ __launch_bounds__(256) void k_sift_rank(const float* __restrict__ cand, const int* __restrict__ cand_i, const int* __restrict__ ncand_status,
                                                   int* __restrict__ order, int* __restrict__ dup) {
    __shared__ float s_k[4][256];
    __shared__ int s_i[2][256];
    const int n = ncand_status[0], t = (int)threadIdx.x, i = (int)blockIdx.x * 256 + t;
    if ((int)blockIdx.x * 256 >= n) return;
    const bool live = i < n;
    const int ii = live ? i : 0;
    const float r = cand[3 * SI_MAX + ii], s = cand[2 * SI_MAX + ii], y = cand[SI_MAX + ii], x = cand[ii];
    const int ol = cand_i[ii], rc = cand_i[SI_MAX + ii], o = ol >> 2;
    int rank = 0, same = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        if (j0 + t < n) {
            s_k[0][t] = cand[3 * SI_MAX + j0 + t]; s_k[1][t] = cand[2 * SI_MAX + j0 + t]; s_k[2][t] = cand[SI_MAX + j0 + t]; s_k[3][t] = cand[j0 + t];
            s_i[0][t] = cand_i[j0 + t]; s_i[1][t] = cand_i[SI_MAX + j0 + t];
        }
        __syncthreads();
        const int m = n - j0 < 256 ? n - j0 : 256;
        for (int jj = 0; jj < m; ++jj) {
            const float rj = s_k[0][jj], sj = s_k[1][jj], yj = s_k[2][jj], xj = s_k[3][jj];
            const int olj = s_i[0][jj], oj = olj >> 2;
            const bool before = rj > r || (rj == r && (sj > s || (sj == s && (oj > o || (oj == o && (yj > y || (yj == y && (xj > x || (xj == x && j0 + jj < i)))))))));
            rank += before ? 1 : 0;
            same += (olj == ol && s_i[1][jj] == rc && j0 + jj < i) ? 1 : 0;
        }
    }
    if (live) { order[rank] = i; dup[i] = same > 0 ? 1 : 0; }
}

__device__ __forceinline__ float si_atan2deg(float y, float x) {
    float a = isxpm::pm_atan2f(y, x) * (float)(180.0 / 3.14159265358979323846);
    if (a < 0.f) a = a + 360.f;
    if (a >= 360.f) a = a - 360.f;
    return a;
}

// calcOrientationHist and the peaks of ranked candidate q = blockIdx.x: npeaks[q], angles[q * SI_PEAKS ..]
__global__ __launch_bounds__(SI_ORI_NT) void k_sift_orient(SiPlan P, const float* __restrict__ pyr, const float* __restrict__ cand, const int* __restrict__ cand_i,
                                                           const int* __restrict__ ncand_status, const int* __restrict__ order, const int* __restrict__ dup,
                                                           int* __restrict__ npeaks, float* __restrict__ angles) {
    __shared__ int s_bin[SI_ORI_LEN];
    __shared__ float s_val[SI_ORI_LEN], s_raw[SI_ORI_BINS], s_hist[SI_ORI_BINS];
    const int q = (int)blockIdx.x, t = (int)threadIdx.x;
    if (q >= ncand_status[0]) return;
    const int ci = order[q];
    if (dup[ci]) {
        if (t == 0) npeaks[q] = 0;
        return;
    }
    const int ol = cand_i[ci], rc = cand_i[SI_MAX + ci], o = ol >> 2, l = ol & 3, r = rc >> 16, c = rc & 0xFFFF;
    const int rows = P.rows[o], cols = P.cols[o];
    const float* img = pyr + P.goff[o] + (long long)l * rows * cols;
    const float scl = cand[2 * SI_MAX + ci] * 0.5f / (float)(1 << o);
    int radius = cvround_x86(4.5f * scl);
    radius = radius < SI_ORI_RMAX ? radius : SI_ORI_RMAX;      // (layer + xi < 3.5, so 4.5f * 1.6f * 2^(3.5 / 3) = 16.2 bounds it)
    const float sigma = 1.5f * scl, expf_scale = -1.f / (2.f * sigma * sigma);
    const int w = 2 * radius + 1, len = w * w;
    for (int k = t; k < len; k += SI_ORI_NT) {
        const int i = k / w - radius, j = k % w - radius, y = r + i, x = c + j;
        int bin = -1;
        float val = 0.f;
        if (y > 0 && y < rows - 1 && x > 0 && x < cols - 1) {
            const float* p = img + y * cols + x;
            const float dx = p[1] - p[-1], dy = p[-cols] - p[cols];
            const float wgt = isxpm::pm_expf((float)(i * i + j * j) * expf_scale);
            const float ori = si_atan2deg(dy, dx), mag = sqrtf(dx * dx + dy * dy);
            bin = cvround_x86((float)(36.0 / 360.0) * ori);
            if (bin >= SI_ORI_BINS) bin -= SI_ORI_BINS;
            if (bin < 0) bin += SI_ORI_BINS;
            val = wgt * mag;
        }
        s_bin[k] = bin; s_val[k] = val;
    }
    __syncthreads();
    if (t < SI_ORI_BINS) {
        float h = 0.f;
        for (int k = 0; k < len; ++k)
            if (s_bin[k] == t) h += s_val[k];
        s_raw[t] = h;
    }
    __syncthreads();
    if (t < SI_ORI_BINS) {
        const float m2 = s_raw[(t + SI_ORI_BINS - 2) % SI_ORI_BINS], m1 = s_raw[(t + SI_ORI_BINS - 1) % SI_ORI_BINS], p1 = s_raw[(t + 1) % SI_ORI_BINS],
                    p2 = s_raw[(t + 2) % SI_ORI_BINS];
        s_hist[t] = (m2 + p2) * (1.f / 16.f) + (m1 + p1) * (4.f / 16.f) + s_raw[t] * (6.f / 16.f);
    }
    __syncthreads();
    if (t == 0) {
        float top = s_hist[0];
        for (int k = 1; k < SI_ORI_BINS; ++k) top = s_hist[k] > top ? s_hist[k] : top;
        const float thr = top * 0.8f;
        int np = 0;
        for (int k = 0; k < SI_ORI_BINS; ++k) {
            const float lf = s_hist[k > 0 ? k - 1 : SI_ORI_BINS - 1], rt = s_hist[k < SI_ORI_BINS - 1 ? k + 1 : 0], hk = s_hist[k];
            if (hk > lf && hk > rt && hk >= thr && np < SI_PEAKS) {
                float bin = (float)k + 0.5f * (lf - rt) / (lf - 2.f * hk + rt);
                bin = bin < 0.f ? (float)SI_ORI_BINS + bin : (bin >= (float)SI_ORI_BINS ? bin - (float)SI_ORI_BINS : bin);
                float ang = 360.f - 10.f * bin;
                if (fabsf(ang - 360.f) < FLT_EPSILON) ang = 0.f;
                angles[q * SI_PEAKS + np] = ang;
                ++np;
            }
        }
        npeaks[q] = np;
    }
}

// the first output row of every ranked candidate, the count and the status
__global__ __launch_bounds__(SI_SCAN_NT) void k_sift_compact(const int* __restrict__ ncand_status, const int* __restrict__ npeaks, int* __restrict__ first,
                                                             int nfeatures, SiOut O) {
    __shared__ int s_tot[SI_SCAN_NT / WAVE];
    const int n = ncand_status[0], t = (int)threadIdx.x, chunk = SI_MAX / SI_SCAN_NT;
    const int lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += npeaks[i];
    int total;
    int run = block_sum_before<SI_SCAN_NT>(mine, s_tot, total);
    for (int i = lo; i < hi; ++i) { first[i] = run; run += npeaks[i]; }
    if (t == 0) {
        const int kept = nfeatures > 0 && total > nfeatures ? nfeatures : total;
        O.count_status[0] = kept < O.cap ? kept : O.cap;
        O.count_status[1] = ncand_status[1] | (kept > O.cap ? (int)ISX_SIFT_TRUNCATED : 0);
    }
}

// calcSIFTDescriptor of output row blockIdx.x
__global__ __launch_bounds__(SI_DESC_NT) void k_sift_describe(SiPlan P, const float* __restrict__ pyr, const float* __restrict__ cand, const int* __restrict__ cand_i,
                                                              const int* __restrict__ ncand_status, const int* __restrict__ order, const int* __restrict__ first,
                                                              const float* __restrict__ angles, SiOut O) {
    __shared__ int s_base[SI_DESC_NT];
    __shared__ float s_v[SI_DESC_NT][8], s_hist[SI_HIST], s_dst[128];
    const int row = (int)blockIdx.x, t = (int)threadIdx.x;
    if (row >= O.count_status[0]) return;
    // the last ranked candidate whose first row is not past this one (candidates without a peak share their successor's first row)
    int lo = 0, hi = ncand_status[0] - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= row) lo = mid; else hi = mid - 1;
    }
    const int q = lo, ci = order[q];
    const float angle = angles[q * SI_PEAKS + (row - first[q])];
    const int ol = cand_i[ci], o = ol >> 2, l = ol & 3;
    const int rows = P.rows[o], cols = P.cols[o];
    const float* img = pyr + P.goff[o] + (long long)l * rows * cols;
    const float two_o = (float)(1 << o), size = cand[2 * SI_MAX + ci], ptx = cand[ci], pty = cand[SI_MAX + ci];
    const float scl = size * 0.5f / two_o;
    float ori = 360.f - angle;
    if (fabsf(ori - 360.f) < FLT_EPSILON) ori = 0.f;
    const int px = cvround_x86(ptx / two_o), py = cvround_x86(pty / two_o);
    float sn, cs;
    isxpm::pm_sincosf(ori * (float)(3.14159265358979323846 / 180.0), sn, cs);
    const float bins_per_rad = (float)(8.0 / 360.0), exp_scale = -1.f / (4.f * 4.f * 0.5f), hist_width = 3.f * scl;
    int radius = cvround_x86(hist_width * 1.4142135623730951f * 5.f * 0.5f);
    const int diag = (int)sqrt((double)cols * (double)cols + (double)rows * (double)rows);
    radius = radius < diag ? radius : diag;
    const float cos_t = cs / hist_width, sin_t = sn / hist_width;
    const int w = 2 * radius + 1;
    const long long len = (long long)w * w;
    const int ri = t / 60, cj = (t / 10) % 6, ok_ = t % 10;       // this work item's cell of the 6 x 6 x 10 histogram
    float cell = 0.f;
    for (long long k0 = 0; k0 < len; k0 += SI_DESC_NT) {
        const long long k = k0 + t;
        int base = -1;
        if (k < len) {
            const int i = (int)(k / w) - radius, j = (int)(k % w) - radius;
            const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
            float rbin = r_rot + 2.f - 0.5f, cbin = c_rot + 2.f - 0.5f;
            const int r = py + i, c = px + j;
            if (rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && r > 0 && r < rows - 1 && c > 0 && c < cols - 1) {
                const float* p = img + r * cols + c;
                const float dx = p[1] - p[-1], dy = p[-cols] - p[cols];
                const float wgt = isxpm::pm_expf((c_rot * c_rot + r_rot * r_rot) * exp_scale);
                float obin = (si_atan2deg(dy, dx) - ori) * bins_per_rad;
                const float mag = sqrtf(dx * dx + dy * dy) * wgt;
                const float fr = floorf(rbin), fc = floorf(cbin), fo = floorf(obin);
                rbin -= fr; cbin -= fc; obin -= fo;
                const int r0 = (int)fr, c0 = (int)fc;
                int o0 = (int)fo;
                if (o0 < 0) o0 += 8;
                if (o0 >= 8) o0 -= 8;
                const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
                const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
                const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
                const float v111 = v_rc11 * obin, v110 = v_rc11 - v111;
                const float v101 = v_rc10 * obin, v100 = v_rc10 - v101;
                const float v011 = v_rc01 * obin, v010 = v_rc01 - v011;
                const float v001 = v_rc00 * obin, v000 = v_rc00 - v001;
                s_v[t][0] = v000; s_v[t][1] = v001; s_v[t][2] = v010; s_v[t][3] = v011;
                s_v[t][4] = v100; s_v[t][5] = v101; s_v[t][6] = v110; s_v[t][7] = v111;
                base = (r0 + 1) | ((c0 + 1) << 8) | (o0 << 16);
            }
        }
        s_base[t] = base;
        __syncthreads();
        if (t < SI_HIST) {
            const int m = len - k0 < SI_DESC_NT ? (int)(len - k0) : SI_DESC_NT;
            for (int kk = 0; kk < m; ++kk) {
                const int b = s_base[kk];
                if (b < 0) continue;
                const int dr = ri - (b & 255), dc = cj - ((b >> 8) & 255), dob = ok_ - (b >> 16);
                if ((unsigned)dr < 2u && (unsigned)dc < 2u && (unsigned)dob < 2u) cell += s_v[kk][(dr * 2 + dc) * 2 + dob];
            }
        }
        __syncthreads();
    }
    if (t < SI_HIST) s_hist[t] = cell;
    __syncthreads();
    if (t < 128) {
        const int i = t / 32, j = (t / 8) % 4, k = t % 8, idx = ((i + 1) * 6 + (j + 1)) * 10;
        s_dst[t] = k < 2 ? s_hist[idx + k] + s_hist[idx + 8 + k] : s_hist[idx + k];
    }
    __syncthreads();
    if (t == 0) {
        float nrm2 = 0.f;
        for (int k = 0; k < 128; ++k) nrm2 += s_dst[k] * s_dst[k];
        const float thr = sqrtf(nrm2) * 0.2f;
        nrm2 = 0.f;
        for (int k = 0; k < 128; ++k) {
            const float v = s_dst[k] < thr ? s_dst[k] : thr;
            s_dst[k] = v;
            nrm2 += v * v;
        }
        const float root = sqrtf(nrm2);
        s_hist[0] = 512.f / (root > FLT_EPSILON ? root : FLT_EPSILON);
        float* kp = (float*)((char*)O.kp + (long long)row * O.kp_step);
        float* mt = (float*)((char*)O.meta + (long long)row * O.meta_step);
        kp[0] = ptx * 0.5f; kp[1] = pty * 0.5f;
        mt[0] = size * 0.5f; mt[1] = angle; mt[2] = cand[3 * SI_MAX + ci]; mt[3] = (float)(o - 1); mt[4] = (float)l;
    }
    __syncthreads();
    if (t < 128) ((float*)((char*)O.desc + (long long)row * O.desc_step))[t] = (float)sat_u8(cvround_x86(s_dst[t] * s_hist[0]));
}

constexpr int SM_FNS = 2;
__host__ __device__ inline float sm_selftest_item(int fn, float a) { return fn == 0 ? isxpm::pm_expf(a) : isxpm::pm_exp2f(a); }
__global__ __launch_bounds__(256) void k_selftest_sift_math(int fn, int n, const float* __restrict__ in, float* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    out[i] = sm_selftest_item(fn, in[i]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
void default_params(isx_sift_params& p) { p.nfeatures = 0; p.n_octave_layers = 3; p.contrast_threshold = 0.04; p.edge_threshold = 10.0; p.sigma = 1.6; }

int check_params(const isx_sift_params* q, const char* who) {
    ISX_CHECK_ARG(q != nullptr, ISX_ERR_INVALID, "%s: null params", who);
    ISX_CHECK_ARG(q->nfeatures >= 0, ISX_ERR_INVALID, "%s: nfeatures %d is negative", who, q->nfeatures);
    ISX_CHECK_ARG(q->contrast_threshold >= 0.0 && q->contrast_threshold <= 3.0e38, ISX_ERR_INVALID, "%s: contrast_threshold %g is not in [0, 3e38]", who,
                  q->contrast_threshold);
    ISX_CHECK_ARG(q->edge_threshold > 0.0 && q->edge_threshold <= 3.0e38, ISX_ERR_INVALID, "%s: edge_threshold %g is not in (0, 3e38]", who, q->edge_threshold);
    ISX_CHECK_ARG(q->sigma == q->sigma, ISX_ERR_INVALID, "%s: sigma is not a number", who);
    ISX_CHECK_ARG(q->n_octave_layers == SI_LAYERS, ISX_ERR_UNSUPPORTED, "%s: n_octave_layers %d (3 only: the blur taps are committed tables)", who, q->n_octave_layers);
    ISX_CHECK_ARG(q->sigma == 1.6, ISX_ERR_UNSUPPORTED, "%s: sigma %g (1.6 only: the blur taps are committed tables)", who, q->sigma);
    return ISX_OK;
}

// cvRound(log(m) / log 2 - 2) + 1 in integers: the largest c with 2^(2 c + 1) <= m^2, or 0
int octave_count(int m) {
    const long long mm = (long long)m * m;
    int c = 0;
    while ((1ll << (2 * (c + 1) + 1)) <= mm) ++c;
    return (1ll << (2 * c + 1)) <= mm ? c : 0;
}

// the geometry of a W x H image: the built octaves, where their layers lie, the search workgroups
int plan_image(const isx_sift_params& q, int W, int H, const char* who, SiPlan& P) {
    ISX_CHECK_ARG(W <= ISX_SIFT_MAX_SIDE && H <= ISX_SIFT_MAX_SIDE, ISX_ERR_UNSUPPORTED, "%s: an image of %d x %d (at most %d a side)", who, W, H, ISX_SIFT_MAX_SIDE);
    ISX_CHECK_ARG((long long)W * H <= ISX_SIFT_MAX_PIXELS, ISX_ERR_UNSUPPORTED, "%s: an image of %d x %d (at most %d pixels)", who, W, H, ISX_SIFT_MAX_PIXELS);
    std::memset(&P, 0, sizeof(P));
    P.W = W; P.H = H; P.nfeatures = q.nfeatures;
    P.thr = (float)std::floor(0.5 * q.contrast_threshold / SI_LAYERS * 255.0);
    P.ct = (float)q.contrast_threshold; P.et = (float)q.edge_threshold;
    int r = 2 * H, c = 2 * W;
    const int want = octave_count(std::min(r, c));
    long long at = 0, blocks = 0;
    // the first octave's layers exist whatever the size: the base image is made in them
    for (int o = 0; o < SI_OCT && (o == 0 || (o < want && r >= 2 * SI_BORDER + 1 && c >= 2 * SI_BORDER + 1)); ++o, r /= 2, c /= 2) {
        const bool built = o < want && r >= 2 * SI_BORDER + 1 && c >= 2 * SI_BORDER + 1;
        P.rows[o] = r; P.cols[o] = c;
        P.goff[o] = at; at += (long long)SI_G * r * c;
        P.doff[o] = at; at += (long long)SI_D * r * c;
        if (!built) break;
        P.noct = o + 1;
        for (int l = 1; l <= SI_LAYERS; ++l) {
            P.blk_off[o * SI_LAYERS + l - 1] = (int)blocks;
            blocks += ((long long)(r - 2 * SI_BORDER) * (c - 2 * SI_BORDER) + 255) / 256;
        }
    }
    for (int k = P.noct * SI_LAYERS; k <= SI_OCT * SI_LAYERS; ++k) P.blk_off[k] = (int)blocks;
    P.nblocks = (int)blocks;
    P.pyr_floats = at;
    P.tmp_floats = (long long)4 * W * H;
    return ISX_OK;
}

// one buffer: [staged host image] [pyramid] [row-pass buffer] [workgroup counts | bases] [ncand, status] [candidates: floats | ints]
// [order | dup | npeaks | first] [angles] [staged host outputs]
struct SiLayout { size_t o_image, upload_bytes, o_pyr, o_tmp, o_blk_count, o_blk_base, o_ncand, o_cand, o_cand_i, o_order, o_dup, o_npeaks, o_first, o_angles; };
void lay_out(Bump& lay, const SiPlan& P, size_t image_bytes, SiLayout& o) {
    o.o_image = lay.take(image_bytes);
    o.upload_bytes = lay.at;
    o.o_pyr = lay.take((size_t)P.pyr_floats * 4);
    o.o_tmp = lay.take((size_t)P.tmp_floats * 4);
    const size_t blocks = (size_t)std::max(P.nblocks, 1);
    o.o_blk_count = lay.take(blocks * 4); o.o_blk_base = lay.take(blocks * 4);
    o.o_ncand = lay.take(8);
    o.o_cand = lay.take((size_t)4 * SI_MAX * 4); o.o_cand_i = lay.take((size_t)2 * SI_MAX * 4);
    o.o_order = lay.take((size_t)SI_MAX * 4); o.o_dup = lay.take((size_t)SI_MAX * 4); o.o_npeaks = lay.take((size_t)SI_MAX * 4); o.o_first = lay.take((size_t)SI_MAX * 4);
    o.o_angles = lay.take((size_t)SI_MAX * SI_PEAKS * 4);
}

struct SiScratch : UploadScratch {};

inline dim3 tiles(int cols, int rows) { return dim3(cdiv(cols, WAVE), cdiv(rows, 4)); }

}  // namespace

extern "C" {

int isx_sift_default_params(isx_sift_params* params) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(params != nullptr, ISX_ERR_INVALID, "sift_default_params: null params");
    default_params(*params);
    return ISX_OK;
} ISX_EXIT("isx_sift_default_params")

int isx_sift_release(void) ISX_ENTRY {
    clear_error();
    return per_thread<SiScratch>().release();
} ISX_EXIT("isx_sift_release")

int isx_sift_reserve(const isx_sift_params* params, int width, int height, int cap, int device) ISX_ENTRY {
    clear_error();
    const char* who = "sift_reserve";
    ISX_TRY(check_params(params, who));
    ISX_CHECK_ARG(width >= 1 && height >= 1, ISX_ERR_SIZE, "%s: an image of %d x %d", who, width, height);
    ISX_CHECK_ARG(cap >= 1, ISX_ERR_SIZE, "%s: outputs of %d rows", who, cap);
    SiPlan P;
    ISX_TRY(plan_image(*params, width, height, who, P));
    Bump lay;
    SiLayout o;
    lay_out(lay, P, 0, o);
    ISX_HIP(hipSetDevice(device));
    SiScratch& s = per_thread<SiScratch>();
    ISX_TRY(s.begin(device, nullptr, std::max(lay.at, s.work.cap), 0));
    return ISX_OK;
} ISX_EXIT("isx_sift_reserve")

int isx_sift_find(const isx_mat* image, const isx_sift_params* params, isx_mat* keypoints, isx_mat* meta, isx_mat* descriptors, isx_mat* count_status,
                  int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "sift_find";
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(image && keypoints && meta && descriptors && count_status, ISX_ERR_INVALID, "%s: null image, keypoints, meta, descriptors or count_status", who);
    ISX_TRY(check_params(params, who));
    ISX_CHECK_ARG(image->type == ISX_8UC1 || image->type == ISX_8UC3 || image->type == ISX_8UC4, ISX_ERR_TYPE, "%s: the image is %s (CV_8UC1, CV_8UC3 or CV_8UC4)", who,
                  type_name(image->type));
    ISX_CHECK_ARG(image->rows >= 1 && image->cols >= 1, ISX_ERR_SIZE, "%s: an image of %d x %d", who, image->cols, image->rows);
    const int cn = mat_cn(image->type), W = image->cols, H = image->rows;
    SiPlan P;
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
    ISX_TRY(check_mat_holds(*descriptors, ISX_32FC1, cap, 128, 4, STOP_NO_ROW_WANTED, device, who, "descriptors", 0));
    ISX_TRY(check_mat_holds(*count_status, ISX_32SC1, 1, 2, 4, STOP_NO_ROW_WANTED, device, who, "count_status", 0));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    bool capturing = false;
    ISX_TRY(is_capturing(st, capturing));
    const bool any_host = image->device < 0 || keypoints->device < 0 || meta->device < 0 || descriptors->device < 0 || count_status->device < 0;
    ISX_CHECK_ARG(!capturing || !any_host, ISX_ERR_STATE, "%s: the stream is capturing and a mat is a host mat (staging it synchronises)", who);

    Bump lay;
    SiLayout o;
    const size_t image_bytes = image->device < 0 ? (size_t)H * W * cn : 0;
    lay_out(lay, P, image_bytes, o);
    StagedMat m_kp, m_meta, m_desc, m_cs;
    m_kp.plan(lay, *keypoints, cap, 8);
    m_meta.plan(lay, *meta, cap, 20);
    m_desc.plan(lay, *descriptors, cap, 512);
    m_cs.plan(lay, *count_status, 1, 8);

    SiScratch& s = per_thread<SiScratch>();
    if (capturing) {
        // nothing may be allocated, uploaded or fenced inside a capture: the scratch holds the call as it is, or the call is refused
        ISX_CHECK_ARG(s.device == device && s.work.p != nullptr && s.work.cap >= lay.at, ISX_ERR_STATE,
                      "%s: the stream is capturing and the scratch would have to grow (isx_sift_reserve first)", who);
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
    float* const d_pyr = (float*)(dev + o.o_pyr);
    float* const d_tmp = (float*)(dev + o.o_tmp);
    int* const d_blk_count = (int*)(dev + o.o_blk_count);
    int* const d_blk_base = (int*)(dev + o.o_blk_base);
    int* const d_ncand = (int*)(dev + o.o_ncand);
    float* const d_cand = (float*)(dev + o.o_cand);
    int* const d_cand_i = (int*)(dev + o.o_cand_i);
    int* const d_order = (int*)(dev + o.o_order);
    int* const d_dup = (int*)(dev + o.o_dup);
    int* const d_npeaks = (int*)(dev + o.o_npeaks);
    int* const d_first = (int*)(dev + o.o_first);
    float* const d_angles = (float*)(dev + o.o_angles);
    SiOut O;
    m_kp.bind(dev, O.kp, O.kp_step);
    m_meta.bind(dev, O.meta, O.meta_step);
    m_desc.bind(dev, O.desc, O.desc_step);
    m_cs.bind(dev, O.count_status);
    O.cap = cap;
    auto gauss = [&](int oc, int l) { return d_pyr + P.goff[oc] + (long long)l * P.rows[oc] * P.cols[oc]; };
    auto dog = [&](int oc, int l) { return d_pyr + P.doff[oc] + (long long)l * P.rows[oc] * P.cols[oc]; };

    // ---- the launches ----
    const double px = 4.0 * W * H;
    const double sx = resize_scale(W, 2 * W), sy = resize_scale(H, 2 * H);
    // the doubled image goes to layer 1's place, its blur is layer 0
    if (cn == 1) ISX_LAUNCH("sift_base", px * 5, st, k_sift_base<1>, tiles(2 * W, 2 * H), dim3(256), 0, d_img, img_step, W, H, sx, sy, gauss(0, 1));
    else if (cn == 3) ISX_LAUNCH("sift_base", px * 5, st, k_sift_base<3>, tiles(2 * W, 2 * H), dim3(256), 0, d_img, img_step, W, H, sx, sy, gauss(0, 1));
    else ISX_LAUNCH("sift_base", px * 5, st, k_sift_base<4>, tiles(2 * W, 2 * H), dim3(256), 0, d_img, img_step, W, H, sx, sy, gauss(0, 1));
    ISX_LAUNCH("sift_blur_rows", px * 8, st, k_sift_blur<false>, tiles(2 * W, 2 * H), dim3(256), 0, (const float*)gauss(0, 1), d_tmp, (const float*)nullptr,
               (float*)nullptr, 2 * H, 2 * W, 0);
    ISX_LAUNCH("sift_blur_cols", px * 8, st, k_sift_blur<true>, tiles(2 * W, 2 * H), dim3(256), 0, (const float*)d_tmp, gauss(0, 0), (const float*)nullptr,
               (float*)nullptr, 2 * H, 2 * W, 0);
    for (int oc = 0; oc < P.noct; ++oc) {
        const int r = P.rows[oc], c = P.cols[oc];
        const double opx = (double)r * c;
        if (oc > 0)
            ISX_LAUNCH("sift_half", opx * 8, st, k_sift_half, tiles(c, r), dim3(256), 0, (const float*)gauss(oc - 1, SI_LAYERS), P.cols[oc - 1], gauss(oc, 0), r, c);
        for (int l = 1; l < SI_G; ++l) {
            ISX_LAUNCH("sift_blur_rows", opx * 8, st, k_sift_blur<false>, tiles(c, r), dim3(256), 0, (const float*)gauss(oc, l - 1), d_tmp, (const float*)nullptr,
                       (float*)nullptr, r, c, l);
            ISX_LAUNCH("sift_blur_cols", opx * 16, st, k_sift_blur<true>, tiles(c, r), dim3(256), 0, (const float*)d_tmp, gauss(oc, l), (const float*)gauss(oc, l - 1),
                       dog(oc, l - 1), r, c, l);
        }
    }
    const dim3 search_grid(std::max(P.nblocks, 1));
    ISX_LAUNCH("sift_extrema_count", (double)P.nblocks * 1024, st, k_sift_extrema<false>, search_grid, dim3(256), 0, P, (const float*)d_pyr, d_blk_count,
               (const int*)d_blk_base, d_cand, d_cand_i);
    ISX_LAUNCH("sift_prefix", (double)P.nblocks * 12, st, k_sift_prefix, dim3(1), dim3(SI_SCAN_NT), 0, P.nblocks, (const int*)d_blk_count, d_blk_base, d_ncand);
    ISX_LAUNCH("sift_extrema_write", (double)P.nblocks * 1024, st, k_sift_extrema<true>, search_grid, dim3(256), 0, P, (const float*)d_pyr, d_blk_count,
               (const int*)d_blk_base, d_cand, d_cand_i);
    ISX_LAUNCH("sift_rank", (double)SI_MAX * 24, st, k_sift_rank, dim3(SI_MAX / 256), dim3(256), 0, (const float*)d_cand, (const int*)d_cand_i, (const int*)d_ncand,
               d_order, d_dup);
    ISX_LAUNCH("sift_orient", (double)SI_MAX * 4096, st, k_sift_orient, dim3(SI_MAX), dim3(SI_ORI_NT), 0, P, (const float*)d_pyr, (const float*)d_cand,
               (const int*)d_cand_i, (const int*)d_ncand, (const int*)d_order, (const int*)d_dup, d_npeaks, d_angles);
    ISX_LAUNCH("sift_compact", (double)SI_MAX * 8, st, k_sift_compact, dim3(1), dim3(SI_SCAN_NT), 0, (const int*)d_ncand, (const int*)d_npeaks, d_first, P.nfeatures, O);
    const int desc_blocks = (int)std::min<long long>(cap, (long long)SI_MAX * SI_PEAKS);
    ISX_LAUNCH("sift_describe", (double)cap * 24576, st, k_sift_describe, dim3(desc_blocks), dim3(SI_DESC_NT), 0, P, (const float*)d_pyr, (const float*)d_cand,
               (const int*)d_cand_i, (const int*)d_ncand, (const int*)d_order, (const int*)d_first, (const float*)d_angles, O);
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
} ISX_EXIT("isx_sift_find")

int isx_selftest_sift_math(int fn, int n, const float* in, float* out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 0 && (n == 0 || (in && out)), ISX_ERR_INVALID, "selftest_sift_math: n %d, or null in / out", n);
    ISX_CHECK_ARG(fn >= 0 && fn < SM_FNS, ISX_ERR_INVALID, "selftest_sift_math: fn %d", fn);
    for (int i = 0; i < n; ++i) out[i] = sm_selftest_item(fn, in[i]);
    return ISX_OK;
} ISX_EXIT("isx_selftest_sift_math")

int isx_selftest_sift_math_device(int fn, int n, const float* in, float* out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 0 && (n == 0 || (in && out)), ISX_ERR_INVALID, "selftest_sift_math_device: n %d, or null in / out", n);
    ISX_CHECK_ARG(fn >= 0 && fn < SM_FNS, ISX_ERR_INVALID, "selftest_sift_math_device: fn %d", fn);
    if (n == 0) return ISX_OK;
    hipStream_t st = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    DevBuf din, dout;
    ISX_TRY(din.reserve(bytes));
    ISX_TRY(dout.reserve(bytes));
    ISX_HIP(hipMemcpyAsync(din.p, in, bytes, hipMemcpyHostToDevice, st));
    ISX_LAUNCH("selftest_sift_math", (double)bytes * 2.0, st, k_selftest_sift_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fn, n, (const float*)din.p,
               (float*)dout.p);
    ISX_HIP(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));
    return ISX_OK;
} ISX_EXIT("isx_selftest_sift_math_device")

}  // extern "C"
