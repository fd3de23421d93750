// warp_polar.hip — the fisheye and the stereographic projector (cv::FisheyeWarper B:94, cv::StereographicWarper B:95; OpenCV 3.4.x
// warpers_inl.hpp, recalled and UNPINNED) for MI355X (gfx950).
// Unlike the cylindrical, spherical and plane kinds of warp.hip nothing here is separable: atan2f, sqrtf, sinf and cosf (and atanf for the
// stereographic map) depend on both destination coordinates, so there are no column / row tables and every pixel evaluates
// proj_math.hpp's mapBackward in registers - the same text the host compiles and tests/helpers/polar_np.py restates, bit for bit.
// detectResultRoi is the base class's: mapForward of EVERY source pixel, min / max.  The device evaluates the exact u, v (not stand-ins), so
// one launch reduces them to four order-preserving keys and the host reads four floats back: no candidates, no host re-evaluation.
// These kernels are VALU-bound: the five calls run in double (half rate on CDNA4) - k_polar_build_maps is 738 VALU instructions of which
// 343 are double (static, both kinds' paths together), against two divisions and a 3 x 3 transform for the tabulated kinds.
// The polynomial paths are selects, not branches; the only divergent branches are the special values of atan2f.
#include "isx_device.hpp"
#include "isx_internal.hpp"
#include "proj_math.hpp"
#include "warp_polar.hpp"
#include "warp_sample.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

using namespace isx;
using namespace isxd;
using namespace isxpm;

namespace {

__host__ __device__ inline void polar_forward(const PolarProj& p, float x, float y, float& u, float& v) {
    if (p.kind == ISX_WARP_STEREOGRAPHIC) pm_map_forward<true>(p.r_kinv, p.scale, x, y, u, v);
    else pm_map_forward<false>(p.r_kinv, p.scale, x, y, u, v);
}
__device__ __forceinline__ void polar_backward(const PolarProj& p, int du, int dv, float& x, float& y) {
    if (p.kind == ISX_WARP_STEREOGRAPHIC) pm_map_backward<true>(p.k_rinv, p.scale, (float)du, (float)dv, x, y);
    else pm_map_backward<false>(p.k_rinv, p.scale, (float)du, (float)dv, x, y);
}

// RotationWarper::warp (W:145-161): one destination pixel per thread, 64 x 4 pixels per block
template <class T, int CN>
__global__ __launch_bounds__(256) void k_polar_warp(PolarProj p, SrcView src, unsigned char* dst, size_t dstep, int x0, int y0, int dw, int dh, int interp, int border) {
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    float mx, my;
    polar_backward(p, x0 + dx, y0 + dy, mx, my);
    T o[CN];
    if (interp == ISX_INTER_NEAREST) sample_nearest<T, CN>(src, mx, my, border, o);
    else sample_linear<T, CN>(src, mx, my, border, o, (interp & ISX_INTER_TIES_EVEN) != 0);
    T* q = (T*)(dst + (size_t)dy * dstep) + (size_t)dx * CN;
#pragma unroll
    for (int c = 0; c < CN; ++c) q[c] = o[c];
}

// W:229 + W:232 fused: image LINEAR / REFLECT and mask NEAREST / CONSTANT from one map evaluation.  OUT16: the image as CV_16SC3 (W:294).
// GAIN: GainCompensator::apply folded into the store, the 256-entry table of isx_warper_set_gain applied to the remapped byte.
struct PolarLut { unsigned v[64]; };
template <bool OUT16, bool GAIN>
__global__ __launch_bounds__(256) void k_polar_warp_img_mask(PolarProj p, SrcView img, SrcView msk, int has_mask, PolarLut lut, unsigned char* dimg, size_t dimg_step,
                                                             unsigned char* dmask, size_t dmask_step, int x0, int y0, int dw, int dh) {
    __shared__ unsigned char s_lut[GAIN ? 256 : 4];
    if constexpr (GAIN) {      // before any thread leaves: everyone reaches the barrier
        if (threadIdx.x < 64) ((unsigned*)s_lut)[threadIdx.x] = lut.v[threadIdx.x];
        __syncthreads();
    }
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    float mx, my;
    polar_backward(p, x0 + dx, y0 + dy, mx, my);
    unsigned char o[3];
    sample_linear<unsigned char, 3>(img, mx, my, ISX_BORDER_REFLECT, o);
    unsigned char m;
    if (has_mask) sample_nearest<unsigned char, 1>(msk, mx, my, ISX_BORDER_CONSTANT, &m);
    else {      // masks[i].setTo(255) (W:213-214) warped NEAREST / CONSTANT: 255 iff cvRound(x) in [0, cols) and cvRound(y) in [0, rows)
        const int nx = clamp_short(cvround_x86(mx)), ny = clamp_short(cvround_x86(my));
        m = ((unsigned)nx < (unsigned)img.cols && (unsigned)ny < (unsigned)img.rows) ? 255 : 0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v = o[c];
        if constexpr (GAIN) v = s_lut[v];
        if constexpr (OUT16) ((short*)(dimg + (size_t)dy * dimg_step))[(size_t)dx * 3 + c] = (short)v;
        else (dimg + (size_t)dy * dimg_step)[(size_t)dx * 3 + c] = (unsigned char)v;
    }
    dmask[(size_t)dy * dmask_step + dx] = m;
}

// buildMaps (W:133-141)
__global__ __launch_bounds__(256) void k_polar_build_maps(PolarProj p, float* xmap, size_t xstep, float* ymap, size_t ystep, int x0, int y0, int dw, int dh) {
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    float mx, my;
    polar_backward(p, x0 + dx, y0 + dy, mx, my);
    ((float*)((char*)xmap + (size_t)dy * xstep))[dx] = mx;
    ((float*)((char*)ymap + (size_t)dy * ystep))[dx] = my;
}

// order-preserving float -> uint key for atomicMin / atomicMax (warp.hip's fkey; fkey_inv is the host's there)
__device__ __forceinline__ unsigned fkey(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// detectResultRoi (W:64-88): one block scans a band of POLAR_ROI_ROWS rows of a 256-column strip, reduces its four extrema through shuffles
// and LDS, and touches the four global keys once (a few hundred same-address atomics per scan, as k_roi_scan's)
constexpr int POLAR_ROI_ROWS = 16;
__global__ __launch_bounds__(256) void k_polar_roi_scan(PolarProj p, int sw, int sh, unsigned* keys) {
    __shared__ float red[4][4];
    float tl_u = FLT_MAX, tl_v = FLT_MAX, br_u = -FLT_MAX, br_v = -FLT_MAX;      // W:66-69
    const int y0 = blockIdx.y * POLAR_ROI_ROWS, y1 = min(y0 + POLAR_ROI_ROWS, sh);
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < sw) {
        for (int y = y0; y < y1; ++y) {
            float u, v;
            polar_forward(p, (float)x, (float)y, u, v);
            tl_u = (u < tl_u) ? u : tl_u; tl_v = (v < tl_v) ? v : tl_v;     // (std::min)(tl, u): a NaN never replaces a value  W:77-78
            br_u = (br_u < u) ? u : br_u; br_v = (br_v < v) ? v : br_v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {      // (no NaN in here: the four start finite and a NaN never got in)
        tl_u = fminf(tl_u, __shfl_xor(tl_u, o)); tl_v = fminf(tl_v, __shfl_xor(tl_v, o));
        br_u = fmaxf(br_u, __shfl_xor(br_u, o)); br_v = fmaxf(br_v, __shfl_xor(br_v, o));
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wv] = tl_u; red[1][wv] = tl_v; red[2][wv] = br_u; red[3][wv] = br_v; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        const float a = red[k][0], b = red[k][1], c = red[k][2], d = red[k][3];
        if (k < 2) {
            const unsigned key = fkey(fminf(fminf(a, b), fminf(c, d)));
            if (key < __hip_atomic_load(&keys[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&keys[k], key);
        } else {
            const unsigned key = fkey(fmaxf(fmaxf(a, b), fmaxf(c, d)));
            if (key > __hip_atomic_load(&keys[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&keys[k], key);
        }
    }
}

// ---- the self-test of proj_math.hpp: item i of function fn, by the host's loop and by a thread ------------------------------------------------
constexpr int PM_FNS = 5;
__host__ __device__ inline float pm_selftest_item(int fn, float a, float b) {
    switch (fn) {
    case 0: return pm_sinf(a);
    case 1: return pm_cosf(a);
    case 2: return pm_atan2f(a, b);
    case 3: return pm_atanf(a);
    default: return pm_acosf(a);
    }
}
__global__ __launch_bounds__(256) void k_selftest_proj_math(int fn, int n, const float* __restrict__ in, const float* __restrict__ in2, float* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    out[i] = pm_selftest_item(fn, in[i], in2 ? in2[i] : 0.f);
}

inline int f2i_host(float v) { return (std::fabs(v) < 2147483648.0f) ? (int)v : INT_MIN; }
inline SrcView view(const PolarSrc& s) { return SrcView{s.data, s.step, s.rows, s.cols}; }

}  // namespace

namespace isx {

void polar_map_forward_host(const PolarProj& p, float x, float y, float& u, float& v) { polar_forward(p, x, y, u, v); }

void polar_roi_host(const PolarProj& p, int sw, int sh, int roi[4], float mm[4]) {
    float tl_u = FLT_MAX, tl_v = FLT_MAX, br_u = -FLT_MAX, br_v = -FLT_MAX;
    for (int y = 0; y < sh; ++y)
        for (int x = 0; x < sw; ++x) {
            float u, v;
            polar_forward(p, (float)x, (float)y, u, v);
            tl_u = (std::min)(tl_u, u); tl_v = (std::min)(tl_v, v);
            br_u = (std::max)(br_u, u); br_v = (std::max)(br_v, v);
        }
    if (mm) { mm[0] = tl_u; mm[1] = tl_v; mm[2] = br_u; mm[3] = br_v; }
    roi[0] = f2i_host(tl_u); roi[1] = f2i_host(tl_v); roi[2] = f2i_host(br_u); roi[3] = f2i_host(br_v);
}

int polar_launch_warp(hipStream_t st, const PolarProj& p, int type, double bytes, const PolarSrc& src, unsigned char* dst, size_t dstep, int x0, int y0, int dw, int dh,
                      int interp, int border) {
    if (type != ISX_8UC1 && type != ISX_8UC3 && type != ISX_32FC1 && type != ISX_32FC3)
        return fail(ISX_ERR_TYPE, "warp: src type %s is not supported (CV_8UC1/3, CV_32FC1/3)", type_name(type));
    const dim3 grid(cdiv(dw, 64), cdiv(dh, 4));
    const SrcView sv = view(src);
    if (type == ISX_8UC1) ISX_LAUNCH("polar_warp", bytes, st, (k_polar_warp<unsigned char, 1>), grid, dim3(256), 0, p, sv, dst, dstep, x0, y0, dw, dh, interp, border);
    else if (type == ISX_8UC3) ISX_LAUNCH("polar_warp", bytes, st, (k_polar_warp<unsigned char, 3>), grid, dim3(256), 0, p, sv, dst, dstep, x0, y0, dw, dh, interp, border);
    else if (type == ISX_32FC1) ISX_LAUNCH("polar_warp", bytes, st, (k_polar_warp<float, 1>), grid, dim3(256), 0, p, sv, dst, dstep, x0, y0, dw, dh, interp, border);
    else ISX_LAUNCH("polar_warp", bytes, st, (k_polar_warp<float, 3>), grid, dim3(256), 0, p, sv, dst, dstep, x0, y0, dw, dh, interp, border);
    return ISX_OK;
}

int polar_launch_warp_img_mask(hipStream_t st, const PolarProj& p, bool out16, double bytes, const PolarSrc& img, const PolarSrc& msk, const unsigned char* lut,
                               const isx_mat& dimg, const isx_mat& dmask, int x0, int y0, int dw, int dh) {
    const dim3 grid(cdiv(dw, 64), cdiv(dh, 4));
    const SrcView iv = view(img), mv = view(msk);
    const int has_mask = msk.data ? 1 : 0;
    PolarLut pl;
    memset(&pl, 0, sizeof(pl));
    if (lut) memcpy(pl.v, lut, 256);
    unsigned char* di = (unsigned char*)dimg.data;
    unsigned char* dm = (unsigned char*)dmask.data;
    if (out16) {
        if (lut) ISX_LAUNCH("polar_warp_img_mask", bytes, st, (k_polar_warp_img_mask<true, true>), grid, dim3(256), 0, p, iv, mv, has_mask, pl, di, dimg.step, dm, dmask.step, x0, y0, dw, dh);
        else ISX_LAUNCH("polar_warp_img_mask", bytes, st, (k_polar_warp_img_mask<true, false>), grid, dim3(256), 0, p, iv, mv, has_mask, pl, di, dimg.step, dm, dmask.step, x0, y0, dw, dh);
    } else {
        if (lut) ISX_LAUNCH("polar_warp_img_mask", bytes, st, (k_polar_warp_img_mask<false, true>), grid, dim3(256), 0, p, iv, mv, has_mask, pl, di, dimg.step, dm, dmask.step, x0, y0, dw, dh);
        else ISX_LAUNCH("polar_warp_img_mask", bytes, st, (k_polar_warp_img_mask<false, false>), grid, dim3(256), 0, p, iv, mv, has_mask, pl, di, dimg.step, dm, dmask.step, x0, y0, dw, dh);
    }
    return ISX_OK;
}

int polar_launch_build_maps(hipStream_t st, const PolarProj& p, const isx_mat& xmap, const isx_mat& ymap, int x0, int y0, int dw, int dh) {
    const dim3 grid(cdiv(dw, 64), cdiv(dh, 4));
    ISX_LAUNCH("polar_build_maps", (double)dw * dh * 8.0, st, k_polar_build_maps, grid, dim3(256), 0, p, (float*)xmap.data, xmap.step, (float*)ymap.data, ymap.step, x0, y0, dw, dh);
    return ISX_OK;
}

int polar_launch_roi_scan(hipStream_t st, const PolarProj& p, int sw, int sh, unsigned* keys) {
    const dim3 grid(cdiv(sw, 256), cdiv(sh, POLAR_ROI_ROWS));
    ISX_LAUNCH("polar_roi_scan", 0.0, st, k_polar_roi_scan, grid, dim3(256), 0, p, sw, sh, keys);
    return ISX_OK;
}

}  // namespace isx

extern "C" {

int isx_selftest_proj_math(int fn, int n, const float* in, const float* in2, float* out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 0 && (n == 0 || (in && out)), ISX_ERR_INVALID, "selftest_proj_math: n %d, or null in / out", n);
    ISX_CHECK_ARG(fn >= 0 && fn < PM_FNS && (fn != 2 || n == 0 || in2), ISX_ERR_INVALID, "selftest_proj_math: fn %d (atan2f takes in2)", fn);
    for (int i = 0; i < n; ++i) out[i] = pm_selftest_item(fn, in[i], in2 ? in2[i] : 0.f);
    return ISX_OK;
} ISX_EXIT("isx_selftest_proj_math")

int isx_selftest_proj_math_device(int fn, int n, const float* in, const float* in2, float* out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 0 && (n == 0 || (in && out)), ISX_ERR_INVALID, "selftest_proj_math_device: n %d, or null in / out", n);
    ISX_CHECK_ARG(fn >= 0 && fn < PM_FNS && (fn != 2 || n == 0 || in2), ISX_ERR_INVALID, "selftest_proj_math_device: fn %d (atan2f takes in2)", fn);
    if (n == 0) return ISX_OK;
    hipStream_t st = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    DevBuf din, din2, dout;
    ISX_TRY(din.reserve(bytes));
    ISX_TRY(dout.reserve(bytes));
    ISX_HIP(hipMemcpyAsync(din.p, in, bytes, hipMemcpyHostToDevice, st));
    if (in2) {
        ISX_TRY(din2.reserve(bytes));
        ISX_HIP(hipMemcpyAsync(din2.p, in2, bytes, hipMemcpyHostToDevice, st));
    }
    ISX_LAUNCH("selftest_proj_math", (double)bytes * 3.0, st, k_selftest_proj_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fn, n, (const float*)din.p,
               (const float*)(in2 ? din2.p : nullptr), (float*)dout.p);
    ISX_HIP(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));
    return ISX_OK;
} ISX_EXIT("isx_selftest_proj_math_device")

}  // extern "C"
