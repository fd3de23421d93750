// resize.hip — seam finding at reduced scale (OpenCV's stitching_detailed / Stitcher::composePanorama around W:264-302) on gfx950:
//   isx_resize                  cv::resize(src, dst, dst.size(), 0, 0, INTER_NEAREST | INTER_LINEAR) on CV_8U / CV_32F, 1 or 3 channels
//   isx_mask_dilate_resize_and  resize(dilate(seam_mask, MORPH_RECT kw x kh), out.size(), INTER_LINEAR) & warped_mask in one launch
// Restated from OpenCV 3.4.2 imgproc/src/resize.cpp, plain C++ path (tests/helpers/resize_np.py is the model).  The taps are
// resize_taps.hpp's, computed per pixel in the kernel from the two scales the host passes: no table, no upload, nothing a capture rejects.
// Both kernels are byte-bound: a lane owns four adjacent output pixels of a row and stores them as whole dwords, no LDS.
#include "isx_device.hpp"
#include "isx_internal.hpp"
#include "scratch.hpp"
#include "resize_taps.hpp"

#include <algorithm>
#include <cstdint>

using namespace isx;
using namespace isxd;

namespace {

constexpr int RZ_PX = 4;                   // output pixels per lane; a wave covers 256 pixels of one row, a workgroup of 4 waves 4 rows
enum { RZ_NEAREST = 0, RZ_LINEAR = 1, RZ_HALF = 2 };   // RZ_HALF: INTER_LINEAR with src = 2 dst in both directions, OpenCV's 2 x 2 area rule

// one element of a row that may start at any byte
template <class T> struct Unaligned { typedef T type __attribute__((aligned(1))); };
typedef unsigned u32u __attribute__((aligned(1)));
typedef unsigned u32x3u __attribute__((ext_vector_type(3), aligned(1)));
typedef unsigned u32x4u __attribute__((ext_vector_type(4), aligned(1)));
template <class T> __device__ __forceinline__ T ld(const unsigned char* row, int i) { return ((const typename Unaligned<T>::type*)row)[i]; }

// INTER_LINEAR on one channel value: CV_8U in 11-bit fixed point, CV_32F in floats (a multiply, then an add)
__device__ __forceinline__ unsigned char lin(const unsigned char* r0, const unsigned char* r1, int i0, int i1, bool two, float fx, float fy, unsigned char) {
    const int a0 = resize_coef(1.f - fx), a1 = resize_coef(fx), b0 = resize_coef(1.f - fy), b1 = resize_coef(fy);
    (void)two;                             // a1 = 0 where no tap lies to the right, and i1 = i0 there
    const int h0 = (int)r0[i0] * a0 + (int)r0[i1] * a1, h1 = (int)r1[i0] * a0 + (int)r1[i1] * a1;
    return (unsigned char)resize_vert_u8(h0, h1, b0, b1);
}
__device__ __forceinline__ float lin(const unsigned char* r0, const unsigned char* r1, int i0, int i1, bool two, float fx, float fy, float) {
    const float a0 = 1.f - fx;
    const float h0 = two ? ld<float>(r0, i0) * a0 + ld<float>(r0, i1) * fx : ld<float>(r0, i0);
    const float h1 = two ? ld<float>(r1, i0) * a0 + ld<float>(r1, i1) * fx : ld<float>(r1, i0);
    return h0 * (1.f - fy) + h1 * fy;
}
// the 2 x 2 area rule: (a + b + c + d + 2) >> 2, and (((a + b) + c) + d) * 0.25f in the order (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)
__device__ __forceinline__ unsigned char half2(const unsigned char* r0, const unsigned char* r1, int i0, int i1, unsigned char) {
    return (unsigned char)(((int)r0[i0] + (int)r0[i1] + (int)r1[i0] + (int)r1[i1] + 2) >> 2);
}
__device__ __forceinline__ float half2(const unsigned char* r0, const unsigned char* r1, int i0, int i1, float) {
    return (((ld<float>(r0, i0) + ld<float>(r0, i1)) + ld<float>(r1, i0)) + ld<float>(r1, i1)) * 0.25f;
}

template <class T, int CN, int MODE>
__global__ __launch_bounds__(256) void k_resize(const unsigned char* __restrict__ src, size_t sstep, int sw, int sh, unsigned char* __restrict__ dst, size_t dstep,
                                                int dw, int dh, double scale_x, double scale_y) {
    const int x = ((int)blockIdx.x * WAVE + (int)(threadIdx.x & (WAVE - 1))) * RZ_PX;
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x / WAVE);
    if (x >= dw || y >= dh) return;
    const int np = min(RZ_PX, dw - x);     // pixels of this group inside the row
    // the two source rows (one for NEAREST)
    int sy0, sy1;
    float fy = 0.f;
    if constexpr (MODE == RZ_NEAREST) sy0 = sy1 = nearest_tap(y, scale_y, sh);
    else if constexpr (MODE == RZ_HALF) { sy0 = 2 * y; sy1 = 2 * y + 1; }
    else { const RowTap q = row_tap(y, scale_y, sh); sy0 = q.sy0; sy1 = q.sy1; fy = q.fy; }
    const unsigned char* r0 = src + (size_t)sy0 * sstep;
    const unsigned char* r1 = src + (size_t)sy1 * sstep;
    T o[RZ_PX * CN];
#pragma unroll
    for (int k = 0; k < RZ_PX; ++k) {
        const int dx = min(x + k, dw - 1);                 // (a partial group computes its last pixel again and does not store it)
        int sx, sx1;
        float fx = 0.f;
        if constexpr (MODE == RZ_NEAREST) sx = sx1 = nearest_tap(dx, scale_x, sw);
        else if constexpr (MODE == RZ_HALF) { sx = 2 * dx; sx1 = 2 * dx + 1; }
        else { const ColTap t = col_tap(dx, scale_x, sw); sx = t.sx; sx1 = min(t.sx + 1, sw - 1); fx = t.a1; }
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            if constexpr (MODE == RZ_NEAREST) o[k * CN + c] = ld<T>(r0, sx * CN + c);
            else if constexpr (MODE == RZ_HALF) o[k * CN + c] = half2(r0, r1, sx * CN + c, sx1 * CN + c, T());
            else o[k * CN + c] = lin(r0, r1, sx * CN + c, sx1 * CN + c, sx1 != sx, fx, fy, T());
        }
    }
    // four pixels = CN dwords of bytes or 4 CN floats, stored whole at whatever alignment the row has; a row's last, partial group value by value
    unsigned char* dp = dst + (size_t)y * dstep + (size_t)x * CN * sizeof(T);
    if (np == RZ_PX) {
        constexpr int NW = CN * (int)sizeof(T);            // dwords of the group: 1, 3, 4 or 12
        unsigned w[NW];
        if constexpr (sizeof(T) == 1) {
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = (unsigned)o[4 * i] | ((unsigned)o[4 * i + 1] << 8) | ((unsigned)o[4 * i + 2] << 16) | ((unsigned)o[4 * i + 3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = __float_as_uint(o[i]);
        }
        if constexpr (NW == 1) *(u32u*)dp = w[0];
        else if constexpr (NW == 3) *(u32x3u*)dp = (u32x3u){w[0], w[1], w[2]};
        else {
#pragma unroll
            for (int i = 0; i < NW; i += 4) *(u32x4u*)(dp + 4 * i) = (u32x4u){w[i], w[i + 1], w[i + 2], w[i + 3]};
        }
    } else {
        for (int k = 0; k < np * CN; ++k) ((typename Unaligned<T>::type*)dp)[k] = o[k];
    }
}

// ---- resize(dilate(seam, kw x kh), out.size(), INTER_LINEAR) & warped ------------------------------------------------------------------------
// A lane owns 4 adjacent pixels of DR_ROWS adjacent output rows.  An output pixel takes the (at most) 2 x 2 taps (sy0 | sy1) x (sx | sx + 1) of the
// dilated small mask; a tap is the maximum of the small mask over [s - k / 2, s - k / 2 + k) cut to the image (isx_mask_dilate_and's anchor and
// border rule).  The four taps of a pixel are reduced together - every row of the (kh + 1) x (kw + 1) neighbourhood is read once for the two
// column windows and goes into the row windows it lies in - and kept while the next pixel or the next row asks for the same taps, which at
// the scales this stage runs at (a 0.1 Mpix mask to a 4K tile: 9 output pixels per tap) is most of the time.  The small mask stays in cache.
// dilated_taps is the form for any element; dilated_taps3 below is the 3 x 3 one.
constexpr int DR_ROWS = 4;

struct Taps4 { int d00, d01, d10, d11; };          // dilated (sy0, sx), (sy0, sx1), (sy1, sx), (sy1, sx1)
__device__ __forceinline__ Taps4 dilated_taps(const unsigned char* __restrict__ m, size_t step, int mw, int mh, int kw, int kh, int sy0, int sy1, int sx, int sx1) {
    const int ax = kw / 2, ay = kh / 2;
    const int xl0 = sx - ax, xr0 = sx1 - ax;                                   // the two column windows [x0, x0 + kw)
    const int xa = max(xl0, 0), xb = min(xr0 + kw, mw);                        // their union inside the image (sx <= sx1 <= sx + 1)
    const int ya = max(sy0 - ay, 0), yb = min(sy1 - ay + kh, mh);              // the row windows' union (sy0 <= sy1 <= sy0 + 1)
    Taps4 t{0, 0, 0, 0};
    for (int y = ya; y < yb; ++y) {
        const unsigned char* r = m + (size_t)y * step;
        int hl = 0, hr = 0;
        for (int x = xa; x < xb; ++x) {
            const int v = r[x];
            if (x < xl0 + kw) hl = max(hl, v);
            if (x >= xr0) hr = max(hr, v);
        }
        if (y < sy0 - ay + kh) { t.d00 = max(t.d00, hl); t.d01 = max(t.d01, hr); }
        if (y >= sy1 - ay) { t.d10 = max(t.d10, hl); t.d11 = max(t.d11, hr); }
    }
    return t;
}

// The 3 x 3 element (dilate(.., Mat()), what the compose loop runs): the four taps' windows lie in the 4 x 4 pixels around (sy0, sx), read as one
// unaligned dword per row where the four columns are inside the row and pixel by pixel at the image's sides.  Rows and columns outside
// the image are replaced by the nearest one inside, which is inside the same window and leaves its maximum as it is.  Where sx1 == sx (the
// last column; its coefficient is 0) the right taps are not those of a window and are not used.
__device__ __forceinline__ Taps4 dilated_taps3(const unsigned char* __restrict__ m, size_t step, int mw, int mh, int sy0, int sy1, int sx) {
    int hl[4], hr[4];
    const bool whole = sx >= 1 && sx + 2 < mw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned char* r = m + (size_t)min(max(sy0 - 1 + i, 0), mh - 1) * step;
        unsigned w;
        if (whole) w = *(const u32u*)(r + sx - 1);
        else w = (unsigned)r[max(sx - 1, 0)] | ((unsigned)r[sx] << 8) | ((unsigned)r[min(sx + 1, mw - 1)] << 16) | ((unsigned)r[min(sx + 2, mw - 1)] << 24);
        const int b0 = (int)(w & 255u), b1 = (int)((w >> 8) & 255u), b2 = (int)((w >> 16) & 255u), b3 = (int)(w >> 24);
        hl[i] = max(max(b0, b1), b2);
        hr[i] = max(max(b1, b2), b3);
    }
    Taps4 t;
    t.d00 = max(max(hl[0], hl[1]), hl[2]);
    t.d01 = max(max(hr[0], hr[1]), hr[2]);
    const bool same = sy1 == sy0;                                              // both row indices clamped to one row: one window
    t.d10 = same ? t.d00 : max(max(hl[1], hl[2]), hl[3]);
    t.d11 = same ? t.d01 : max(max(hr[1], hr[2]), hr[3]);
    return t;
}

template <bool HALF, bool K3>
__global__ __launch_bounds__(256) void k_dilate_resize_and(const unsigned char* __restrict__ m, size_t mstep, int mw, int mh, int kw, int kh,
                                                           const unsigned char* other, size_t ostep, unsigned char* dst, size_t dstep,   // (out may be the warped mask itself)
                                                           int dw, int dh, double scale_x, double scale_y) {
    const int x = ((int)blockIdx.x * WAVE + (int)(threadIdx.x & (WAVE - 1))) * RZ_PX;
    const int y0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x / WAVE)) * DR_ROWS;
    if (x >= dw || y0 >= dh) return;
    const int np = min(RZ_PX, dw - x);
    const int nr = min(DR_ROWS, dh - y0);
    int sx[RZ_PX], sx1[RZ_PX], a0[RZ_PX], a1[RZ_PX];
#pragma unroll
    for (int k = 0; k < RZ_PX; ++k) {
        const int dx = min(x + k, dw - 1);
        if constexpr (HALF) { sx[k] = 2 * dx; sx1[k] = 2 * dx + 1; a0[k] = a1[k] = 0; }
        else {
            const ColTap t = col_tap(dx, scale_x, mw);
            sx[k] = t.sx; sx1[k] = min(t.sx + 1, mw - 1);
            a0[k] = resize_coef(1.f - t.a1); a1[k] = resize_coef(t.a1);
        }
    }
    int sy0 = -1, sy1 = -1;
    Taps4 t[RZ_PX];
#pragma unroll
    for (int r = 0; r < DR_ROWS; ++r) {
        if (r >= nr) break;
        const int y = y0 + r;
        int qy0, qy1, b0 = 0, b1 = 0;
        if constexpr (HALF) { qy0 = 2 * y; qy1 = 2 * y + 1; }
        else { const RowTap q = row_tap(y, scale_y, mh); qy0 = q.sy0; qy1 = q.sy1; b0 = resize_coef(1.f - q.fy); b1 = resize_coef(q.fy); }
        if (qy0 != sy0 || qy1 != sy1) {            // uniform over the wave: a row is a wave's
            sy0 = qy0; sy1 = qy1;
#pragma unroll
            for (int k = 0; k < RZ_PX; ++k) {
                if (k > 0 && sx[k] == sx[k - 1] && sx1[k] == sx1[k - 1]) t[k] = t[k - 1];
                else if constexpr (K3) t[k] = dilated_taps3(m, mstep, mw, mh, sy0, sy1, sx[k]);
                else t[k] = dilated_taps(m, mstep, mw, mh, kw, kh, sy0, sy1, sx[k], sx1[k]);
            }
        }
        unsigned o = 0;
#pragma unroll
        for (int k = 0; k < RZ_PX; ++k) {
            int v;
            if constexpr (HALF) v = (t[k].d00 + t[k].d01 + t[k].d10 + t[k].d11 + 2) >> 2;
            else v = resize_vert_u8(t[k].d00 * a0[k] + t[k].d01 * a1[k], t[k].d10 * a0[k] + t[k].d11 * a1[k], b0, b1);
            o |= (unsigned)v << (8 * k);
        }
        unsigned char* dp = dst + (size_t)y * dstep + x;
        const unsigned char* op = other ? other + (size_t)y * ostep + x : nullptr;
        if (np == RZ_PX) {
            if (op) o &= *(const u32u*)op;
            *(u32u*)dp = o;
        } else {
            for (int k = 0; k < np; ++k) {
                unsigned v = (o >> (8 * k)) & 255u;
                if (op) v &= op[k];
                dp[k] = (unsigned char)v;
            }
        }
    }
}

// nothing may synchronise on a capturing stream, and staging a host mat does
int no_host_mats_while_capturing(hipStream_t st, bool any_host, const char* who) {
    bool capturing = false;
    ISX_TRY(is_capturing(st, capturing));
    ISX_CHECK_ARG(!capturing || !any_host, ISX_ERR_STATE, "%s: the stream is capturing and a mat is a host mat (staging it synchronises)", who);
    return ISX_OK;
}
int not_empty(const isx_mat* m, const char* what) {
    ISX_CHECK_ARG(m != nullptr, ISX_ERR_INVALID, "%s: null isx_mat", what);
    ISX_CHECK_ARG(m->rows > 0 && m->cols > 0, ISX_ERR_SIZE, "%s: empty mat (%d x %d)", what, m->cols, m->rows);
    return check_mat(m, what);
}
// the launch grids count rows in 16 bits, and the byte offsets inside a row are ints
constexpr int RZ_MAX_ROWS = 4 * 65535, RZ_MAX_COLS = 1 << 26;

// Both kernels read neighbours of the pixel they write, so an output that lies over an input races.  A mat's bytes are taken as the one range
// [data, data + (rows - 1) step + cols elemSize): two views whose rows interleave inside one buffer (side by side) count as sharing, views one
// after the other do not.  Mats in different memories (host / device, two devices) share nothing.
bool share_a_byte(const isx_mat* a, const isx_mat* b) {
    if ((a->device < 0) != (b->device < 0) || (a->device >= 0 && a->device != b->device)) return false;
    const uintptr_t a0 = (uintptr_t)a->data, a1 = a0 + (size_t)(a->rows - 1) * a->step + (size_t)a->cols * mat_elem_size(a->type);
    const uintptr_t b0 = (uintptr_t)b->data, b1 = b0 + (size_t)(b->rows - 1) * b->step + (size_t)b->cols * mat_elem_size(b->type);
    return a0 < b1 && b0 < a1;
}
// one view of one memory: every pixel at the same address (the pitch of a single row addresses nothing)
bool same_view(const isx_mat* a, const isx_mat* b) {
    return a->data == b->data && a->device == b->device && a->rows == b->rows && a->cols == b->cols && a->type == b->type && (a->step == b->step || a->rows == 1);
}

template <class T, int CN>
int launch_resize(int mode, const isx_mat& s, const isx_mat& d, hipStream_t st) {
    const double bytes = ((double)d.rows * d.cols + (mode == RZ_NEAREST ? (double)d.rows * d.cols : (double)s.rows * s.cols)) * CN * sizeof(T);
    const dim3 grid(cdiv(cdiv(d.cols, RZ_PX), WAVE), cdiv(d.rows, 4));
    const double scale_x = resize_scale(s.cols, d.cols), scale_y = resize_scale(s.rows, d.rows);
#define ISX_RZ(M) ISX_LAUNCH("resize", bytes, st, (k_resize<T, CN, M>), grid, dim3(256), 0, (const unsigned char*)s.data, s.step, s.cols, s.rows, \
                             (unsigned char*)d.data, d.step, d.cols, d.rows, scale_x, scale_y)
    if (mode == RZ_NEAREST) ISX_RZ(RZ_NEAREST);
    else if (mode == RZ_HALF) ISX_RZ(RZ_HALF);
    else ISX_RZ(RZ_LINEAR);
#undef ISX_RZ
    return ISX_OK;
}

}  // namespace

extern "C" {

int isx_resize(const isx_mat* src, isx_mat* dst, int interpolation, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    ISX_TRY(not_empty(src, "resize: src"));
    ISX_TRY(not_empty(dst, "resize: dst"));
    ISX_CHECK_ARG(interpolation == ISX_INTER_NEAREST || interpolation == ISX_INTER_LINEAR, ISX_ERR_UNSUPPORTED,
                  "resize: interpolation %d (INTER_NEAREST and INTER_LINEAR)", interpolation);
    ISX_CHECK_ARG(src->type == ISX_8UC1 || src->type == ISX_8UC3 || src->type == ISX_32FC1 || src->type == ISX_32FC3, ISX_ERR_UNSUPPORTED,
                  "resize: %s (CV_8UC1, CV_8UC3, CV_32FC1 and CV_32FC3)", type_name(src->type));
    ISX_CHECK_ARG(dst->type == src->type, ISX_ERR_TYPE, "resize: dst is %s, src is %s", type_name(dst->type), type_name(src->type));
    ISX_CHECK_ARG(std::max(src->rows, dst->rows) <= RZ_MAX_ROWS && std::max(src->cols, dst->cols) <= RZ_MAX_COLS, ISX_ERR_UNSUPPORTED,
                  "resize: %d x %d -> %d x %d passes %d rows or %d columns", src->cols, src->rows, dst->cols, dst->rows, RZ_MAX_ROWS, RZ_MAX_COLS);
    ISX_CHECK_ARG(!share_a_byte(src, dst), ISX_ERR_INVALID, "resize: dst shares bytes with src (the kernel reads the neighbours of the pixel it writes)");
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool any_host = src->device < 0 || dst->device < 0;
    ISX_TRY(no_host_mats_while_capturing(st, any_host, "resize"));
    MatStage si, so;
    ISX_TRY(si.use_in(src, st, "resize: src"));
    ISX_TRY(so.use_out(dst, st, "resize: dst"));
    int mode = interpolation == ISX_INTER_NEAREST ? RZ_NEAREST : RZ_LINEAR;
    if (mode == RZ_LINEAR && src->cols == 2 * dst->cols && src->rows == 2 * dst->rows) mode = RZ_HALF;
    if (src->type == ISX_8UC1) ISX_TRY((launch_resize<unsigned char, 1>(mode, si.d, so.d, st)));
    else if (src->type == ISX_8UC3) ISX_TRY((launch_resize<unsigned char, 3>(mode, si.d, so.d, st)));
    else if (src->type == ISX_32FC1) ISX_TRY((launch_resize<float, 1>(mode, si.d, so.d, st)));
    else ISX_TRY((launch_resize<float, 3>(mode, si.d, so.d, st)));
    ISX_TRY(so.finish_out(st));
    if (any_host) ISX_HIP(hipStreamSynchronize(st));   // the staging buffers are freed on return
    return ISX_OK;
} ISX_EXIT("isx_resize")

int isx_mask_dilate_resize_and(const isx_mat* seam_mask, const isx_mat* warped_mask, int kw, int kh, isx_mat* out, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "dilate_resize_and";
    ISX_TRY(not_empty(seam_mask, "dilate_resize_and: seam_mask"));
    ISX_TRY(not_empty(out, "dilate_resize_and: out"));
    ISX_CHECK_ARG(seam_mask->type == ISX_8UC1 && out->type == ISX_8UC1, ISX_ERR_TYPE, "%s: masks must be CV_8U", who);
    ISX_CHECK_ARG(kw >= 1 && kh >= 1 && kw <= 4096 && kh <= 4096, ISX_ERR_INVALID, "%s: bad structuring element %dx%d", who, kw, kh);
    if (warped_mask) {
        ISX_TRY(not_empty(warped_mask, "dilate_resize_and: warped_mask"));
        ISX_CHECK_ARG(warped_mask->type == ISX_8UC1 && warped_mask->rows == out->rows && warped_mask->cols == out->cols, ISX_ERR_SIZE,
                      "%s: the AND operand must be a CV_8U mask of out's size (%d x %d)", who, out->cols, out->rows);
    }
    ISX_CHECK_ARG(std::max(seam_mask->rows, out->rows) <= RZ_MAX_ROWS && std::max(seam_mask->cols, out->cols) <= RZ_MAX_COLS, ISX_ERR_UNSUPPORTED,
                  "%s: %d x %d -> %d x %d passes %d rows or %d columns", who, seam_mask->cols, seam_mask->rows, out->cols, out->rows, RZ_MAX_ROWS, RZ_MAX_COLS);
    ISX_CHECK_ARG(!share_a_byte(seam_mask, out), ISX_ERR_INVALID, "%s: out shares bytes with seam_mask (the kernel reads the neighbours of the pixel it writes)", who);
    // a lane reads the dword of warped_mask that it then writes: the same view is safe, a shifted one is not
    ISX_CHECK_ARG(!warped_mask || same_view(warped_mask, out) || !share_a_byte(warped_mask, out), ISX_ERR_INVALID,
                  "%s: out shares bytes with warped_mask and is not the same view of it (same data, step and size)", who);
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool any_host = seam_mask->device < 0 || out->device < 0 || (warped_mask && warped_mask->device < 0);
    ISX_TRY(no_host_mats_while_capturing(st, any_host, who));
    MatStage sm, sw, sd;
    ISX_TRY(sm.use_in(seam_mask, st, "dilate_resize_and: seam_mask"));
    if (warped_mask) ISX_TRY(sw.use_in(warped_mask, st, "dilate_resize_and: warped_mask"));
    ISX_TRY(sd.use_out(out, st, "dilate_resize_and: out"));
    const int mw = seam_mask->cols, mh = seam_mask->rows, dw = out->cols, dh = out->rows;
    const double bytes = (double)dw * dh * (warped_mask ? 2.0 : 1.0);
    const dim3 grid(cdiv(cdiv(dw, RZ_PX), WAVE), cdiv(dh, 4 * DR_ROWS));
    const double scale_x = resize_scale(mw, dw), scale_y = resize_scale(mh, dh);
#define ISX_DR(HALF, K3) ISX_LAUNCH("dilate_resize_and", bytes, st, (k_dilate_resize_and<HALF, K3>), grid, dim3(256), 0, (const unsigned char*)sm.d.data, sm.d.step, mw, mh, kw, kh, \
                                    warped_mask ? (const unsigned char*)sw.d.data : nullptr, warped_mask ? sw.d.step : (size_t)0, (unsigned char*)sd.d.data, sd.d.step, \
                                    dw, dh, scale_x, scale_y)
    const bool half = mw == 2 * dw && mh == 2 * dh, k3 = kw == 3 && kh == 3;
    if (half && k3) ISX_DR(true, true);
    else if (half) ISX_DR(true, false);
    else if (k3) ISX_DR(false, true);
    else ISX_DR(false, false);
#undef ISX_DR
    ISX_TRY(sd.finish_out(st));
    if (any_host) ISX_HIP(hipStreamSynchronize(st));   // the staging buffers are freed on return
    return ISX_OK;
} ISX_EXIT("isx_mask_dilate_resize_and")

}  // extern "C"
