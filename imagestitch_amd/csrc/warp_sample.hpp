// warp_sample.hpp — the device samplers of cv::remap that the warp kernels share (warp.hip, warp_polar.hip): the source view, INTER_NEAREST
// and INTER_LINEAR with every border mode.  In an unnamed namespace like the kernels that call them: each translation unit has its own.
#pragma once
#include "../../include/imagestitch_hip.h"
#include "isx_device.hpp"

namespace {

using isxd::border_index;
using isxd::cvround_x86;
using isxd::sat_u8;

struct SrcView {
    const unsigned char* data;
    size_t step;
    int rows, cols;
};

__device__ __forceinline__ int clamp_short(int v) { return min(max(v, -32768), 32767); }

// cv::remap, INTER_NEAREST on a u8 / f32 image of CN channels
template <class T, int CN>
__device__ __forceinline__ void sample_nearest(const SrcView& s, float mx, float my, int border, T* out) {
    int sx = clamp_short(cvround_x86(mx)), sy = clamp_short(cvround_x86(my));
    if (!((unsigned)sx < (unsigned)s.cols && (unsigned)sy < (unsigned)s.rows)) {
        if (border == ISX_BORDER_CONSTANT) {
#pragma unroll
            for (int c = 0; c < CN; ++c) out[c] = 0;
            return;
        }
        sx = border_index(sx, s.cols, border); sy = border_index(sy, s.rows, border);
    }
    const T* q = (const T*)(s.data + (size_t)sy * s.step) + (size_t)sx * CN;
#pragma unroll
    for (int c = 0; c < CN; ++c) out[c] = q[c];
}

// cv::remap, INTER_LINEAR: coordinates quantised to 1/32 px (cvRound(x*32)), taps through
// borderInterpolate; u8 uses the 15-bit fixed-point table, f32 the float table.
template <class T, int CN>
__device__ __forceinline__ void sample_linear(const SrcView& s, float mx, float my, int border, T* out, bool ties_even = false) {
    int isx = cvround_x86(mx * 32.f), isy = cvround_x86(my * 32.f);
    int fx = isx & 31, fy = isy & 31;
    int sx = clamp_short(isx >> 5), sy = clamp_short(isy >> 5);
    if (border == ISX_BORDER_CONSTANT && (sx >= s.cols || sx + 1 < 0 || sy >= s.rows || sy + 1 < 0)) {
#pragma unroll
        for (int c = 0; c < CN; ++c) out[c] = 0;
        return;
    }
    int sx0 = border_index(sx, s.cols, border), sx1 = border_index(sx + 1, s.cols, border);
    int sy0 = border_index(sy, s.rows, border), sy1 = border_index(sy + 1, s.rows, border);
    const bool ok00 = sx0 >= 0 && sy0 >= 0, ok01 = sx1 >= 0 && sy0 >= 0, ok10 = sx0 >= 0 && sy1 >= 0, ok11 = sx1 >= 0 && sy1 >= 0;
    const T* r0 = (const T*)(s.data + (size_t)max(sy0, 0) * s.step);
    const T* r1 = (const T*)(s.data + (size_t)max(sy1, 0) * s.step);
    const int o0 = max(sx0, 0) * CN, o1 = max(sx1, 0) * CN;
    if constexpr (sizeof(T) == 1) {
        // BilinearTab_i: (32-fx)(32-fy)*32 ... ; entry (0,0) saturates to {32767,0,0,1}
        int w0 = (32 - fx) * (32 - fy) * 32, w1 = fx * (32 - fy) * 32, w2 = (32 - fx) * fy * 32, w3 = fx * fy * 32;
        if ((fx | fy) == 0) { w0 = 32767; w3 = 1; }
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            int v0 = ok00 ? r0[o0 + c] : 0, v1 = ok01 ? r0[o1 + c] : 0, v2 = ok10 ? r1[o0 + c] : 0, v3 = ok11 ? r1[o1 + c] : 0;
            const int sum = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3;
            int r = (sum + (1 << 14)) >> 15;                               // FixedPtCast: round half up (OpenCV's CPU remap)
            // ISX_INTER_TIES_EVEN: the same sum as OpenCV's OpenCL (UMat) remap rounds it — half to even
            if (ties_even) r = (fx | fy) == 0 ? v0 : r - (((sum & 32767) == (1 << 14)) & (r & 1));
            out[c] = (T)sat_u8(r);
        }
    } else {
        float ax1 = fx * (1.f / 32.f), ax0 = 1.f - ax1, ay1 = fy * (1.f / 32.f), ay0 = 1.f - ay1;
        float w0 = ay0 * ax0, w1 = ay0 * ax1, w2 = ay1 * ax0, w3 = ay1 * ax1;
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            float v0 = ok00 ? r0[o0 + c] : 0.f, v1 = ok01 ? r0[o1 + c] : 0.f, v2 = ok10 ? r1[o0 + c] : 0.f, v3 = ok11 ? r1[o1 + c] : 0.f;
            out[c] = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3;
        }
    }
}

}  // namespace
