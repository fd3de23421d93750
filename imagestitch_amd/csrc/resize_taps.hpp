// resize_taps.hpp — the taps of cv::resize in plain C++ that the host compiler and the device compiler both take: the tables of
// BlocksGainCompensator's gain-map apply (blocks_gain_host.hpp, also built stand-alone under the host compiler's sanitizers) and the kernels
// of resize.hip, which compute the same taps per pixel, are one text.  Restated from OpenCV 3.4.2 imgproc/src/resize.cpp (plain C++ path; not
// in the reference tree).  A handful of IEEE double and float operations, no contraction (-ffp-contract=off): the same bits on either side.
// What is measured of that (profiles/README.md, "Resize past its suite"): with only the double expression of col_tap / row_tap contracted
// on gfx950 (36 v_fma_f64 in resize.o) the sweep of tests/test_gpu_resize_edges.py - 416 length pairs, rows and columns, 1.7 million taps -
// differed in no pixel, so no test shows that the TAPS need the flag: a fused product moves fx only where the double lies within one of its
// own ulps of a float rounding boundary, about 2^-29 per tap.  What the flag does hold is the CV_32F arithmetic on the taps' values: built
// with -ffp-contract=fast, 408 of the 416 pairs differ.
// Internal, not part of the ABI.
#pragma once
#include <cmath>

#if defined(__HIP__) || defined(__HIPCC__)
#define ISX_HD __host__ __device__
#else
#define ISX_HD
#endif

namespace isx {

// scale = 1.0 / inv_scale with inv_scale = (double)dst / src, as resize() derives it from dsize
inline double resize_scale(int src_n, int dst_n) { return 1.0 / ((double)dst_n / src_n); }

// INTER_LINEAR.  Columns: fx = (float)((dx + 0.5) scale - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> sx = 0, fx = 0; sx >= src_w - 1 -> sx = src_w - 1,
// fx = 0 (no tap to the right is read there).  Rows: the same fy, but fy is KEPT and the two row indices sy, sy + 1 are each clamped to [0, src_h - 1].
struct ColTap { int sx; float a1; };
struct RowTap { int sy0, sy1; float fy; };
ISX_HD inline ColTap col_tap(int dx, double scale_x, int src_w) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = (int)std::floor(fx);
    fx -= (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= src_w - 1) { sx = src_w - 1; fx = 0.f; }
    return ColTap{sx, fx};
}
ISX_HD inline RowTap row_tap(int dy, double scale_y, int src_h) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    const int sy = (int)std::floor(fy);
    fy -= (float)sy;
    const int lo = sy < 0 ? 0 : sy, hi = sy + 1 < 0 ? 0 : sy + 1;
    return RowTap{lo < src_h - 1 ? lo : src_h - 1, hi < src_h - 1 ? hi : src_h - 1, fy};
}

// INTER_NEAREST: min(floor(d scale), src_n - 1) in double
ISX_HD inline int nearest_tap(int d, double scale, int src_n) {
    const int s = (int)std::floor(d * scale);
    return s < src_n - 1 ? s : src_n - 1;
}

// CV_8U's fixed-point coefficient: saturate_cast<short>(cvRound(f * 2048)), f in [0, 1] (so the saturation never acts); ties to even
ISX_HD inline int resize_coef(float f) { return (int)std::rint(f * 2048.f); }
// CV_8U's vertical pass on two horizontal sums H = S[sx] a0 + S[sx + 1] a1
ISX_HD inline int resize_vert_u8(int h0, int h1, int b0, int b1) {
    const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace isx
