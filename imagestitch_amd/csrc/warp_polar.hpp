// warp_polar.hpp — what warp.hip calls of warp_polar.hip: the fisheye and the stereographic projector (ISX_WARP_FISHEYE,
// ISX_WARP_STEREOGRAPHIC).  Their maps are not separable, so they take no column / row tables: the kernels evaluate proj_math.hpp per pixel.
// Internal.
#pragma once
#include "isx_internal.hpp"

namespace isx {

struct PolarProj {           // warp.hip's Proj, field for field
    float r_kinv[9], k_rinv[9];
    float scale;
    int kind;
};
struct PolarSrc {
    const unsigned char* data;
    size_t step;
    int rows, cols;
};

inline bool polar_kind(int kind) { return kind == ISX_WARP_FISHEYE || kind == ISX_WARP_STEREOGRAPHIC; }
inline const char* polar_kind_name(int kind) { return kind == ISX_WARP_FISHEYE ? "fisheye" : "stereographic"; }

// mapForward of one point and RotationWarperBase::detectResultRoi as a plain loop over every source pixel, on the host: the same text
// the device runs (proj_math.hpp)
void polar_map_forward_host(const PolarProj& p, float x, float y, float& u, float& v);
void polar_roi_host(const PolarProj& p, int sw, int sh, int roi[4], float mm[4]);

// The launchers.  (x0, y0): the destination rectangle's top left corner, dw x dh its size.
// type: one of CV_8UC1 / CV_8UC3 / CV_32FC1 / CV_32FC3 (anything else is ISX_ERR_TYPE)
int polar_launch_warp(hipStream_t st, const PolarProj& p, int type, double bytes, const PolarSrc& src, unsigned char* dst, size_t dstep, int x0, int y0, int dw, int dh,
                      int interp, int border);
// image LINEAR / REFLECT + mask NEAREST / CONSTANT (msk.data null: the all-255 mask); lut: isx_warper_set_gain's 256 bytes or null
int polar_launch_warp_img_mask(hipStream_t st, const PolarProj& p, bool out16, double bytes, const PolarSrc& img, const PolarSrc& msk, const unsigned char* lut,
                               const isx_mat& dimg, const isx_mat& dmask, int x0, int y0, int dw, int dh);
int polar_launch_build_maps(hipStream_t st, const PolarProj& p, const isx_mat& xmap, const isx_mat& ymap, int x0, int y0, int dw, int dh);
// detectResultRoi: the exact u, v of every source pixel reduced into keys[0..3] = min u, min v, max u, max v as order-preserving keys
// (armed by the caller: 0xffffffff, 0xffffffff, 0, 0)
int polar_launch_roi_scan(hipStream_t st, const PolarProj& p, int sw, int sh, unsigned* keys);

}  // namespace isx
