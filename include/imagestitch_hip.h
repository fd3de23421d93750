/*
 * imagestitch_hip.h — C-ABI of the MI355X (gfx950) warp + multi-band blend hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one call the
 * reference makes on cv::detail::RotationWarper / cv::detail::Blender (or their in-tree
 * restatements).  Reference files, cited as alias:line (raw-file line numbers):
 *   W = /root/reference/圆柱面投影变换/圆柱面投影变换/圆柱面投影.cpp   (cylindrical warper demo)
 *   B = /root/reference/图像融合/图像融合/图像融合.cpp                 (blend demo)
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions across the boundary.
 *   - every function returns an isx_status (0 = OK); isx_last_error() returns a thread-local
 *     human-readable message for the last failure (the analogue of cv::Exception::what()).
 *   - isx_mat mirrors cv::Mat{data,rows,cols,type(),step}; `type` uses OpenCV's numeric type
 *     codes so an adapter can pass mat.type() through unchanged.  `device` = -1 means `data`
 *     is a host pointer (the library stages it through HBM, PCIe-inclusive), >= 0 means
 *     `data` is a HIP device pointer on that device (zero-copy; the measured path).
 *   - output mats are caller-allocated (replaces OutputArray::create, W:128-129,150); the
 *     *_roi / *_result_size queries give the sizes.
 *   - all work is enqueued on the handle's HIP stream (isx_*_set_stream); calls that return
 *     host values (ROI, corner) synchronise that stream, the others are asynchronous when all
 *     mats are device mats.
 */
#ifndef IMAGESTITCH_HIP_H
#define IMAGESTITCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (CV_Assert / CV_Error analogue, W:94-96) ------------------------------ */
typedef enum {
    ISX_OK = 0,
    ISX_ERR_INVALID = 1,     /* bad argument (null pointer, bad enum, bad size)                 */
    ISX_ERR_TYPE = 2,        /* wrong isx_mat type for this call (CV_Assert(type()==...))       */
    ISX_ERR_STATE = 3,       /* call order violated (feed before prepare, blend twice, ...)     */
    ISX_ERR_HIP = 4,         /* a HIP runtime call failed; message carries hipGetErrorString    */
    ISX_ERR_NOMEM = 5,       /* hipMalloc failed                                                */
    ISX_ERR_UNSUPPORTED = 6, /* valid in OpenCV, not implemented on this path                   */
    ISX_ERR_SIZE = 7,        /* caller-allocated output has the wrong rows/cols                 */
    ISX_ERR_PLAN = 8,        /* a planned (sync-free) run saw geometry that differs from plan   */
    ISX_ERR_INTERNAL = 9     /* a C++ exception was stopped at this boundary (never propagated) */
} isx_status;

/* ---- cv::Mat type codes: depth + ((cn-1)<<3), same numbers as OpenCV -------------------- */
enum {
    ISX_8UC1 = 0,   /* CV_8UC1  : masks (W:213-214,232)                                       */
    ISX_8UC3 = 16,  /* CV_8UC3  : source and warped images (W:166-169,229)                    */
    ISX_8UC4 = 24,  /* CV_8UC4  : a BGRA source image (F:959-960): isx_orb_find only          */
    ISX_16SC3 = 19, /* CV_16SC3 : Blender::feed input / blend output (W:294,302,313)          */
    ISX_32SC1 = 4,  /* CV_32SC1 : the seam finder's label image labels_ (S:83)                    */
    ISX_32FC1 = 5,  /* CV_32FC1 : xmap / ymap (W:128-129)                                     */
    ISX_32FC3 = 21, /* CV_32FC3 : float images (W:261; B:143-145)                             */
    ISX_64FC1 = 6   /* CV_64FC1 : MatchesInfo::H and confidence (R:862, R:874): isx_find_homography only */
};

/* cv::InterpolationFlags / cv::BorderTypes values used by W:229,232 */
enum { ISX_INTER_NEAREST = 0, ISX_INTER_LINEAR = 1,
       /* not an OpenCV flag: OR it to ISX_INTER_LINEAR in isx_warper_warp / isx_remap to round the 8-bit bilinear sum half to
        * EVEN, as OpenCV's OpenCL (UMat / T-API) remap does — the arithmetic the reference's committed images_warped_f[0].bmp
        * was produced with.  Default (OpenCV's CPU remap, the reference CPU path): half up.                         */
       ISX_INTER_TIES_EVEN = 0x100 };
enum { ISX_BORDER_CONSTANT = 0, ISX_BORDER_REPLICATE = 1, ISX_BORDER_REFLECT = 2,
       ISX_BORDER_WRAP = 3, ISX_BORDER_REFLECT_101 = 4 };

/* warper kinds: cv::CylindricalWarper (W:219) / cv::SphericalWarper (B:93, commented) / cv::PlaneWarper (B:91, commented) /
 * cv::FisheyeWarper (B:94, commented) / cv::StereographicWarper (B:95, commented).
 * The last two are not separable (no column / row tables): every pixel evaluates the restated float32 sinf / cosf / atan2f / atanf / acosf
 * of csrc/proj_math.hpp, and detectResultRoi is the base class's scan of every source pixel, exact on the device (one launch, four floats
 * back).  They serve isx_warper_create, _camera, _roi, _warp_point, _build_maps(_roi), _warp(_roi), _warp_with_mask(_roi), _set_gain,
 * _set_stream and _set_roi_cache.  isx_warper_warp_with_mask_planned, _queue_verify, _verify_is_light, _begin_batch, _set_dst_columns,
 * _set_deferred_verify(on) and a non-zero _set_translation return ISX_ERR_UNSUPPORTED for them and change no state.                  */
enum { ISX_WARP_CYLINDRICAL = 0, ISX_WARP_SPHERICAL = 1, ISX_WARP_PLANE = 2, ISX_WARP_FISHEYE = 3, ISX_WARP_STEREOGRAPHIC = 4 };

/* cv::detail::Blender::{NO, FEATHER, MULTI_BAND} (W:271,276,278) */
enum { ISX_BLEND_NO = 0, ISX_BLEND_FEATHER = 1, ISX_BLEND_MULTI_BAND = 2 };

/* pyramid precision of the multi-band blender */
enum {
    ISX_PREC_I16 = 0,      /* OpenCV's arithmetic: int16 Laplacian pyramid, fp32 weights       */
    ISX_PREC_F32 = 1,      /* everything fp32, same order of operations, no short casts        */
    ISX_PREC_F16ACC32 = 2  /* Gaussian levels stored fp16, arithmetic + accumulators fp32      */
};

typedef struct isx_mat {
    void*  data;    /* first byte of row 0                                                     */
    int    rows;
    int    cols;
    int    type;    /* ISX_8UC1 ...                                                            */
    size_t step;    /* bytes between consecutive rows (cv::Mat::step)                          */
    int    device;  /* -1: host pointer; >=0: HIP device pointer on that device                */
} isx_mat;

typedef struct isx_warper  isx_warper;
typedef struct isx_blender isx_blender;

/* ---- library ---------------------------------------------------------------------------- */
const char* isx_last_error(void);            /* thread-local message of the last failure      */
const char* isx_version(void);
int         isx_device_count(int* count);    /* hipGetDeviceCount; ISX_ERR_HIP if no runtime  */

/* ---- warper: replaces warper_creator->create(scale) + RotationWarper (W:217-233) -------- */
/* replaces Ptr<RotationWarper> w = warper_creator->create(float scale)  (W:217-222; the
 * in-tree twin hard-codes `float scale = 2707.47f`, W:30).  `device` is the HIP device.      */
int isx_warper_create(int kind, float scale, int device, isx_warper** out);
int isx_warper_destroy(isx_warper* w);
int isx_warper_set_stream(isx_warper* w, void* hip_stream /* hipStream_t, NULL = default */);

/* setCameraParams (W:90-120): K, R are 3x3 row-major CV_32F.  Writes r_kinv = R*K^-1 (W:108)
 * and k_rinv = K*R^T (W:113) as the library computes them (for inspection / parity tests).   */
int isx_warper_camera(isx_warper* w, const float K[9], const float R[9],
                      float r_kinv[9], float k_rinv[9]);

/* detectResultRoi (W:64-88): full forward scan of every source pixel on the GPU.
 * roi = {tl.x, tl.y, br.x, br.y} (inclusive br, trunc-toward-zero casts, W:83-86).
 * minmax (optional, may be NULL) receives the four float extrema {min u, min v, max u, max v}. */
int isx_warper_roi(isx_warper* w, int src_w, int src_h, const float K[9], const float R[9],
                   int roi[4], float minmax[4]);
/* Opt-in: remember detectResultRoi's result per (K, R, scale, source size) - it is a pure function of them - so that a
 * fixed rig's repeated isx_warper_warp / _roi / _build_maps calls skip the GPU scan and its host round trip (the corner
 * must reach the host before the destination can be sized, W:148-150).  The spherical ROI (host code) is not cached.
 * Off by default: only the LAST result is then remembered - the reference asks for the same ROI twice in a row (warp(img, K, R), then
 * warp(mask, K, R), W:229,232) and the second call returns the first one's answer; any other call computes its ROI as the reference does. */
int isx_warper_set_roi_cache(isx_warper* w, int on);
/* Introspection of the mapBackward table arena: how many times it has started over.  Tables are cached per (kind, scale, ROI) in 4 MiB
 * chunks, at most 1024 entries and 16 MiB; when either is full the arena starts over, after waiting for the current stream and for every
 * stream this handle left (isx_warper_set_stream) since the last start-over.  A chunk that a warp enqueued on a CAPTURING stream read from is
 * never rewritten: a start-over sets it aside until isx_warper_destroy and continues in fresh chunks - at most the 4 chunks (16 MiB) the
 * arena held per start-over that follows a capture.  A warp on a capturing stream whose table is not cached fails with ISX_ERR_STATE
 * before it enqueues anything: run the same warp once eagerly before the capture.
 * The fisheye and stereographic kinds have no tables; their rule on a capturing stream ("Capture"): _warp_roi, _warp_with_mask_roi
 * and _build_maps_roi on device mats are one kernel launch and can be captured; any entry given a host mat, and _roi / _warp /
 * _warp_with_mask / _build_maps for a camera and source size whose ROI the handle does not remember (isx_warper_set_roi_cache), fail with
 * ISX_ERR_STATE before the handle changes or anything is enqueued: pass device mats, and query the ROI once before the capture.      */
int isx_warper_table_resets(isx_warper* w, long long* resets);
/* compensator->apply(i, corners[i], images_warped[i], masks_warped[i]) (W:241-244) folded into the fused tile warps that
 * follow (isx_warper_warp_with_mask / _roi / _planned with src_mask == NULL): every byte of the warped IMAGE becomes
 * saturate_cast<uchar>(cvRound((double)byte * gain)) - exactly isx_gain_apply on the warped tile, one pass over it less (the gain acts on
 * the remapped byte, not on the source: remap of scaled pixels is a different number).  gain = 1.0 switches it off.                    */
int isx_warper_set_gain(isx_warper* w, double gain);
/* cv::detail::PlaneWarper's translation (B:91 `cv::PlaneWarper()`, created at W:217-222): the T of its warp / buildMaps / warpRoi /
 * warpPoint (src, K, R, T, ...) overloads, a 3x1 CV_32F.  Sticky like the gain: every call that follows on this handle projects with it;
 * the default is zero, which is what the overloads without T pass.  Finite values only.  ISX_ERR_UNSUPPORTED on a handle that is not a
 * plane warper, unless T is all zero.  The plane ROI is mapForward of the four source corners (min / max, trunc-toward-zero casts): it is
 * computed on the caller's thread, with nothing launched and no synchronisation; a planned warp's ROI is verified by the same rule when the
 * warp is issued, and isx_warper_plan_status reports a mismatch.                                                                          */
int isx_warper_set_translation(isx_warper* w, const float T[3]);
/* RotationWarper::warpPoint(pt, K, R) (the creators of B:91-95, W:217-222): mapForward of one source point under (K, R) - and the handle's
 * translation, for a plane warper - on the host, with the host's libm as the stock classes use it.  out_uv = {u, v}; no device work.
 * Like every entry that takes (K, R) it is a setCameraParams on the handle: it overwrites the handle's current projection (harmless - each
 * entry sets the camera it is given - but a change of handle state), so it must not run concurrently with another call on the same handle. */
int isx_warper_warp_point(isx_warper* w, const float K[9], const float R[9], float x, float y, float out_uv[2]);

/* buildMaps (W:122-144): xmap,ymap are caller-allocated CV_32FC1 of
 * (roi[3]-roi[1]+1) rows x (roi[2]-roi[0]+1) cols (W:128-129).                               */
int isx_warper_build_maps(isx_warper* w, int src_w, int src_h, const float K[9], const float R[9],
                          isx_mat* xmap, isx_mat* ymap, int roi[4]);

/* The map fill of buildMaps (W:133-141) over a rectangle the caller already has - isx_warper_roi's result for this camera, or the
 * rectangle of maps it keeps - without the scan: xmap(v - roi[1], u - roi[0]) = mapBackward(u, v).x, same for ymap.               */
int isx_warper_build_maps_roi(isx_warper* w, const float K[9], const float R[9], const int roi[4], isx_mat* xmap, isx_mat* ymap);

/* Point warp(src,K,R,interp,border,dst) (W:145-161; stock call sites B:105,109): buildMaps +
 * cv::remap (W:157) fused into one gather kernel; the maps are never written to HBM.
 * src: CV_8UC3 / CV_8UC1 (fixed-point bilinear) or CV_32FC3 / CV_32FC1 (float bilinear).
 * dst: caller-allocated, same type, (roi.h+1) x (roi.w+1) (W:150).  corner = roi.tl() (W:160).
 * Limits: none that refuses a mat.  The two calls the reference makes (CV_8UC3 LINEAR / REFLECT, CV_8UC1 NEAREST / CONSTANT) take the tile
 * kernels while the source has step < 2^24 bytes, step * rows < 2^31 and at most 32767 pixels a side and the destination step < 2^24
 * and step * rows < 2^32 (a host mat: its dense staged copy); any other mat takes the generic kernel (64-bit addresses), same bits. */
int isx_warper_warp(isx_warper* w, const isx_mat* src, const float K[9], const float R[9],
                    int interp, int border, isx_mat* dst, int corner[2]);

/* The second half of the same call for adapters that must size `dst` themselves (OutputArray::create, W:150): `roi` is what
 * isx_warper_roi just returned for the same (source size, K, R) on this handle, so that ONE reference warp() = one
 * detectResultRoi (W:126) = isx_warper_roi + isx_warper_warp_roi, not two scans.  No scan, no host synchronisation (device
 * mats).  A `roi` that is not detectResultRoi's is not checked: the result is then the remap over that rectangle.          */
int isx_warper_warp_roi(isx_warper* w, const isx_mat* src, const float K[9], const float R[9],
                        int interp, int border, const int roi[4], isx_mat* dst);
/* ... and of the fused image + mask call below.                                                                        */
int isx_warper_warp_with_mask_roi(isx_warper* w, const isx_mat* src_img, const isx_mat* src_mask, const float K[9],
                                  const float R[9], const int roi[4], isx_mat* dst_img, isx_mat* dst_mask);

/* The two calls of W:229 + W:232 on one tile fused: image LINEAR/REFLECT and mask
 * NEAREST/CONSTANT in one pass over the destination.  src_mask may be NULL = all 255
 * (W:213-214).  dst_img may be CV_8UC3 or CV_16SC3 (= warp + convertTo(CV_16S), W:294).
 * Limits (this call, _roi, _planned and the batched form; there is no generic kernel behind them): src_img with step < 2^24 bytes,
 * step * rows < 2^31 and at most 32767 pixels a side; dst_img AND dst_mask each with step < 2^24 and step * rows < 2^32 (host mats:
 * their dense staged copies).  Past any of them: ISX_ERR_UNSUPPORTED, nothing is written - inside a batch the tile is not collected
 * and the batch ends as for any failing warp.  src_mask (its size is src_img's) is read through 64-bit addresses: any pitch.      */
int isx_warper_warp_with_mask(isx_warper* w, const isx_mat* src_img, const isx_mat* src_mask,
                              const float K[9], const float R[9],
                              isx_mat* dst_img, isx_mat* dst_mask, int corner[2]);

/* Sync-free variant for captured / batched runs: the caller supplies the ROI it planned with
 * isx_warper_roi; the ROI scan still runs on the GPU and is compared with `planned_roi` on
 * the device; a mismatch raises the sticky flag read by isx_warper_plan_status.               */
int isx_warper_warp_with_mask_planned(isx_warper* w, const isx_mat* src_img,
                                      const isx_mat* src_mask, const float K[9],
                                      const float R[9], const int planned_roi[4],
                                      isx_mat* dst_img, isx_mat* dst_mask);
/* Several tiles' warps in ONE launch.  Between begin and end the fused tile warps of this handle (isx_warper_warp_with_mask / _roi / _planned
 * with src_mask == NULL, device mats, no gain) are collected instead of launched, and isx_warper_end_batch sends them off as one launch of up
 * to 8 tiles per kernel variant (blockIdx.z = tile): the per-image loop of the reference (W:223-233) issues one warp after the other, and on
 * a GPU each launch waits for the last - longest-lived - waves of the one before and pays its own dispatch ramp (~3 us of a 175 us step).
 * Same kernel body, same bits.  The outputs are not written, nor even enqueued, before isx_warper_end_batch returns: use them (feed them)
 * after it.  isx_warper_verify / _join / _plan_status / _set_stream end the collection's pending launches as well; anything that cannot be
 * collected (a caller-supplied source mask, host mats, a gain) is launched at once, behind what was collected so far.                  */
/* A warp that FAILS while a batch is collecting (a wrong dst size, say) ends the batch: the warps collected before it are launched and the
 * handle is no longer batching (a following isx_warper_end_batch returns ISX_OK and launches nothing).  isx_warper_destroy launches an open
 * batch before it waits for the stream: a warp that returned ISX_OK always writes its output.                                          */
int isx_warper_begin_batch(isx_warper* w);
int isx_warper_end_batch(isx_warper* w);
/* The count is STICKY for the life of the handle, for every kind: the device-side counter of the cylindrical / spherical scans is never
 * cleared, and neither is the host-side count of a plane handle's four-corner checks (isx_warper_discard_pending drops verifications that
 * have not run yet, not findings).  After one stale plan every later isx_warper_plan_status of that handle returns ISX_ERR_PLAN: make a
 * new plan on a new handle.
 * What the check can miss.  The device compares monotone stand-ins of the scanned extrema (the diamond angle d of u; v / scale for the
 * cylinder, w = -cos(v / scale) for the sphere) with the stand-ins of the ends of each planned bound's truncation interval, and allows
 * 4e-6 * max(1, |stand-in of either end|) beyond an end: the blind zone is relative IN STAND-IN SPACE.  In pixels that is 4e-6 to 1.6e-5 *
 * scale for u, 4e-6 * max(scale, |v|) for the cylinder's v, and for the sphere's v about 4e-6 * scale / sin(v / scale) away from the poles
 * but sqrt(d * d + 8e-6 * scale * scale) - d at d pixels from a pole: 0.0028 * scale at the pole itself (1.7 px at scale 617).  Three
 * kinds of stale plan are decided exactly, on the host, when the verification is issued, with no allowance: a u bound beyond
 * +-(int)(scale * pi_f); with a pole of the sphere inside the image, a value other than the pole's own for the bound it dictates
 * (br.v = (int)(float)(pi * scale) for the north pole, tl.v = 0 for the south pole); and, for the other bounds beside a pole, a tl above
 * the pole's value or a br below it (tl.u > 0, br.u < 0).  They are counted on the device like every other stale plan: once per
 * verification, and once per replay of a captured one.                                                                               */
int isx_warper_plan_status(isx_warper* w, int* mismatches /* synchronises the stream */);
/* The verification scans of planned warps run on an internal side stream.  isx_warper_join makes the
 * handle's stream wait for them without blocking the host — required before hipStreamEndCapture when
 * the planned step is captured into a hipGraph (the forked work must re-join the capturing stream).   */
int isx_warper_join(isx_warper* w);
/* By default the verification scan of a planned warp is enqueued right behind its warp kernel.  With
 * deferred verification the scans are queued and isx_warper_verify enqueues them behind the stream's
 * position at THAT call — e.g. after the last warp of a step, so that the (VALU-bound) scans run under the
 * (memory-bound) pyramid kernels that follow.  join / plan_status flush the queue themselves.            */
int isx_warper_set_deferred_verify(isx_warper* w, int on);
/* Column range of the warped tile (nothing in the reference; the companion of isx_blender_set_window): the isx_warper_warp_with_mask*
 * calls that follow (without a source mask) compute only the columns [col0, col1) of dst_img / dst_mask - the left end rounded down to a
 * block of 64, the right end exactly col1 - and leave the rest of the mats as it is (of a host mat only the computed columns are copied
 * back from its staging buffer; the same holds for the padded last strip of a windowed blend).  For a rank that needs part of a neighbour's tile to blend its strip of a
 * panorama (imagestitch_amd/mosaic.py: tile_columns_for_window gives the range).  (0, 0) = the whole tile again.              */
int isx_warper_set_dst_columns(isx_warper* w, int col0, int col1);
int isx_warper_verify(isx_warper* w);
/* Verification beside a hipGraph instead of inside it (a fork of the verification stream inside a captured step costs the replay 12 us at 4K):
 * isx_warper_discard_pending drops the scans the planned warps of a CAPTURED step queued; after every replay the caller queues the same
 * verifications from the rig alone - isx_warper_queue_verify(source size, K, R, planned ROI): the scan reads no image - and starts them with
 * isx_warper_verify.  isx_warper_plan_status reports a stale plan as for any planned warp.                                           */
int isx_warper_discard_pending(isx_warper* w);
int isx_warper_queue_verify(isx_warper* w, int src_w, int src_h, const float K[9], const float R[9], const int planned_roi[4]);
/* Scheduling hint (nothing in the reference): is the verification of a planned warp of a src_cols x src_rows source under (K, R) a
 * border scan - one workgroup over the 2 (W + H) border pixels, which starts at once, with no event on the handle's stream - (1), or
 * the full detectResultRoi scan of every source pixel (0), which is worth placing under memory-bound work
 * (isx_blender_set_mark_event + isx_warper_verify_after)?  Spherical: always 1.  Cylindrical: 1 when the extrema provably lie on the
 * border (the image in front of the camera, no pole within two pixels of it).                                                          */
int isx_warper_verify_is_light(isx_warper* w, int src_cols, int src_rows, const float K[9], const float R[9], int* light);
/* Same, but the scans start once `hip_event` (a hipEvent_t already recorded, e.g. by
 * isx_blender_set_mark_event during blend()) has completed instead of at the stream's current position.  */
int isx_warper_verify_after(isx_warper* w, void* hip_event);

/* cv::remap(src, dst, xmap, ymap, interp_mode, border_mode) itself (W:157), for callers that keep the maps of a
 * fixed rig (isx_warper_build_maps once, isx_remap per frame).  CV_32FC1 maps; src / dst CV_8UC1, CV_8UC3, CV_32FC1 or
 * CV_32FC3; OpenCV's CPU arithmetic (coordinates quantised to 1/32 pixel, 15-bit fixed-point weights for 8-bit images).
 * Limits: a source of more than 32767 pixels a side is ISX_ERR_UNSUPPORTED (cv::remap's short coordinates), dst untouched; any pitch. */
int isx_remap(const isx_mat* src, const isx_mat* xmap, const isx_mat* ymap, int interp_mode, int border_mode,
              isx_mat* dst, int device, void* hip_stream);

/* ---- blender: replaces Blender::createDefault + MultiBandBlender (W:271-281,302,313) ---- */
/* Blender::createDefault(type, try_gpu) (W:271,276,278) + setNumBands (W:273).
 * type: ISX_BLEND_MULTI_BAND (num_bands default in OpenCV: 5), ISX_BLEND_FEATHER (the blender every
 * reference demo actually runs, W:278-280; num_bands / precision are ignored, sharpness 0.02) or ISX_BLEND_NO
 * (W:276: the base class - feed() is a masked copy, blend() zeroes what no mask covered).            */
int isx_blender_create(int type, int num_bands, int precision, int device, isx_blender** out);
int isx_blender_destroy(isx_blender* b);
int isx_blender_set_stream(isx_blender* b, void* hip_stream);
int isx_blender_set_num_bands(isx_blender* b, int num_bands);   /* mb->setNumBands(n), W:273 */
int isx_blender_num_bands(isx_blender* b, int* num_bands);      /* after prepare: the clamped */
int isx_blender_set_sharpness(isx_blender* b, float sharpness); /* fb->setSharpness(0.1), W:280 */

/* blender->prepare(corners, sizes) (W:281): corners_xy = {x0,y0,x1,y1,...}, sizes_wh likewise */
int isx_blender_prepare(isx_blender* b, int n, const int* corners_xy, const int* sizes_wh);
/* MultiBandBlender::prepare(Rect dst_roi).
 * Limits (both forms): the ROI padded to a multiple of 2^num_bands must stay below 2^24 pixels a side and 2^31 pixels in all (records are
 * indexed with 32 bits; Blender::NO and FEATHER: one level); beyond: ISX_ERR_UNSUPPORTED before anything is allocated.              */
int isx_blender_prepare_roi(isx_blender* b, int x, int y, int width, int height);

/* blender->feed(img [CV_16SC3], mask [CV_8U], tl) (W:302).  img may also be CV_32FC3 in
 * the F32 / F16ACC32 precisions, and CV_8UC3: OpenCV then takes createLaplacePyr's 8-bit branch,
 * whose numbers are those of the CV_16S branch on the converted image (bytes never saturate in
 * pyrDown / pyrUp) - the same path as isx_blender_feed_u8.
 * Limits (isx_blender_feed, _feed_u8, _feed_dilated): none that refuses a tile.  A CV_8UC3 / CV_16SC3 tile whose image and mask both have
 * step < 2^24 bytes and step * rows < 2^31 is read with 32-bit offsets (the fused feed of mode 2, k_collapse_roll as the last step);
 * any other tile through 64-bit addresses (mode 2: a plain private copy; the last step k_collapse_gather when the caller's mat itself
 * is read) - same bits, isx_blender_feed_path / isx_blender_last_path say which.                 */
int isx_blender_feed(isx_blender* b, const isx_mat* img, const isx_mat* mask, int tl_x, int tl_y);
/* images_warped.convertTo(CV_16S) (W:261,294) fused into feed: img is CV_8UC3 and is widened
 * to int16 on load; results are identical to converting first and calling isx_blender_feed.   */
int isx_blender_feed_u8(isx_blender* b, const isx_mat* img, const isx_mat* mask, int tl_x, int tl_y);
/* the mask preparation of W:286-301 inside the feed - mask = dilate(seam_mask, getStructuringElement(MORPH_RECT, Size(kw, kh)))
 * & warped_mask is computed straight into the mask buffer the blender keeps for the tile (its private copy under
 * isx_blender_set_deferred_level0 = 2), then blender->feed(img, mask, tl) (W:302) as isx_blender_feed does: identical results, no
 * intermediate mask mat, one pass over the mask less.  Every blender type; elements up to 33 a side (ISX_ERR_UNSUPPORTED beyond:
 * isx_mask_dilate_and + isx_blender_feed); img CV_16SC3 or CV_8UC3.                                                                */
int isx_blender_feed_dilated(isx_blender* b, const isx_mat* img, const isx_mat* seam_mask, const isx_mat* warped_mask, int kw, int kh,
                             int tl_x, int tl_y);

/* Opt-in: deferred mode.  feed() then only RECORDS the tile and blend() does all the work: the
 * Gaussian chains of all tiles (one launch per level), then a collapse chain whose every step
 * gathers the tiles' Laplacians in registers.  The destination Laplacian / weight pyramid
 * (32 B/px of read-modify-write per feed, 16 B/px read back by blend) never touches HBM.
 * Results are identical to the eager path.  THE CONTRACT THAT CHANGES: every DEVICE mat passed to
 * feed()/feed_u8() must stay valid and unmodified until blend() returns (OpenCV's feed() consumes
 * its inputs immediately — the reference clears the fed images before blend(), W:305-308 — so this
 * is not the default).  Host mats are staged in per-tile device buffers owned by the blender:
 * nothing changes for them.  A launch's arguments hold 20 tiles: a cycle of more tiles (up to 4096, one type) runs the same chain with the
 * tiles' descriptors in a table in device memory (isx_blender_last_path: cycle 4; round 4's column strips of at most 20 tiles, cycle 3, remain
 * as ISX_TAB=0), bit-identical; when a tile of another type is fed, when isx_blender_debug_level is called, and for an int16 cycle of CV_8UC3
 * tiles stacked more than 128 deep over one place, the recorded tiles are replayed through the eager path.
 * on = 2 keeps OpenCV's contract: feed() takes a private copy of every DEVICE mat it records, so the caller may release or overwrite
 * the fed mats as soon as feed() returns - the drop-in mode for callers written against cv::detail::Blender (W:286-308).  For CV_8UC3
 * and CV_16SC3 tiles that copy is a by-product of the pass that builds level 1 of the tile's pyramid (one read of the caller's mats per
 * feed, isx_blender_feed_path); other mats take one device-to-device pass on the handle's stream.                                  */
int isx_blender_set_deferred_level0(isx_blender* b, int on);
/* In deferred mode: start each fed tile's Gaussian chain immediately on an internal side stream, so that
 * the (memory-bound) chain of tile t overlaps with whatever the caller enqueues next on the handle's
 * stream — typically the (VALU-bound) warp of tile t+1.  blend() joins the side streams.               */
int isx_blender_set_overlap(isx_blender* b, int on);
/* Scheduling hook, nothing in the reference: a deferred blend() records `hip_event` (hipEvent_t, NULL = off) on its
 * stream right after the pyrDown launch that produces level after_level + 1 of the tile pyramids.  From there to the
 * last collapse step the launches are small and leave most of the GPU idle: the place for unrelated VALU-bound work
 * such as the ROI verification scans (isx_warper_verify_after).                                           */
int isx_blender_set_mark_event(isx_blender* b, void* hip_event, int after_level);
/* Column window (one panorama of many tiles cut into column strips, a strip per GPU, no exchange before the final
 * gather).  Nothing in the reference corresponds to it.  With a window [x0, x1) set - columns of the result, 0 = the left edge of
 * dst_roi, x0 a multiple of ISX_WINDOW_GRANULE - blend() of a deferred cycle (MultiBandBlender or FeatherBlender) computes and writes those columns
 * only, into mats that are x1 - x0 wide (columns past the result's right edge, when x1 exceeds its width, are not touched); every
 * pixel equals the same pixel of the whole blend, bit for bit.  prepare() still gets EVERY tile's corner and size (dst_roi is the
 * whole panorama's); only the tiles that can reach the window need to be fed: those whose fed rectangle - the tile widened by the
 * gap 3 * 2^num_bands on either side, as MultiBandBlender::feed does - comes within 2^(num_bands + 1) columns of the window
 * (imagestitch_amd/mosaic.py: tiles_for_window; for the FeatherBlender simply the tiles that overlap the window).  The window stays
 * set until changed; (0, 0) removes it.                                                                                       */
#define ISX_WINDOW_GRANULE 128
int isx_blender_set_window(isx_blender* b, int x0, int x1);

/* size of the result of blend(): dst_roi_final_ (unpadded union of the fed tiles)             */
int isx_blender_result_size(isx_blender* b, int* width, int* height);
/* Which code path the last isx_blender_blend / _blend_batch of a multi-band blender took - the fast kernels have limits (tile type, tiles
 * per place, tile count: DESIGN.md §3) and nothing else says which side of them a blend ran on.  cycle: 0 eager (the destination pyramid),
 * 1 deferred, 2 deferred inside a batched chain, 3 deferred in column strips (ISX_TAB=0 and more than 20 recorded tiles: the library cuts the
 * result into strips that at most 20 tiles reach and runs the deferred chain per strip - bit-identical to the whole blend), 4 deferred with the
 * tiles in a device-resident table (more than 20 recorded tiles: one chain over all of them); last_step: the kernel of the last collapse step -
 * 0 none (a 0-band blend), 1 k_collapse, 2 k_collapse_gather, 3 k_collapse_roll.  Either pointer may be NULL.                    */
int isx_blender_last_path(isx_blender* b, int* cycle, int* last_step);
/* Layout of level 1 of the tiles' Gaussian pyramids in the last deferred isx_blender_blend (an internal buffer; reported because the step's
 * byte count depends on it): 0 = 16-byte records, 1 = planar (12-byte image records, int16: 6, + a weight plane), 2 = planar with the image
 * channels as three unsigned shorts (fp32 pyramids over CV_8UC3 tiles: level 1 is k / 256 exactly, DESIGN.md §3 "Round 5").               */
int isx_blender_level1_format(isx_blender* b, int* format);
/* Introspection of cycle 4: how many 3.5 KB pieces of tile tables this blender has uploaded so far.  They travel in kernel arguments, in
 * stream order, and only where they differ from what the device holds: a fixed rig uploads on its first blend() and never again.      */
int isx_blender_table_uploads(isx_blender* b, long long* pieces);
/* Once a step of this blender has been captured into a hipGraph (its stream was seen capturing), a later call that outgrows one of its device
 * buffers - more tiles, a larger panorama, more bands - keeps the old allocation alive until isx_blender_destroy instead of freeing it, since
 * a replay of the graph still reads and writes it.  This reports the bytes so kept (0 for a blender that was never captured).          */
int isx_blender_retained_bytes(isx_blender* b, long long* bytes);
/* How the tiles of the last isx_blender_blend were FED in mode 2 (isx_blender_set_deferred_level0 = 2, OpenCV's contract W:302-308).
 * fused_tiles: tiles whose feed() was ONE pass over the caller's CV_8UC3 / CV_16SC3 device mats - level 1 of the tile's pyramid and the
 * private copy out of the same read (round 5; 0: host mats, other tile types, ISX_FEED_FUSE=0).  narrowed: 0 = no private copy was
 * narrowed; 1 = the CV_16SC3 tiles held only byte values (always the case after convertTo(CV_16S) of a warped CV_8UC3 image, W:294),
 * their private copies were kept as CV_8UC3 and the last collapse step ran its CV_8UC3 form - same bits, 3 fewer bytes per pixel written
 * and read; 2 = some tile held a value outside [0, 255]: the copies were widened to CV_16SC3 before the last step (same bits; this
 * blender keeps CV_16SC3 copies from then on).  The check is made on the device while the tile is read; blend() reads its one-word
 * answer from pinned memory after it has enqueued everything that does not depend on it - no stream synchronisation.  Either pointer
 * may be NULL.                                                                                                                    */
int isx_blender_feed_path(isx_blender* b, int* fused_tiles, int* narrowed);
/* Narrowed private copies (mode 2, CV_16SC3 device tiles) make blend() WAIT FOR THE GPU once: before it picks the last step's kernel the
 * calling thread polls the pinned word that the first launch of blend()'s own chain publishes, i.e. it waits until the GPU has worked off
 * whatever the stream held in front of that launch (no hipStreamSynchronize, but with a deep queue on the stream the host stalls for the
 * backlog, and a stream gated behind something this thread would only release AFTER blend() returns - a host callback, a host-signalled
 * event - would never reach the launch: the wait gives up into a stream synchronisation after 20 s).  on = 0 switches the narrowing off
 * for this blender (what the environment variable ISX_FEED_NARROW=0 does for the process): private copies of CV_16SC3 tiles stay
 * CV_16SC3, blend() enqueues and returns without looking at the device; same bits, 3 more bytes per pixel written and read (a 4K pair:
 * the last step 50 -> 60 us).  on = 1 (default) allows it again.  Call it before the first feed of a cycle (ISX_ERR_STATE otherwise).
 * hipGraph capture never narrows.                                                                                                    */
int isx_blender_set_narrow_copies(isx_blender* b, int on);
/* blender->blend(result, result_mask) (W:313).  dst: CV_16SC3 (I16: exact; F32: saturate_cast
 * round-half-even), CV_32FC3 (F32/F16ACC32 only) or CV_8UC3 (= blend to CV_16SC3 followed by
 * result.convertTo(CV_8U), what imwrite (W:315) does to the panorama); dst_mask: CV_8UC1.  Releases the pyramids:
 * prepare must be called again before the next feed (as in OpenCV).
 * Limits: dst AND dst_mask each need step < 2^24 bytes and step * rows < 2^32 (with a column window: plus the window's first column in
 * bytes; host mats: their dense staged copies).  Past them: ISX_ERR_UNSUPPORTED, nothing is written and the blender stays prepared and
 * fed - blend() into smaller-pitched mats then succeeds.  The same holds per blender in isx_blender_blend_batch.      */
int isx_blender_blend(isx_blender* b, isx_mat* dst, isx_mat* dst_mask);
/* blend() of n blenders at once - the per-image loop of the reference's main() (W:223-233, 285-302, 313) run for a BATCH of independent
 * mosaics (BASELINE configs 3 and 4: 16 / 4 pairs per step).  Blenders that are in the deferred cycle (isx_blender_set_deferred_level0)
 * with the same precision, band count, tile type, device and stream share ONE chain of launches, up to 6 mosaics / 20 tiles per chain:
 * every level's Gaussian chain and collapse step is one launch for all of them (the mosaic is the grid's z), so the levels that
 * are launch-latency-bound for one pair run at P times the waves.  Every mosaic is bit for bit what isx_blender_blend gives; blenders
 * that do not qualify are blended one by one.  dsts / dst_masks: n mats (dst_masks may be NULL).                                   */
int isx_blender_blend_batch(isx_blender** bs, int n, isx_mat* dsts, isx_mat* dst_masks);

/* introspection for parity tests: copy destination pyramid level `level` (after feeds, before
 * blend) to host buffers.  lap: rows*cols*3 of int16 (I16) or float (F32/F16ACC32); weight:
 * rows*cols float.  Either may be NULL.  rows/cols are always written.                        */
int isx_blender_debug_level(isx_blender* b, int level, void* lap, float* weight,
                            int* rows, int* cols);

/* ---- mask preparation between seam finding and feed (W:286-301) ----------------------------- */
/* dilate(masks_seam[k], element) with element = getStructuringElement(MORPH_RECT, Size(kw, kh))
 * (W:286,295) followed by `& masks_warped[k]` (W:299; `other` may be NULL = dilate only).          */
int isx_mask_dilate_and(const isx_mat* mask, const isx_mat* other, int kw, int kh, isx_mat* out,
                        int device, void* hip_stream);

/* ---- exposure compensation (W:238-244) ---------------------------------------------------------- */
/* compensator->apply(i, corners[i], images_warped[i], masks_warped[i]) of the GainCompensator every demo creates
 * (W:238-239): multiply(image, gain, image) in place on a CV_8UC3 (or CV_8UC1) image, gain = gains_(i, 0) as
 * computed by compensator->feed (isx_gain_compensator_feed below).                                        */
int isx_gain_apply(isx_mat* image, double gain, int device, void* hip_stream);
/* compensator->feed(corners, images_warped, masks_warped) of GainCompensator (W:238-240, S:1165-1167, B:117-119; OpenCV 3.4.2
 * GainCompensator::feed): the overlap statistics of every pair of tiles in one GPU pass - N(i,j) = max(1, count of pixels where both
 * masks are 255) where the tiles' rectangles overlap and 0 where they do not, I(i,j) = mean of sqrt(r^2 + g^2 + b^2) of image i over
 * those pixels (0 without any; exact sums: the mean is math.fsum of the terms / N) - then
 * OpenCV's linear system (alpha = 0.01, beta = 100) solved on the host by LU with partial pivoting.  corners_xy: n (x, y) pairs;
 * images: n CV_8UC3 mats; masks: n CV_8U mats of the images' sizes; either host or device.  gains: n doubles.  n_out / i_out (may be
 * NULL): the n x n matrices N and I, row-major, I's diagonal 0.  Synchronises hip_stream (it returns host values); keeps its work table
 * (about 120 B per band of rows, on the device and pinned on the host) per calling thread between calls.
 * ISX_ERR_INVALID for num_images < 1, ISX_ERR_TYPE for other mat types, ISX_ERR_SIZE for a mask that is not its image's size. */
int isx_gain_compensator_feed(int num_images, const int* corners_xy, const isx_mat* images, const isx_mat* masks,
                              double* gains, long long* n_out, double* i_out, int device, void* hip_stream);

/* BlocksGainCompensator(bl_width = 32, bl_height = 32), what ExposureCompensator::createDefault(ExposureCompensator::GAIN_BLOCKS) returns
 * (W:238-239; OpenCV's own default in cv::Stitcher and stitching_detailed): one gain per block of every image, estimated by
 * GainCompensator::feed on the blocks as if each were an image, kept as one smoothed CV_32F gain map per image and applied through
 * cv::resize(map, image.size(), 0, 0, INTER_LINEAR).  A handle: the maps live on the device between feed and apply.  Restated from OpenCV
 * 3.4.2 (tests/helpers/blocks_gain_np.py is the model); parity with OpenCV itself is unpinned.  `device` is the HIP device;
 * create touches no device.  One handle serves one thread at a time.                                                              (W:238-244) */
typedef struct isx_blocks_gain isx_blocks_gain;
/* one pair of blocks of different images whose rectangles meet (block_i < block_j, blocks numbered image by image, rows of blocks outer):
 * N = max(1, pixels where both masks are 255), I_ij = mean of sqrt(r^2 + g^2 + b^2) of block_i's image over them, I_ji of block_j's.
 * isx_blocks_gain_stats gives the records by block_i ascending, then block_j */
typedef struct isx_block_pair {
    int block_i, block_j;
    long long n;
    double i_ij, i_ji;
} isx_block_pair;
int isx_blocks_gain_create(int bl_width, int bl_height, int device, isx_blocks_gain** out);                              /* W:238-239 */
int isx_blocks_gain_destroy(isx_blocks_gain* h);
/* compensator->feed(corners, images_warped, masks_warped) (W:238-240): the statistics of every block and of every pair of blocks that meet
 * in one GPU pass (exact sums, as isx_gain_compensator_feed), OpenCV's system assembled in its loop order, then solved ON THE DEVICE by
 * hal::LU's arithmetic (dense, partial pivoting, double, no FMA); the matrix - (blocks + 1) x blocks doubles - is freed before the
 * call returns.  images: n CV_8UC3, masks: n CV_8U of the images' sizes (255 = in), host or device.  Feeding again replaces everything.
 * ISX_ERR_UNSUPPORTED for more than 16384 blocks in total (a 2 GiB matrix), ISX_ERR_INTERNAL for a singular system, the argument errors of
 * isx_gain_compensator_feed.  Reads results back: on a capturing stream ISX_ERR_STATE with nothing enqueued.                 (W:238-244) */
int isx_blocks_gain_feed(isx_blocks_gain* h, int num_images, const int* corners_xy, const isx_mat* images, const isx_mat* masks,
                         void* hip_stream);
/* compensator->apply(index, corner, image, mask) (W:241-244; corner and mask are unused there): image(y, x) = saturate_cast<uchar>(cvRound(
 * (float)byte * g(y, x))) in place, g = map `index` resized to the image's size (INTER_LINEAR on CV_32F; the map itself when it has the
 * image's size), one launch.  image: CV_8UC3 (ISX_ERR_TYPE otherwise), host or device, any pointer and pitch, of any size - not only the
 * one fed.  ISX_ERR_STATE before feed, ISX_ERR_INVALID for an index out of range.  On a device mat it synchronises nothing and can be
 * captured; a size this handle has not seen yet uploads its tables first (on a capturing stream: ISX_ERR_STATE, nothing enqueued).
 * The tables of every size seen are kept until destroy; a graph captured before a later feed of images of the same sizes reads that
 * feed's maps (after a feed of other sizes the captured launch keeps the old grid's offset and width: capture again).        (W:238-244) */
int isx_blocks_gain_apply(isx_blocks_gain* h, int index, isx_mat* image, void* hip_stream);
/* after feed (ISX_ERR_STATE before): the number of images and of blocks; (nx, ny) per image; the raw gains, one double per block;
 * the smoothed map of one image into a caller's ny x nx CV_32FC1 mat (host: copied at once; device: enqueued on hip_stream); the
 * statistics as sparse records - the count, then up to `capacity` records (ISX_ERR_SIZE when too few; pairs may be NULL) and the diagonal
 * N, one per block (may be NULL); the host's wall-clock milliseconds of the last feed's statistics, assembly, LU and back substitution.
 * Nothing here builds a blocks x blocks array.                                                                               (W:238-244) */
int isx_blocks_gain_num_images(const isx_blocks_gain* h, int* num_images, int* num_blocks);
int isx_blocks_gain_block_counts(const isx_blocks_gain* h, int* nx_ny);
int isx_blocks_gain_gains(const isx_blocks_gain* h, double* gains);
int isx_blocks_gain_map(const isx_blocks_gain* h, int index, isx_mat* out, void* hip_stream);
int isx_blocks_gain_stats(const isx_blocks_gain* h, long long* num_pairs, isx_block_pair* pairs, long long capacity, long long* diag_n);
int isx_blocks_gain_feed_times(const isx_blocks_gain* h, double* ms4);

/* ---- the glue conversions of the reference's main() ---------------------------------- */
/* src.convertTo(dst, dst.type()) with alpha = 1, beta = 0 between the CV_8U, CV_16S and CV_32F depths, same channel count:
 * images_warped[i].convertTo(images_warped_f[i], CV_32F) (W:261), images_warped_f[k].convertTo(images_warped_s[k], CV_16S) (W:294; CV_8U ->
 * CV_16S is the two composed, exact) and result.convertTo(CV_8U) (W:315's input).  Widening is exact; narrowing is OpenCV's
 * saturate_cast (float: cvRound = round-half-even, NaN / overflow -> INT_MIN, then the clamp).  dst is caller-allocated.      */
int isx_convert_to(const isx_mat* src, isx_mat* dst, int device, void* hip_stream);

/* ---- seam finding at reduced scale: what OpenCV's stitching_detailed / Stitcher::composePanorama (3.4.2) put around the seam finder -------- */
/* cv::resize(src, dst, dst.size(), 0, 0, interpolation): the sources resized to seam_megapix before the small warp and the finder (the
 * reference's demos find their seams at full size, W:264; a caller with 4K tiles does not).  dst is caller-allocated, its rows / cols are the
 * dsize.  interpolation: ISX_INTER_NEAREST or ISX_INTER_LINEAR (ISX_ERR_UNSUPPORTED otherwise); CV_8UC1, CV_8UC3, CV_32FC1, CV_32FC3
 * (ISX_ERR_UNSUPPORTED otherwise), src and dst of one type (ISX_ERR_TYPE); an empty mat is ISX_ERR_SIZE.  Restated from OpenCV 3.4.2
 * imgproc/src/resize.cpp, plain C++ path (tests/helpers/resize_np.py is the model): NEAREST takes min(floor(d * scale), n - 1);
 * LINEAR is the 11-bit fixed point on CV_8U and float multiply-then-add on CV_32F, and the 2 x 2 area rule where src is exactly twice dst
 * in BOTH directions.  Parity with OpenCV itself is unpinned (and IPP builds of OpenCV differ by +-1 on CV_8U linear).  Host or device mats,
 * any pointer and pitch.  On device mats one launch, the taps computed in the kernel: nothing synchronises or uploads, and the call can be
 * captured; with a host mat on a capturing stream ISX_ERR_STATE, nothing enqueued.  At most 262140 rows and 2^26 columns a mat
 * (ISX_ERR_UNSUPPORTED beyond).  dst must not share a byte with src (the kernel reads the neighbours of the pixel it writes): ISX_ERR_INVALID
 * with nothing staged or enqueued where the ranges [data, data + (rows - 1) * step + cols * elemSize) of the two meet in one memory (both on
 * the host, or both on one device) - which also turns down two views side by side in one buffer, whose rows interleave; views one after
 * the other are fine.                                                                                              (between W:264 and W:302) */
int isx_resize(const isx_mat* src, isx_mat* dst, int interpolation, int device, void* hip_stream);
/* The compose loop's mask, per tile, in one launch:
 *     dilate(masks_warped[i], dilated_mask, Mat());  resize(dilated_mask, seam_mask, mask_warped.size());  mask_warped = seam_mask & mask_warped;
 * out = resize(dilate(seam_mask, MORPH_RECT kw x kh), out.size(), INTER_LINEAR) & warped_mask.  seam_mask: CV_8UC1 at seam scale; warped_mask:
 * CV_8UC1 of out's size (ISX_ERR_SIZE otherwise) or NULL = no AND; out: CV_8UC1, caller-allocated, may be warped_mask itself.  The dilate is
 * isx_mask_dilate_and's (anchor (kw / 2, kh / 2), outside pixels take no part, 1 <= kw, kh <= 4096 else ISX_ERR_INVALID; 3 x 3 is
 * dilate(.., Mat())), the resize isx_resize's CV_8U arithmetic, the AND bitwise: the result keeps the grey ramp of the resize, which is what
 * OpenCV feeds.  Byte for byte isx_mask_dilate_and(seam_mask, NULL) -> isx_resize -> AND; no intermediate mat at either scale.  Capturable
 * on device mats, as isx_resize, and with its limits.  out must not share a byte with seam_mask (isx_resize's rule and range test:
 * ISX_ERR_INVALID, nothing staged or enqueued).  out may be warped_mask - the same view: same data, step and size, where a lane reads the
 * dword it then writes - but an out that meets warped_mask's range in any other way (shifted, another pitch, a part of it) is
 * ISX_ERR_INVALID too: a lane would read bytes that another has written.                                           (between W:264 and W:302) */
int isx_mask_dilate_resize_and(const isx_mat* seam_mask, const isx_mat* warped_mask, int kw, int kh, isx_mat* out, int device, void* hip_stream);

/* ---- DP seam finder, its data-parallel part (S = 动态规划法寻找最佳缝合线.cpp) ------------------------- */
/* estimateSeam(image1, image2, tl1, tl2, comp, p1, p2, seam, isHorizontal) S:806-957 incl. computeCosts S:733-803
 * (costFunc_ COLOR, what `new DpSeamFinder(DpSeamFinder::COLOR)` W:253 / S:71-72 runs; isx_seam_estimate_cost below takes
 * the cost function): the cost maps and the dynamic programme run on the GPU, direction choice and backtracking on the host.  The component analysis around it
 * (findComponents, findEdges, resolveConflicts, getSeamTips, updateLabelsUsingSeam) stays with the caller and supplies
 * `labels` (labels_, CV_32SC1, union-sized), `label` = comp + 1, roi = {x, y, width, height} of Rect(tls_[comp],
 * brs_[comp]) and the tips p1, p2 (union coordinates).  Images: both CV_32FC3 (W:261) or both CV_8UC3.
 * seam_xy receives *seam_len points (x, y), p1 first; *seam_len = 0 when p2 is not reachable (`return false`).   */
int isx_seam_estimate(const isx_mat* image1, const isx_mat* image2, int tl1_x, int tl1_y, int tl2_x, int tl2_y,
                      int union_tl_x, int union_tl_y, const isx_mat* labels, int label, const int roi[4],
                      int p1_x, int p1_y, int p2_x, int p2_y, int* seam_xy, int cap, int* seam_len,
                      int* is_horizontal, int device, void* hip_stream);
/* DpSeamFinder::CostFunction (S:71) */
enum { ISX_DP_COLOR = 0, ISX_DP_COLOR_GRAD = 1 };
/* isx_seam_estimate with costFunc_ as an argument; isx_seam_estimate is its ISX_DP_COLOR case.  ISX_DP_COLOR_GRAD (what
 * `new DpSeamFinder(DpSeamFinder::COLOR_GRAD)` W:255 / S:1183 runs): computeGradients S:549-572 (cvtColor(COLOR_BGR2GRAY) + two 3 x 3
 * Sobels per image, BORDER_REFLECT_101 at the image's own edges) evaluated over the component's rectangle, and both cost loops'
 * COLOR_GRAD branches S:767-772 / S:792-797: a cell is costColor / costGrad, costGrad = the four |gradients| next to the cell + 1
 * (evaluation order and OpenCV parity: DESIGN.md §8).  Any other cost_func -> ISX_ERR_INVALID.                          */
int isx_seam_estimate_cost(const isx_mat* image1, const isx_mat* image2, int tl1_x, int tl1_y, int tl2_x, int tl2_y,
                           int union_tl_x, int union_tl_y, const isx_mat* labels, int label, const int roi[4],
                           int p1_x, int p1_y, int p2_x, int p2_y, int* seam_xy, int cap, int* seam_len,
                           int* is_horizontal, int cost_func, int device, void* hip_stream);
/* The gradient maps of computeGradients S:549-572 for one image, as magnitudes (all S:769-770 / S:794-795 read): abs_gradx =
 * |Sobel(gray, CV_32F, 1, 0)| (S:562, S:570), abs_grady = |Sobel(gray, CV_32F, 0, 1)| (S:563, S:571), gray =
 * cvtColor(image, COLOR_BGR2GRAY) (S:558, S:566), over rect = {x, y, width, height} of the image.  The values are those of
 * the whole image's maps (borders reflect at the image's edges, not the rectangle's).  image: CV_32FC3 or CV_8UC3; outputs:
 * caller-allocated CV_32FC1 of the rectangle's size; host or device mats.                                                */
int isx_seam_gradients(const isx_mat* image, const int rect[4], isx_mat* abs_gradx, isx_mat* abs_grady, int device,
                       void* hip_stream);

/* seam_finder->find(images_warped_f, corners, masks_seam) of the in-tree DP seam finder as a whole (S:87-124 `find`, as
 * the S demo calls it at S:1192; W:253 is the stock `DpSeamFinder(DpSeamFinder::COLOR)` it restates): every pair of
 * images, last pair first; component / contour / graph logic on the host, the cost maps and the dynamic programme of every
 * estimateSeam on the GPU.  images: n mats, all CV_32FC3 (W:261) or all CV_8UC3, host or device; masks: n CV_8UC1 mats
 * of the images' sizes, edited in place.                                                                            */
int isx_dp_seam_find(int num_images, const isx_mat* images, const int* corners_xy, isx_mat* masks, int device,
                     void* hip_stream);
/* isx_dp_seam_find with the finder's cost function (S:71-72; process -> resolveConflicts S:398-399 -> estimateSeam ->
 * computeCosts S:765-772, S:790-797): ISX_DP_COLOR is isx_dp_seam_find itself, ISX_DP_COLOR_GRAD the `new
 * DpSeamFinder(DpSeamFinder::COLOR_GRAD)` every demo lists as the alternative (W:255, S:1183).  Any other cost_func ->
 * ISX_ERR_INVALID, the masks untouched.                                                                              */
int isx_dp_seam_find_cost(int num_images, const isx_mat* images, const int* corners_xy, isx_mat* masks, int cost_func,
                          int device, void* hip_stream);
/* isx_dp_seam_find / isx_seam_estimate (and their _cost forms, isx_seam_gradients) keep their work images (about 6-10 B per union
 * pixel on the host, the staged images, gradient maps, cost maps and DP records on the device) per calling thread between calls; this returns all of it (the analogue of the
 * DpSeamFinder going out of scope, S:1188-1192).  PER THREAD: the state is thread-local and is NOT freed when a thread ends (the
 * HIP runtime may already be gone then) - a thread-pool caller calls this on every worker thread before that thread exits, or
 * leaks one finder (tens of MB at 4K) per thread.                                                                    */
int isx_dp_seam_release(void);

/* ---- the stock graph-cut seam finder of the W demo (W:257, W:264) ----------------------------------------------------------- */
/* GraphCutSeamFinder::CostType */
enum { ISX_GC_COST_COLOR = 0, ISX_GC_COST_COLOR_GRAD = 1 };
/* seam_finder = new GraphCutSeamFinder(GraphCutSeamFinder::COST_COLOR) (W:257); seam_finder->find(images_warped_f, corners, masks_warped)
 * (W:264), OpenCV 3.4.2's PairwiseSeamFinder + GraphCutSeamFinder::Impl restated (OpenCV parity unpinned): for every pair
 * i < j (outer i, inner j) whose overlapRoi is not empty, on the masks as the earlier pairs left them, a max-flow over the padded overlap
 * ((roi.h + 20) x (roi.w + 20) nodes) on the GPU, and the write-back over the roi.  The cut is the MAXIMAL source side of a maximum flow
 * (the nodes that cannot reach the sink in its residual graph): unique, so the masks do not depend on the schedule.  Where the minimum cut
 * is not unique OpenCV's Boykov-Kolmogorov search may choose another cut of the same cost.
 * images: n mats, all CV_32FC3 (W:261: convertTo of the byte tiles) or all CV_8UC3, host or device; CV_32FC3 values must be integers in
 * [0, 255] (then every capacity is an exact integer): any other value gives ISX_ERR_UNSUPPORTED before a mask is written.  masks: n CV_8UC1
 * mats of the images' sizes, host or device, edited in place.
 * cost_type ISX_GC_COST_COLOR, or ISX_GC_COST_COLOR_GRAD (setGraphWeightsColorGrad; CV_32FC3 tiles only, CV_8UC3 tiles give
 * ISX_ERR_UNSUPPORTED with the masks untouched): every edge weight becomes (|d(p)|^2 + |d(q)|^2) / grad + 1.f (+ 1000.f), grad = dx1(p) +
 * dx1(q) + dx2(p) + dx2(q) + 1.f for a right edge and the same of dy for a down edge, dx_ / dy_ the squared norm over the three channels of
 * the tile's 3 x 3 Sobel derivatives (BORDER_REFLECT_101 at the tile's edges, 0 outside the tile).  On integer tiles that float is a
 * multiple of 2^-23, so the capacities are exact int64 in units of 2^-23 (Q23; terminals 10000 * 2^23) and the cut is as unique as
 * COST_COLOR's.  A pair whose padded grid has more than 2^26 nodes gives ISX_ERR_UNSUPPORTED before anything is launched.
 * Fewer than 2 images: nothing to do.  Synchronises hip_stream (it reads counters back every round), so a capturing
 * stream gives ISX_ERR_STATE.  A pair whose max-flow does not finish within 4096 rounds (16 push-relabel sweeps and a global relabel
 * each) gives ISX_ERR_UNSUPPORTED with that pair's masks untouched; the pairs before it keep their edits.                              */
int isx_graphcut_seam_find(int num_images, const isx_mat* images, const int* corners_xy, isx_mat* masks, int cost_type, int device,
                           void* hip_stream);
/* One pair (images 1 and 2 at corners_xy[0..1] and corners_xy[2..3]) as isx_graphcut_seam_find treats it, optionally returning a
 * certificate of its maximum flow over the padded grid of rows x cols = info[0] x info[1] nodes (row-major, node (y, x) = grid row y,
 * column x; grid (10, 10) is the roi's top-left):
 *   flow       (may be NULL) the maximum flow value (without OpenCV's constant 10000 per node that has both masks); with
 *              ISX_GC_COST_COLOR_GRAD in units of 2^-23
 *   residuals  (may be NULL, with labels) cert_nodes >= rows * cols records of 6 int32 per node: the residual capacities of its edges
 *              to the right, to the left, down, up (0 where the grid ends), of the source's link to it and of its link to the sink;
 *              every edge of weight w has r(u -> v) + r(v -> u) = 2 w
 *   labels     rows * cols bytes: 1 = source side (the maximal one), 0 = sink side
 *   info       (may be NULL) 4 ints: rows, cols, push-relabel rounds, kernel launches; all 0 when the tiles do not overlap
 * ISX_ERR_SIZE when cert_nodes is too small (nothing written).  With ISX_GC_COST_COLOR_GRAD the residuals do not fit 32 bits: residuals
 * must be NULL (ISX_ERR_INVALID otherwise); isx_graphcut_seam_find_pair64 returns them. */
int isx_graphcut_seam_find_pair(const isx_mat* image1, const isx_mat* image2, const int* corners_xy, isx_mat* mask1, isx_mat* mask2,
                                int cost_type, long long* flow, int* residuals, unsigned char* labels, long long cert_nodes, int* info,
                                int device, void* hip_stream);
/* isx_graphcut_seam_find_pair with 6 int64 residuals per node, same order, for either cost type: ISX_GC_COST_COLOR's are the int32 ones
 * widened, ISX_GC_COST_COLOR_GRAD's are in units of 2^-23 (an edge of weight w has r(u -> v) + r(v -> u) = 2 * w * 2^23). */
int isx_graphcut_seam_find_pair64(const isx_mat* image1, const isx_mat* image2, const int* corners_xy, isx_mat* mask1, isx_mat* mask2,
                                  int cost_type, long long* flow, long long* residuals, unsigned char* labels, long long cert_nodes, int* info,
                                  int device, void* hip_stream);
/* The graph-cut finder keeps its graph (28 B per padded node on the device, 48 B with ISX_GC_COST_COLOR_GRAD), counters and staged host mats per calling thread between
 * calls; this returns them.  PER THREAD and not freed at thread exit, as for isx_dp_seam_release.                                      */
int isx_graphcut_seam_release(void);

/* ---- the Voronoi seam finder of the S demo (S:1180, S:1192) ------------------------------------------------------------------ */
/* seam_finder = makePtr<detail::VoronoiSeamFinder>() (S:1180); seam_finder->find(images_warped_f, corners, masks_seam) (S:1192), OpenCV
 * 3.4.2's PairwiseSeamFinder + VoronoiSeamFinder::findInPair restated (OpenCV parity unpinned): for every pair i < j (outer
 * i, inner j) whose overlapRoi is not empty, on the masks as the earlier pairs left them: the two masks' windows over the roi and a gap of
 * 10 cells around it (0 outside a tile), the cells both cover removed from each, distanceTransform(DIST_L1, 3) to what is left of each,
 * and over the roi mask2 = 0 where dist1 < dist2 (compared as the floats the transform returns), mask1 = 0 elsewhere - ties and "neither
 * tile has a cell of its own" included.  Pixels are never read: sizes_wh holds (width, height) per image.
 * masks: n CV_8UC1 mats, host or device, any pointer alignment and step, edited in place.  Checked before the first pair writes: null
 * pointers or a negative size -> ISX_ERR_INVALID; a mask that is not CV_8UC1 -> ISX_ERR_TYPE; a mask whose rows / cols differ from
 * sizes_wh -> ISX_ERR_SIZE; an overlap that passes 32768 cells a side with its gap -> ISX_ERR_UNSUPPORTED.  Fewer than 2 images: nothing
 * to do.
 * Device masks: three kernels per pair are enqueued on hip_stream, nothing is synchronised or read back, and the call works on a
 * capturing stream.  Host masks are staged to the device and back, which synchronises: on a capturing stream -> ISX_ERR_STATE with nothing
 * enqueued.  The scratch (about 8 B per cell of the largest padded overlap) is kept per calling thread and grows only outside a capture:
 * a captured call that needs more than it holds -> ISX_ERR_STATE with nothing enqueued (isx_voronoi_seam_reserve first).               */
int isx_voronoi_seam_find(int num_images, const int* sizes_wh, const int* corners_xy, isx_mat* masks, int device, void* hip_stream);
/* Sizes the calling thread's scratch for overlaps of up to max_roi_width x max_roi_height (the roi, without the gap) ahead of a stream
 * capture (S:1180: the finder's construction).  A captured graph keeps pointing at this scratch: growing it (a larger reserve or find
 * outside the capture, another device) or releasing it while such a graph exists is the caller's error.                                */
int isx_voronoi_seam_reserve(int max_roi_width, int max_roi_height, int device);
/* Returns the scratch and the staged host masks of the calling thread (the finder going out of scope, S:1192).  PER THREAD and not
 * freed at thread exit, as for isx_dp_seam_release.                                                                                    */
int isx_voronoi_seam_release(void);

/* ---- the features finder of the F demo (F = the reference's 特征点检测/特征点检测/特征点检测.cpp) --------------------------------- */
/* Limits and room (orb.hip takes them from here; tests/helpers/orb_np.py repeats them): pyramid levels; the ties a (cell, level) keeps past
 * 2 n_l candidates after the first cut and past n_l keypoints after the final one; the candidates one workgroup ranks; (cell, level)
 * layers; pixels a side.                                                                                                                */
enum { ISX_ORB_MAX_LEVELS = 8, ISX_ORB_CAND_TIE_ROOM = 256, ISX_ORB_KEEP_TIE_ROOM = 32, ISX_ORB_MAX_CANDIDATES = 4096,
       ISX_ORB_MAX_LAYERS = 1024, ISX_ORB_MAX_SIDE = 16384 };
/* status bits of count_status[1] */
enum { ISX_ORB_TRUNCATED = 1,     /* a set had more ties at its cut than room: the first in canonical order were kept            */
       ISX_ORB_BAD_PATTERN = 2 }; /* a DEVICE pattern holds a point with |x| or |y| > 15: count is 0 and no row is written      */
enum { ISX_ORB_HARRIS_SCORE = 0, ISX_ORB_FAST_SCORE = 1 };      /* cv::ORB::HARRIS_SCORE, FAST_SCORE */
/* OrbFeaturesFinder(grid_size, n_features, scaleFactor, nlevels) (F:40-44) and the ORB::create arguments F:45-54 fixes. */
typedef struct isx_orb_params {
    int   grid_width, grid_height; /* F:54: Size(3, 1)                                                                      */
    int   n_features;              /* 1500; a cell finds n_features * (99 + area) / 100 / area (F:43): 510                  */
    float scale_factor;            /* 1.3f, widened to double as `double scaleFactor = 1.3f` does (F:45); > 1                */
    int   nlevels;                 /* 5 (F:46); 1 .. ISX_ORB_MAX_LEVELS                                                     */
    int   edge_threshold;          /* 31 (F:47)   other values: ISX_ERR_UNSUPPORTED                                         */
    int   first_level;             /* 0 (F:48)    other values: ISX_ERR_UNSUPPORTED                                         */
    int   wta_k;                   /* 2 (F:49)    other values: ISX_ERR_UNSUPPORTED                                         */
    int   score_type;              /* ISX_ORB_HARRIS_SCORE (F:50); FAST_SCORE: ISX_ERR_UNSUPPORTED                          */
    int   patch_size;              /* 31 (F:51)   other values: ISX_ERR_UNSUPPORTED                                         */
    int   fast_threshold;          /* 20 (F:52); 1 .. 254                                                                   */
} isx_orb_params;
/* The defaults above. */
int isx_orb_default_params(isx_orb_params* params);
/* The rows a call's outputs need: cells * sum over levels of (n_l + ISX_ORB_KEEP_TIE_ROOM), n_l as F:72-82 gives it.  The parameter checks
 * of isx_orb_find. */
int isx_orb_capacity(const isx_orb_params* params, int* capacity);
/* makeRandomPattern(31) (F:709-718) on the restated cv::RNG of isx_find_homography, seed 0x34985739: 512 (x, y) points into a HOST CV_32SC1
 * mat of at least 512 x 2.  It is what a NULL pattern means.  The reference's learned table bit_pattern_31_ (F:355-706) exists as program
 * text only and is not part of this library: a caller who has OpenCV passes it as `pattern`.                                              */
int isx_orb_default_pattern(isx_mat* pattern);
/* OrbFeaturesFinder::find (F:948-1017) = per grid cell detectAndCompute (F:727-946): computeKeyPoints (F:56-191), HarrisResponses
 * (F:204-246), ICAngles (F:250-283), computeOrbDescriptors (F:287-353).  The specification is tests/helpers/orb_np.py, which the kernels
 * match bit for bit (DESIGN.md §8 "Features finder" lists what is restated, decided and unpinned):
 *   gray        (B*1868 + G*9617 + R*4899 + 8192) >> 14 (F:956-964); CV_8UC1 passes through, CV_8UC4 ignores alpha.
 *   cells       F:984-987's integer bounds; every cell is found on its own and xl, yl are added to pt afterwards (F:1006-1007).
 *   pyramid     layer l is cvRound(cols / scale) x cvRound(rows / scale), scale = (float)pow(scaleFactor, l) (F:792-794), resized from layer
 *               l - 1 by isx_resize's INTER_LINEAR on CV_8U (F:834 asks for INTER_LINEAR_EXACT: a departure).  No border is built (F:842-851):
 *               every keypoint lies 31 px inside its layer and no reader goes further than 25.
 *   FAST        FastFeatureDetector::create(fast_threshold, true) (F:118-119) restated: score = max(a, -b) - 1 over the 16 arcs of 9, a corner
 *               where score >= threshold, kept where its score is strictly greater than its 8 neighbours'.
 *   cuts        runByImageBorder(31) (F:123), retainBest(2 n_l) by FAST score (F:126), Harris block 7, k = 0.04f (F:155), retainBest(n_l)
 *               (F:172); retainBest keeps every point >= the n-th largest.  Points strictly above a cut always fit; its ties fill
 *               ISX_ORB_CAND_TIE_ROOM / ISX_ORB_KEEP_TIE_ROOM rows in canonical order; dropped ties set ISX_ORB_TRUNCATED.
 *   angle       the moments of F:261-280 through the restated atan2f (csrc/proj_math.hpp) in degrees, [0, 360) (F:281 calls fastAtan2).
 *   descriptor  F:299-352 on the layer blurred 7 x 7, sigma 2 in exact integers (F:936; Q8 taps 18 34 49 54 49 34 18), the restated
 *               cosf / sinf, WTA_K = 2, 32 bytes.
 *   order       cell (row-major), level, y, x.  (OpenCV's own order is what nth_element leaves.)
 *   image        CV_8UC1, CV_8UC3 or CV_8UC4, host or device, any pointer alignment and step, 1 .. ISX_ORB_MAX_SIDE pixels a side.
 *   pattern      NULL, or a CV_32SC1 mat of 512 x 2, host or device, 4-byte aligned.  A host pattern with |x| or |y| > 15 is refused
 *                (ISX_ERR_INVALID); a device pattern is checked by the kernel that reads it (ISX_ORB_BAD_PATTERN).
 *   keypoints    CV_32FC1, at least cap x 2: pt.x, pt.y - the layout isx_match_features takes.      cap = isx_orb_capacity(params)
 *   meta         CV_32FC1, at least cap x 4: size (31 scale), angle, response (Harris), octave.
 *   descriptors  CV_8UC1, at least cap x 32, any pointer alignment and step.
 *   count_status CV_32SC1, at least 1 x 2: the number of keypoints, the status bits.  Rows from count on are not written.
 * keypoints, meta and count_status are 4-byte aligned in pointer and step.  Checked before anything is written or enqueued: null pointers,
 * a parameter out of range, a grid finer than the image, a misaligned mat, a bad host pattern -> ISX_ERR_INVALID; the parameters F fixes at
 * another value, more than ISX_ORB_MAX_CANDIDATES candidates a layer (2 n_0 + ISX_ORB_CAND_TIE_ROOM), more than ISX_ORB_MAX_LAYERS layers,
 * a side past ISX_ORB_MAX_SIDE -> ISX_ERR_UNSUPPORTED; a mat of another type -> ISX_ERR_TYPE; an empty image, a pattern that is not
 * 512 x 2, too few rows or columns -> ISX_ERR_SIZE.
 * With device mats throughout nothing is read back or synchronised: count_status stays on the device.  Host mats synchronise.  On a
 * capturing stream the call works with device mats once isx_orb_reserve has sized the scratch (the default pattern then lies there); a host
 * mat, or a call that would have to grow the scratch, -> ISX_ERR_STATE with nothing enqueued.  The launch count depends on nlevels only.  */
int isx_orb_find(const isx_mat* image, const isx_orb_params* params, const isx_mat* pattern, isx_mat* keypoints, isx_mat* meta,
                 isx_mat* descriptors, isx_mat* count_status, int device, void* hip_stream);
/* Sizes the calling thread's scratch for device images of up to width x height under `params` and uploads the default pattern, ahead of a
 * stream capture.  A captured graph keeps pointing at this scratch: growing or releasing it while such a graph exists is the caller's
 * error.                                                                                                                                  */
int isx_orb_reserve(const isx_orb_params* params, int width, int height, int device);
/* Returns the scratch of the calling thread.  PER THREAD and not freed at thread exit, as for isx_match_release.                          */
int isx_orb_release(void);

/* ---- the features finder every main of the reference comments out: `//finder = new SurfFeaturesFinder();` (B:37, C:296, S:1104) ------- */
/* Limits (surf.hip takes them from here; tests/helpers/surf_np.py repeats them): the maxima that are ranked; pixels a side; pixels.     */
enum { ISX_SURF_MAX_CANDIDATES = 32768, ISX_SURF_MAX_SIDE = 16384, ISX_SURF_MAX_PIXELS = 1 << 24,
       ISX_SURF_MAX_OCTAVES = 4, ISX_SURF_MAX_LAYERS = 4 };
/* status bits of count_status[1] */
enum { ISX_SURF_TRUNCATED = 1,            /* more keypoints than cap: the first cap in canonical order (strongest first) were written      */
       ISX_SURF_CANDIDATES_DROPPED = 2 }; /* more than ISX_SURF_MAX_CANDIDATES maxima: the first in scan order (octave, layer, y, x) ranked */
/* SurfFeaturesFinder(hess_thresh, num_octaves, num_layers, num_octaves_descr, num_layers_descr) of OpenCV 3.4.2's stitching module.      */
typedef struct isx_surf_params {
    double hess_thresh;            /* 300; >= 0, compared as (float)                                                         */
    int    num_octaves;            /* 3; 1 .. ISX_SURF_MAX_OCTAVES                                                           */
    int    num_layers;             /* 4; 1 .. ISX_SURF_MAX_LAYERS                                                            */
    int    num_octaves_descr;      /* 3; any value but num_octaves: ISX_ERR_UNSUPPORTED (one detectAndCompute)               */
    int    num_layers_descr;       /* 4; any value but num_layers: ISX_ERR_UNSUPPORTED                                       */
    int    extended;               /* 0; non-zero (128 floats): ISX_ERR_UNSUPPORTED                                          */
    int    upright;                /* 0; non-zero: ISX_ERR_UNSUPPORTED                                                       */
} isx_surf_params;
/* The defaults above. */
int isx_surf_default_params(isx_surf_params* params);
/* SurfFeaturesFinder::find = SURF::detectAndCompute(image, no mask) with extended = false, upright = false.  OpenCV's source is in neither
 * tree: the specification is tests/helpers/surf_np.py, which the kernels match bit for bit, and OpenCV parity is UNPINNED (DESIGN.md §8
 * "Features finder, SURF" lists what is decided).
 *   gray        as isx_orb_find.
 *   integral    (rows + 1) x (cols + 1), unsigned 32-bit with wrapping adds; box differences are exact.
 *   Hessian     octave o < num_octaves, layer l < num_layers + 2: filter (9 + 6 l) << o at step 1 << o; det = dx dy - 0.81f dxy dxy.
 *   maxima      det > (float)hess_thresh and strictly above its 26 neighbours, then interpolateKeypoint (Cramer's rule in float32).
 *   order       response, size, octave, pt.y, pt.x descending (KeypointGreater), then the scan index (octave, layer, y, x) ascending.
 *   angle       113 Haar samples, a 60 degree window every 5 degrees, through the restated atan2f in degrees, [0, 360).
 *   descriptor  the rotated window walked as OpenCV accumulates it, INTER_AREA to 21 x 21 by the general table, 4 x 4 cells of
 *               (sum dx, sum dy, sum |dx|, sum |dy|), normalised: 64 floats.
 *   image        CV_8UC1, CV_8UC3 or CV_8UC4, host or device, any pointer alignment and step, at most ISX_SURF_MAX_SIDE pixels a side and
 *                ISX_SURF_MAX_PIXELS pixels.
 *   keypoints    CV_32FC1, cap x 2: pt.x, pt.y - the layout the matchers take.
 *   meta         CV_32FC1, cap x 5: size, angle, response, octave, laplacian (the sign of the trace).
 *   descriptors  CV_32FC1, cap x 64 - the layout isx_match_features_f32 takes.
 *   count_status CV_32SC1, at least 1 x 2: the number of keypoints, the status bits.  Rows from count on are not written.
 * cap is the caller's: the smallest row count of keypoints, meta and descriptors, at least 1 (ISX_ERR_SIZE).  Every output is 4-byte
 * aligned in pointer and step.  Checked before anything is written or enqueued: null pointers, a parameter out of range, a misaligned mat
 * -> ISX_ERR_INVALID; another descriptor octave / layer pair, extended, upright, a side or a pixel count past its limit ->
 * ISX_ERR_UNSUPPORTED; a mat of another type -> ISX_ERR_TYPE; an empty image, too few rows or columns -> ISX_ERR_SIZE.
 * With device mats throughout nothing is read back or synchronised.  Host mats synchronise.  On a capturing stream the call works with
 * device mats once isx_surf_reserve has sized the scratch; a host mat, or a call that would have to grow the scratch, -> ISX_ERR_STATE
 * with nothing enqueued.  The launch count depends on num_octaves only.                                                                  */
int isx_surf_find(const isx_mat* image, const isx_surf_params* params, isx_mat* keypoints, isx_mat* meta, isx_mat* descriptors,
                  isx_mat* count_status, int device, void* hip_stream);
/* Sizes the calling thread's scratch for device images of up to width x height under `params` and device outputs of `cap` rows, ahead of
 * a stream capture.  A captured graph keeps pointing at this scratch: growing or releasing it while such a graph exists is the caller's
 * error.                                                                                                                                  */
int isx_surf_reserve(const isx_surf_params* params, int width, int height, int cap, int device);
/* Returns the scratch of the calling thread.  PER THREAD and not freed at thread exit, as for isx_orb_release.                           */
int isx_surf_release(void);

/* ---- the third finder cv::Stitcher and stitching_detailed --features sift offer: SIFT, 128 floats a keypoint ------------------------- */
/* Limits (sift.hip takes them from here; tests/helpers/sift_np.py repeats them): the candidates that are ranked; source pixels a side;
 * source pixels (a 3840 x 2160 frame fits).  The doubled pyramid of ISX_SIFT_MAX_PIXELS source pixels is about 2 GiB of scratch: six
 * Gaussian and five DoG layers an octave and one row-pass buffer, float32, at four times the source's pixels in the first octave.      */
enum { ISX_SIFT_MAX_CANDIDATES = 32768, ISX_SIFT_MAX_SIDE = 8192, ISX_SIFT_MAX_PIXELS = 1 << 23 };
/* status bits of count_status[1] */
enum { ISX_SIFT_TRUNCATED = 1,            /* more keypoints than cap: the first cap in canonical order (strongest first) were written       */
       ISX_SIFT_CANDIDATES_DROPPED = 2 }; /* more than ISX_SIFT_MAX_CANDIDATES candidates: the first in scan order (octave, layer, r, c) kept */
/* SIFT::create(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma) of OpenCV 4.x.                                         */
typedef struct isx_sift_params {
    int    nfeatures;              /* 0: all; > 0: the strongest nfeatures (no keep-the-ties rule); < 0: ISX_ERR_INVALID       */
    int    n_octave_layers;        /* 3; any other value: ISX_ERR_UNSUPPORTED (the blur taps are committed tables)             */
    double contrast_threshold;     /* 0.04; in [0, 3e38], compared as (float)                                                  */
    double edge_threshold;         /* 10; in (0, 3e38], compared as (float)                                                    */
    double sigma;                  /* 1.6; any other value: ISX_ERR_UNSUPPORTED                                                */
} isx_sift_params;
/* The defaults above. */
int isx_sift_default_params(isx_sift_params* params);
/* SIFT::detectAndCompute(image, noArray()) (float DoG, SIFT_FIXPT_SCALE 1, firstOctave -1).  OpenCV's source is in neither tree: the
 * specification is tests/helpers/sift_np.py, which the kernels match bit for bit, and OpenCV parity is UNPINNED (DESIGN.md §8 "Features
 * finder, SIFT" lists what is decided).
 *   gray        as isx_orb_find, converted to float32.
 *   base        resize to (2 cols, 2 rows) with the CV_32F INTER_LINEAR taps of isx_resize, blurred by sqrt(1.6^2 - 1).
 *   octaves     the largest c with 2^(2 c + 1) <= m^2, m the smaller side of the doubled image (cvRound(log2 m - 2) + 1 in integers); an
 *               octave narrower than 11 pixels either way and every octave after it are not built.
 *   pyramid     6 Gaussian layers an octave, each a separable blur of the one before (committed taps, BORDER_REFLECT_101 repeated, rows
 *               first, the symmetric sum order); the next octave starts from layer 3 at (2 x, 2 y); 5 DoG layers.
 *   extrema     |v| > floor(0.5 contrast_threshold / 3 * 255) and v >= (v > 0) or <= (v < 0) its 26 neighbours, 5 pixels inside, then
 *               adjustLocalExtrema (Cramer's rule in float32, at most 5 steps, the contrast and the edge tests).
 *   duplicates  a candidate is removed when an earlier one in scan order ends on the same (octave, layer, r, c).
 *   order       response, size, octave, pt.y, pt.x descending, then the scan index (octave, layer, r, c of the starting pixel) ascending;
 *               keypoints follow their candidate's rank, then the ascending bin of the orientation histogram.
 *   angle       36 bins, each summed in sample order, through the restated atan2f in degrees and sift_math.hpp's expf; one keypoint a peak.
 *   descriptor  4 x 4 x 8 trilinear, each cell summed in sample order, clipped at 0.2, scaled by 512, rounded to 0 .. 255: 128 floats.
 *   image        CV_8UC1, CV_8UC3 or CV_8UC4, host or device, any pointer alignment and step, at most ISX_SIFT_MAX_SIDE pixels a side and
 *                ISX_SIFT_MAX_PIXELS pixels.
 *   keypoints    CV_32FC1, cap x 2: pt.x, pt.y in source pixels - the layout the matchers take.
 *   meta         CV_32FC1, cap x 5: size, angle, response, octave (-1 upward), layer (1 .. 3).
 *   descriptors  CV_32FC1, cap x 128 - the layout isx_match_features_f32 takes.
 *   count_status CV_32SC1, at least 1 x 2: the number of keypoints, the status bits.  Rows from count on are not written.
 * cap is the caller's: the smallest row count of keypoints, meta and descriptors, at least 1 (ISX_ERR_SIZE).  count =
 * min(total, nfeatures if nfeatures > 0, cap); ISX_SIFT_TRUNCATED when cap cut it.  Every output is 4-byte aligned in pointer and step.
 * Checked before anything is written or enqueued: null pointers, a parameter out of range or NaN, a misaligned mat -> ISX_ERR_INVALID;
 * another n_octave_layers or sigma, a side or a pixel count past its limit -> ISX_ERR_UNSUPPORTED; a mat of another type -> ISX_ERR_TYPE;
 * an empty image, too few rows or columns -> ISX_ERR_SIZE.
 * With device mats throughout nothing is read back or synchronised.  Host mats synchronise.  On a capturing stream the call works with
 * device mats once isx_sift_reserve has sized the scratch; a host mat, or a call that would have to grow the scratch, -> ISX_ERR_STATE
 * with nothing enqueued.  The launch count depends on the image size only: 10 + 11 n - (n > 0) for n built octaves.                     */
int isx_sift_find(const isx_mat* image, const isx_sift_params* params, isx_mat* keypoints, isx_mat* meta, isx_mat* descriptors,
                  isx_mat* count_status, int device, void* hip_stream);
/* Sizes the calling thread's scratch for device images of up to width x height under `params` and device outputs of `cap` rows, ahead of
 * a stream capture.  A captured graph keeps pointing at this scratch: growing or releasing it while such a graph exists is the caller's
 * error.                                                                                                                                  */
int isx_sift_reserve(const isx_sift_params* params, int width, int height, int cap, int device);
/* Returns the scratch of the calling thread.  PER THREAD and not freed at thread exit, as for isx_orb_release.                           */
int isx_sift_release(void);

/* ---- the features matcher of the M demo (M = the reference's 特征点匹配/特征点匹配/特征点匹配.cpp) --------------------------------- */
/* The tiling of the search kernel (match.hip takes them from here; imagestitch_amd/matcher.py repeats them): queries per block, train rows
 * per LDS tile, train rows per work item, and the row limits - the width of the packed key distance << 22 | row.                          */
enum { ISX_MATCH_QUERY_BLOCK = 128, ISX_MATCH_TRAIN_TILE = 128, ISX_MATCH_TRAIN_CHUNK = 256,
       ISX_MATCH_MAX_ROWS = 1 << 20, ISX_MATCH_MAX_TOTAL_ROWS = 1 << 22 };
/* isx_match_features_f32 shares the query block, the chunk plan and the row limits; its LDS tile holds fewer (wider) rows, and a row has
 * at most ISX_MATCH_F32_MAX_COLS floats.                                                                                                 */
enum { ISX_MATCH_F32_TRAIN_TILE = 32, ISX_MATCH_F32_MAX_COLS = 128 };
/* BestOf2NearestMatcher1 matcher(false, match_conf, ...); matcher(features, pairwise_matches) (M:307-308) up to where M:158 returns, plus
 * the point gather of M:164-179: for every pair of near_pairs (M:131-135) CpuMatcher1::match (M:232-289) with an EXACT 2-nearest-neighbour
 * search over 256-bit Hamming distances in place of the FLANN LSH index of M:241-250 (approximate and randomised: not reproduced).
 *   1->2 (M:256-274): with n_to >= 2, the two nearest rows of image `to` by (distance, row) for every row q of image `from`; accepted when
 *        (float)d0 < k * (float)d1, k = 1.f - match_conf in float32, one rounded multiply; appended as (q, row0, d0) in order of q.
 *   2->1 (M:276-287): the same with the roles swapped, with n_from >= 2; appended as (row0, q, d0) in order of q unless 1->2 accepted
 *        (row0, q).
 * An accepted match has a unique nearest neighbour (d0 < k d1 <= d1), so the list does not depend on how ties are ordered.  A pair with an
 * empty image is skipped: its count is 0 and nothing else of it is written (M:134).  homography, inliers and confidence (M:181-229) are
 * isx_find_homography's, which reads `points` and `counts` where this call leaves them.
 *   descriptors  num_images CV_8UC1 mats of n_i x 32 (ORB; cols != 32 -> ISX_ERR_UNSUPPORTED; CV_32F descriptors go to isx_match_features_f32), host or
 *                device, any pointer alignment and step; rows may be 0 (then data and cols are not looked at).  At most 2^20 rows an
 *                image and 2^22 in all (ISX_ERR_UNSUPPORTED).
 *   keypoints    NULL, or num_images CV_32FC1 mats of n_i x 2 (pt.x, pt.y); then image_sizes_wh holds (width, height) per image (img_size).
 *   pairs_ij     num_pairs (from, to) with from < to.
 *   matches      per pair a CV_32SC1 mat of at least (n_from + n_to) x 3: queryIdx, trainIdx, distance.  Rows from counts[p] on are not
 *                written.
 *   points       NULL, or (with keypoints) per pair a CV_32FC1 mat of at least (n_from + n_to) x 4: row r = src.x, src.y, dst.x, dst.y of
 *                match r, each pt - size * 0.5f in float32 (M:170-178).
 *   counts       a CV_32SC1 mat of at least 1 x num_pairs.
 *   knn          NULL, or 2 * num_pairs CV_32SC1 mats (pair p: 2p is 1->2, 2p + 1 is 2->1) of at least n_query x 4: row0, d0, row1, d1, with -1, -1
 *                where there is no such neighbour.  Not written for a skipped pair.
 *   info         NULL, or 2 ints: the pairs searched and the kernel launches of this call (at most three, however many pairs).
 * Output mats are host or device mats, 4-byte aligned in pointer and step.  Checked before anything is written or enqueued: null pointers,
 * num_images < 0, a pair with from >= to or out of range, match_conf not in [0, 1) (outside it the list would depend on the order of ties),
 * keypoints without image_sizes_wh, points without keypoints, a misaligned output -> ISX_ERR_INVALID; descriptors not CV_8UC1, keypoints or
 * points not CV_32FC1, matches / counts / knn not CV_32SC1 -> ISX_ERR_TYPE; an output with too few rows or cols, keypoints that are not
 * n_i x 2 -> ISX_ERR_SIZE.  The call uploads its tables (and packs and stages host mats): on a capturing stream -> ISX_ERR_STATE with nothing
 * enqueued.  With device mats throughout nothing is read back or synchronised: counts stays on the device.  Host mats synchronise.         */
int isx_match_features(int num_images, const isx_mat* descriptors, const isx_mat* keypoints, const int* image_sizes_wh,
                       int num_pairs, const int* pairs_ij, float match_conf, isx_mat* matches, isx_mat* points, isx_mat* counts,
                       isx_mat* knn, int* info, int device, void* hip_stream);
/* The same call over CV_32F descriptors (SURF 64 / 128, SIFT 128, learned ones; CpuMatcher1::match admits both depths, M:237): an EXACT
 * brute-force L2 2-nearest-neighbour search in place of the FLANN KD-tree index of M:241-250 (approximate and randomised: not reproduced).
 * Every parameter means what it means for isx_match_features, except:
 *   descriptors  num_images CV_32FC1 mats of n_i x cols, 1 <= cols <= 128 (cols > 128 -> ISX_ERR_UNSUPPORTED), the same cols for every image
 *                with rows (else ISX_ERR_SIZE), host or device, 4-byte aligned in pointer and step (else ISX_ERR_INVALID); another type ->
 *                ISX_ERR_TYPE.  Rows may be 0; the row limits are isx_match_features'.
 *   the search   s(q, t) in float32: s = 0, then for c = 0 .. cols - 1 in that order e = a[c] - b[c], s = s + e * e, every operation
 *                rounded on its own (no FMA).  An s that is not finite - overflow, or NaN from non-finite input - becomes +inf: nothing is
 *                refused.  The two nearest rows are the two smallest by (s, row); the distance is d = sqrtf(s), correctly rounded; the
 *                ratio test is d0 < k * d1.  Two distinct s can round to one d: knn is ordered by s.
 *   matches      column 2 carries the IEEE-754 bits of the float32 distance d0 (DMatch::distance is a float).
 *   knn          row0, bits(d0), row1, bits(d1); -1, -1 where there is no such neighbour.
 * Same statuses, same capture rule, at most three launches a call, no read-back with device mats throughout, the same per-thread scratch
 * (isx_match_release).  An accepted match has s0 < s1, so the list is that of any exact L2 matcher computing the same distances; parity
 * with OpenCV is unpinned twice over (the KD-tree is approximate, and its SIMD normL2Sqr sums in another order).                        */
int isx_match_features_f32(int num_images, const isx_mat* descriptors, const isx_mat* keypoints, const int* image_sizes_wh,
                           int num_pairs, const int* pairs_ij, float match_conf, isx_mat* matches, isx_mat* points, isx_mat* counts,
                           isx_mat* knn, int* info, int device, void* hip_stream);
/* Returns the scratch of the calling thread (the matcher going out of scope).  PER THREAD and not freed at thread exit, as for
 * isx_voronoi_seam_release.                                                                                                            */
int isx_match_release(void);

/* ---- findHomography, inliers and confidence (R = the reference's 计算单应性矩阵/计算单应性矩阵/计算单应性矩阵.cpp) ------------------------- */
/* Hypotheses per chunk of the RANSAC kernel (homography.hip takes it from here): one per lane of the pair's wave. */
enum { ISX_HOMOGRAPHY_CHUNK = 64 };
/* status bits of stats column 0 */
enum { ISX_HOMOGRAPHY_H = 1,            /* H is not empty                                                                  */
       ISX_HOMOGRAPHY_PASS2 = 2,        /* the second run on the inliers ran (R:881-909)                                    */
       ISX_HOMOGRAPHY_PASS2_FAILED = 4, /* ... and failed: H is empty (R:909 assigns its result), bit 0 is clear            */
       ISX_HOMOGRAPHY_CLAMPED = 8,      /* the count exceeded the rows of its points or mask mat and was clamped to them    */
       ISX_HOMOGRAPHY_DEGENERATE = 16   /* |det H| < DBL_EPSILON: R:863 returned, H is pass 1's, num_inliers and conf are 0 */ };
/* The second half of BestOf2NearestMatcher1::match, R:836-909, for every pair of a matcher call, WITHOUT the Levenberg-Marquardt polish of
 * R:672 (createLMSolver1(...)->run(H8), R:461-591: opt-in, isx_find_homography_lm below; it changes neither mask, count nor confidence - H here is the least-squares
 * runKernel over the inliers that LM starts from).  Per pair, with n = counts[p]:
 *   n < num_matches_thresh1 (R:836)   H, stats and conf are zeros, the mask is not written.
 *   pass 1 (R:862)                    findHomography2(src, dst, RANSAC, reproj_thresh, mask, max_iters, confidence) (R:602-693): n < 4 fails
 *                                     (R:159; H empty, the mask zeros, R:687); n == 4 is runKernel itself with the mask all ones (R:641-645);
 *                                     else RANSACPointSetRegistrator1::run (R:139-233) with RNG rng((uint64)-1), getSubset's 10000 attempts
 *                                     (R:88-137), checkSubset (R:253-288), runKernel (R:304-373; R itself lost the call between R:196 and
 *                                     R:197, it is in place here), computeError / findInliers in float32 (R:383-402, R:67-86),
 *                                     RANSACUpdateNumIters1 (R:39-59), then runKernel over all inliers (R:657-668).
 *   R:863                             an empty H or |det H| < DBL_EPSILON stops here: num_inliers = 0, conf = 0, the mask stays as written.
 *   R:866-878                         num_inliers = the mask's sum; conf = num_inliers / (8 + 0.3 n) in double, a value > 3 becomes 0.
 *   pass 2 (R:881-909)                with num_inliers >= num_matches_thresh2: findHomography2 again over the inliers only (no mask out, a
 *                                     fresh RNG); H is its result, empty if it fails.
 * cv::eigen (JacobiImpl_), cv::RNG, haveCollinearPoints and cvRound are in neither tree and are restated (DESIGN.md §8 "Homography",
 * tests/helpers/homography_np.py - the specification): parity with OpenCV is not pinned.
 *   points        per pair the matcher's CV_32FC1 mat, rows x >= 4: src.x, src.y, dst.x, dst.y; host or device, 4-byte aligned.
 *   counts        the matcher's CV_32SC1 mat of at least 1 x num_pairs.  A device mat is read ON THE DEVICE, never read back to size anything:
 *                 capacities are the mats' rows.  A count above the rows of its points or mask mat is clamped to them (status bit 3), a
 *                 negative one is 0.
 *   reproj_thresh <= 0 means 3 (R:636); max_iters >= 1; confidence in (0, 1) (R:156); the thresholds >= 0 (6 and 6 at R:781).
 *   H             a CV_64FC1 mat of at least 3 num_pairs x 3, pair p in rows 3p .. 3p + 2; an empty H is nine zeros with status bit 0 clear.
 *   inlier_masks  per pair a CV_8UC1 mat of at least count x 1 (any pointer and step): rows [0, count) get 0 or 1 (R:82), later rows are not
 *                 written.
 *   stats         a CV_32SC1 mat of at least num_pairs x 8: status bits, num_inliers, the iterations run and the winning iteration (-1: none)
 *                 of pass 1, the same of pass 2, getSubset's attempts in total, 0.
 *   conf          a CV_64FC1 mat of at least 1 x num_pairs.
 *   info          NULL, or 2 ints: the pairs processed and the kernel launches of this call - ONE, however many pairs.
 * Output mats are host or device mats, 4-byte aligned in pointer and step, 8-byte for H and conf.  Checked before anything is written or
 * enqueued: null pointers, num_pairs < 0, the scalar ranges above, a misaligned mat -> ISX_ERR_INVALID; a mat of another type ->
 * ISX_ERR_TYPE; too few rows or columns -> ISX_ERR_SIZE.  The call uploads its table (and stages host mats): on a capturing stream ->
 * ISX_ERR_STATE with nothing enqueued.  With device mats throughout nothing is read back or synchronised.  Host mats synchronise.
 * The bits of H and conf are those of the specification except where pow / log of R:51-56 land within an ulp of a rounding boundary of the
 * iteration count.                                                                                                       */
int isx_find_homography(int num_pairs, const isx_mat* points, const isx_mat* counts, double reproj_thresh, int max_iters, double confidence,
                        int num_matches_thresh1, int num_matches_thresh2, isx_mat* H, isx_mat* inlier_masks, isx_mat* stats, isx_mat* conf,
                        int* info, int device, void* hip_stream);
/* isx_find_homography WITH the Levenberg-Marquardt polish of R:672: after the runKernel over the inliers of each pass (R:657-668, n > 4, at
 * least one inlier; also where that runKernel returned 0 and left the RANSAC model; never for n == 4) createLMSolver1(makePtr<
 * HomographyRefineCallback>(src, dst), lm_max_iters)->run(H8) (R:404-591) replaces the first eight doubles of H - H[8] keeps runKernel's
 * bits (R:669) - so H is the reprojection-error minimiser MatchesInfo::H holds in the reference, and the degenerate test of R:863 sees it.
 * Mask, num_inliers and confidence are isx_find_homography's.  OPT-IN AND UNPINNED: the OpenCV calls inside LMSolverImpl1::run
 * (mulTransposed, gemm, norm, dot, solve / invert with DECOMP_EIG) are in neither tree and are restated from OpenCV 3.4.2's published source
 * in tests/helpers/homography_lm_np.py - the specification, to which H agrees bit for bit (DESIGN.md §8 "Homography").
 * Arguments, checks, capture rule, scratch (isx_homography_release) and the ONE launch are isx_find_homography's, except:
 *   lm_max_iters  maxIters of the solver, 10 at R:672; in [1, 1000], else ISX_ERR_INVALID.
 *   stats         at least num_pairs x 12: columns 0 - 7 as above; 8, 9: run()'s return value (the iterations, negated when they reached
 *                 lm_max_iters, R:577-580) and nfJ of pass 1; 10, 11: those of pass 2; 0 where LM did not run.                            */
int isx_find_homography_lm(int num_pairs, const isx_mat* points, const isx_mat* counts, double reproj_thresh, int max_iters, double confidence,
                           int num_matches_thresh1, int num_matches_thresh2, int lm_max_iters, isx_mat* H, isx_mat* inlier_masks, isx_mat* stats,
                           isx_mat* conf, int* info, int device, void* hip_stream);
/* Returns the scratch of the calling thread.  PER THREAD and not freed at thread exit, as for isx_match_release.                          */
int isx_homography_release(void);

/* ---- HomographyBasedEstimator (C = the reference's 恢复相机内参数/恢复相机内参数/恢复相机内参数.cpp) ---------------------------------------- */
/* Images a rig at the most (estimator.hip takes it from here): one per lane of the wave that runs Kruskal and the leaf walks. */
enum { ISX_ESTIMATOR_MAX_IMAGES = 64 };
/* status bits of rig_stats column 0 */
enum { ISX_ESTIMATOR_MEDIAN = 1,    /* the focal is the median of the candidates (C:84-95), not the fallback of C:97-104            */
       ISX_ESTIMATOR_ASSERT = 2,    /* the tree has 0 or more than 2 centers, where C:212 asserts: no walk, every R the identity     */
       ISX_ESTIMATOR_UNREACHED = 4  /* the walk of C:275 did not reach every camera of the rig; those keep the identity              */ };
/* HomographyBasedEstimator1 estimator(is_focals_estimated); estimator(features, pairwise_matches, cameras) (C:313-321) for every rig - an
 * independent image set - of a matcher call, on the mats isx_find_homography / isx_find_homography_lm left.  pairwise_matches[i * n + j]
 * for i < j is pair (i, j)'s H where its status bit ISX_HOMOGRAPHY_H is set, with num_inliers of stats column 1; for i > j it is the dual
 * the reference's matcher stores, H.inv() with the same num_inliers; every other entry has an empty H.  Per rig of n images:
 *   C:253-261    focals not given: estimateFocal1 (C:55-105) - focalsFromHomography1 (C:26-54) over every ordered pair with H, the
 *                candidates sqrt(f0 * f1) where both are ok, their median when there are at least n - 1 (the mean of the middle two times
 *                0.5 for an even count, C:92), else sum(width + height) / n (C:99-103); cameras = CameraParams() with that focal.
 *   C:264-268    focals given: focal, aspect, ppx, ppy per image from focals_in; ppx -= 0.5 * width, ppy -= 0.5 * height.
 *   C:145-213    findMaxSpanningTree: the edges of every ordered pair with H, weight (float)num_inliers, sorted descending (C:169), Kruskal,
 *                the leafs, a breadth-first distance from every leaf (C:193-199), max_dists, the min-max distance, the centers in index
 *                order.  C:212 asserts 1 or 2 centers; with another number (a disconnected graph only) status bit ISX_ESTIMATOR_ASSERT is
 *                set and every R of the rig is the identity - the focals and K are still written.
 *   C:215-243    CalcRotation over the breadth-first walk from centers[0] (C:275): R_to = R_from * ((K_from.inv() * H.inv()) * K_to), H the
 *                entry of the ordered pair (from, to) - for from > to the dual, inverted again as the reference does.  Cameras outside the
 *                root's component keep the identity (ISX_ESTIMATOR_UNREACHED).
 *   C:278-282    ppx += 0.5 * width, ppy += 0.5 * height.
 *   C:329-334, C:385-386   K() and R converted to float32 (round to nearest): what isx_warper_* takes.
 * THE TIE RULE: std::sort leaves the order of edges of equal weight open, and (i, j) and (j, i) always tie.  Here it is fixed: weight
 * descending, then i * n + j ascending.  The weight is compared as the integer num_inliers, which (float) holds exactly up to 2^24; the
 * matcher's row limit (ISX_MATCH_MAX_ROWS) keeps it below 2^21.
 * RESTATED AND UNPINNED: Mat::inv() of a 3 x 3 CV_64F (cofactors times the reciprocal determinant as in OpenCV 3.4.2; nine zeros for a
 * determinant of exactly 0), Mat * Mat (three-term sums, left to right), CameraParams() (aspect 1, ppx = ppy = 0, R = eye, t = 0),
 * CameraParams::K() and Graph::walkBreadthFirst (adjacency in insertion order) are in neither tree: tests/helpers/estimator_np.py is the
 * specification (DESIGN.md §8 "Camera estimator"), to which every output agrees bit for bit.  float64 + - * / sqrt only, no contraction.
 *   image_sizes_wh  (width, height) per image (features[i].img_size).
 *   pairs_from_to   num_pairs (from, to), from < to, both of one rig, no pair twice: row p of stats and conf and rows 3p .. 3p + 2 of H.
 *   rig_first       num_rigs + 1 increasing image offsets from 0 to num_images; NULL = one rig (num_rigs must be 1).  A rig has from 2
 *                   (C:84 indexes all_focals[-1] with one image) to ISX_ESTIMATOR_MAX_IMAGES images.
 *   H, stats, conf  isx_find_homography's: CV_64FC1 of at least 3 num_pairs x 3, CV_32SC1 of at least num_pairs x 2, CV_64FC1 of at least
 *                   1 x num_pairs; a device mat is read ON THE DEVICE.  conf is checked and not read (the estimator weighs by num_inliers).
 *   focals_in       NULL = estimate the focals; else CV_64FC1 of at least num_images x 4: focal, aspect, ppx, ppy (is_focals_estimated).
 *   cameras         CV_64FC1, at least num_images x 16: focal, aspect, ppx, ppy, R[9], t[3] (zeros).
 *   kr32            CV_32FC1, at least num_images x 18: K()[9], then R[9].
 *   tree            CV_32SC1, at least num_images x 2: the parent in the walk as an index inside the rig (-1 the root, -2 not reached) and
 *                   the depth (-1 not reached).
 *   rig_stats       CV_32SC1, at least num_rigs x 8: status bits, focal candidates, the two centers as indices inside the rig (-1 where
 *                   absent), tree edges, cameras reached, the number of centers, the min-max distance.
 *   info            NULL, or 2 ints: the rigs processed and the kernel launches of this call - ONE, a workgroup per rig.
 * Mats are host or device mats, 4-byte aligned in pointer and step, 8-byte for the CV_64FC1 ones.  Checked before anything is written or
 * enqueued: null pointers, fewer than 2 images in a rig, a pair with from >= to, a repeated pair, a pair across two rigs, an index out of
 * range, rig_first not increasing, a misaligned mat -> ISX_ERR_INVALID; a mat of another type -> ISX_ERR_TYPE; too few rows or columns ->
 * ISX_ERR_SIZE; more than ISX_ESTIMATOR_MAX_IMAGES images in a rig -> ISX_ERR_UNSUPPORTED.  The call uploads its table (and stages host
 * mats): on a capturing stream -> ISX_ERR_STATE with nothing enqueued.  With device mats throughout nothing is read back or synchronised.
 * Host mats synchronise.  BundleAdjusterRay, BundleAdjusterReproj and waveCorrect (commented out at C:355-361) are isx_bundle_adjust_ray,
 * isx_bundle_adjust_reproj and isx_wave_correct below.  Not built: leaveBiggestComponent.                                              */
int isx_estimate_cameras(int num_images, const int* image_sizes_wh, int num_pairs, const int* pairs_from_to, int num_rigs, const int* rig_first,
                         const isx_mat* H, const isx_mat* stats, const isx_mat* conf, const isx_mat* focals_in, isx_mat* cameras, isx_mat* kr32,
                         isx_mat* tree, isx_mat* rig_stats, int* info, int device, void* hip_stream);
/* Returns the scratch of the calling thread (its own: isx_homography_release does not free it).  PER THREAD and not freed at thread exit,
 * as for isx_homography_release.                                                                                                       */
int isx_estimator_release(void);

/* ---- BundleAdjusterRay (W = the reference's cylindrical-projection demo, W:183-194; the same lines stand in its other demos) ------------ */
/* Images a rig at the most, and the matches of a tile of the accumulation (bundle.hip takes them from here; tests/helpers/bundle_np.py
 * repeats them): an edge's inlier matches are summed in tiles of ISX_BUNDLE_TILE in match order, the tiles in order, the edges in order. */
enum { ISX_BUNDLE_MAX_IMAGES = ISX_ESTIMATOR_MAX_IMAGES, ISX_BUNDLE_TILE = 64 };
/* status bits of rig_stats_out column 0 */
enum { ISX_BUNDLE_NAN = 1,          /* a parameter ended as NaN: estimate() returns false, the rig's cameras_out are cameras_in           */
       ISX_BUNDLE_NO_EDGES = 2,     /* no pair of the rig has confidence > conf_thresh: the cameras pass through                          */
       ISX_BUNDLE_EST_ASSERT = 4,   /* est_rig_stats carries ISX_ESTIMATOR_ASSERT (or no center inside the rig): the cameras pass through */
       ISX_BUNDLE_SINGULAR_R = 8,   /* a camera's R has no polar factor (R^T R not finite or not positive): it started from the identity  */
       ISX_BUNDLE_DROPPED = 16      /* a pivot of the Cholesky solve fell under the trace rule at least once: that step component was 0   */ };
/* cameras[i].R.convertTo(R, CV_32F) (W:183-188); adjuster = new detail::BundleAdjusterRay(); adjuster->setConfThresh(1);
 * (*adjuster)(features, pairwise_matches, cameras) (W:189-194) for every rig of a matcher call, in ONE launch, on the mats the matcher, the
 * homography stage and the estimator left.  OpenCV 3.4.2's BundleAdjusterBase::estimate and BundleAdjusterRay restated - 4 parameters a
 * camera (focal and a Rodrigues vector), 3 residuals an inlier match.  Per rig:
 *   setUpInitialCameraParams   R as float32 (the kernel rounds cameras_in's float64 R: kr32's bits), its polar factor (svd(R); u * vt; the
 *                              sign of the determinant), Rodrigues, the vector rounded to float32.
 *   the edges                  pairs i < j in index order with conf > conf_thresh; their matches k < counts[p] with inlier_masks[p][k] != 0.
 *   calcError                  H = Rodrigues(rvec) * K.inv(), K = [[f, 0, width / 2], [0, f, height / 2], [0, 0, 1]]; the rays of both
 *                              keypoints divided by their length; sqrt(f1 f2) times their difference.
 *   calcJacobian               central differences, step 1e-3, parameter by parameter.
 *   CvLevMarq                  TermCriteria(EPS + COUNT, max_iter, eps), lambdaLg10 from -3, at most 33 retries an iteration.
 *   after the loop             a NaN parameter: the rig's cameras pass through (ISX_BUNDLE_NAN).  Else focal = param, R = Rodrigues(rvec) as
 *                              float32, then R_i = R_center.inv() * R_i in float64 from those float32 values, rounded once; center =
 *                              span_tree_centers[0] = column 2 of est_rig_stats, the estimator's own findMaxSpanningTree.
 * RESTATED AND UNPINNED: OpenCV's source is in neither tree; tests/helpers/bundle_np.py is the specification (DESIGN.md §8 "Bundle
 * adjuster"), to which every output agrees bit for bit.  THIS PROJECT'S DECISIONS, not OpenCV's: cvSolve(CV_SVD) is a Cholesky factorisation
 * with SVBkSb's truncation rule on the pivots (not > trace * 2 DBL_EPSILON: that parameter's step is 0); sin, cos and acos are restated in
 * + - * / sqrt (csrc/bundle_math.hpp, absolute error below 1e-12); sums run per tile of ISX_BUNDLE_TILE matches, then tiles and edges in
 * order; lambda = 10^lambdaLg10 is a table of correctly rounded literals; the float32 SVD and the SVD inside cvRodrigues2 are one float64
 * polar factor; a match whose queryIdx / trainIdx lies outside its image's keypoints is no inlier; the loop also ends on a NaN parameter.
 *   image_sizes_wh  (width, height) per image.
 *   keypoints       num_images CV_32FC1 mats of n_i x 2 (pt.x, pt.y), the matcher's input.
 *   pairs_from_to   num_pairs (from, to), from < to, both of one rig, no pair twice, any order: row p of counts, stats, conf, matches[p]
 *                   and inlier_masks[p].
 *   matches         per pair the matcher's CV_32SC1 mat, rows x >= 3: queryIdx, trainIdx, distance.
 *   inlier_masks    per pair the homography stage's CV_8UC1 mat, rows x >= 1.
 *   counts          the matcher's CV_32SC1 mat of at least 1 x num_pairs.  A count above the rows of its matches or mask mat is clamped to
 *                   them, a negative one is 0.
 *   stats, conf     the homography stage's: CV_32SC1 of at least num_pairs x 2 (checked, not read), CV_64FC1 of at least 1 x num_pairs.
 *   rig_first       as for isx_estimate_cameras; a rig has from 2 to ISX_BUNDLE_MAX_IMAGES images.
 *   est_rig_stats   the estimator's rig_stats: CV_32SC1, at least num_rigs x 8.
 *   cameras_in      the estimator's cameras: CV_64FC1, at least num_images x 16.
 *   conf_thresh     >= 0 (1 at W:189-194): an edge then has confidence > 0, and with it a mask the homography stage wrote.
 *   max_iter, eps   1000 and DBL_EPSILON in OpenCV; max_iter in [1, 1000].
 *   cameras_out     CV_64FC1, at least num_images x 16: cameras_in with focal and R replaced (R holds float32 values).
 *   kr32_out        CV_32FC1, at least num_images x 18: K()[9], then R[9] - what isx_warper_* takes.
 *   rig_stats_out   CV_32SC1, at least num_rigs x 8: status bits, iterations, Jacobian evaluations, error evaluations, the last
 *                   lambdaLg10, edges, inlier matches, 0.  A rig that passes through before the loop has zeros in columns 1 - 4.
 *   rig_err_out     CV_64FC1, at least num_rigs x 2: the first and the last |err|.
 *   info            NULL, or 2 ints: the rigs processed and the kernel launches of this call - ONE, a workgroup per rig.
 * Mats are host or device mats, 4-byte aligned in pointer and step (masks: any), 8-byte for the CV_64FC1 ones.  A device mat is read ON THE
 * DEVICE: counts, conf and est_rig_stats are never read back, every scratch size comes from the mats' rows.  Checked before anything is
 * written or enqueued: null pointers, fewer than 2 images in a rig, a pair with from >= to, a repeated pair, a pair across two rigs, an index
 * out of range, rig_first not increasing, max_iter outside [1, 1000], conf_thresh negative or not a number, eps not a number, a misaligned
 * mat -> ISX_ERR_INVALID; a mat of another type -> ISX_ERR_TYPE; too few rows or columns -> ISX_ERR_SIZE; more than ISX_BUNDLE_MAX_IMAGES
 * images in a rig -> ISX_ERR_UNSUPPORTED.  The call uploads its tables (and stages host mats): on a capturing stream -> ISX_ERR_STATE with
 * nothing enqueued.  With device mats throughout nothing is read back or synchronised.  Host mats synchronise.  BundleAdjusterReproj
 * (commented out at W:190) and waveCorrect (W:198) follow below.  Not built: leaveBiggestComponent.                                     */
int isx_bundle_adjust_ray(int num_images, const int* image_sizes_wh, const isx_mat* keypoints, int num_pairs, const int* pairs_from_to,
                          const isx_mat* matches, const isx_mat* inlier_masks, const isx_mat* counts, const isx_mat* stats, const isx_mat* conf,
                          int num_rigs, const int* rig_first, const isx_mat* est_rig_stats, const isx_mat* cameras_in, double conf_thresh, int max_iter,
                          double eps, isx_mat* cameras_out, isx_mat* kr32_out, isx_mat* rig_stats_out /* CV_32SC1 rigs x 8 */,
                          isx_mat* rig_err_out /* CV_64FC1 rigs x 2 */, int* info, int device, void* hip_stream);
/* Returns the scratch of the calling thread (its own: isx_estimator_release does not free it).  PER THREAD and not freed at thread exit,
 * as for isx_estimator_release.                                                                                                        */
int isx_bundle_release(void);

/* ---- BundleAdjusterReproj (commented out at W:190, C:340; the default of cv::Stitcher and of stitching_detailed --ba reproj) ------------- */
/* isx_bundle_adjust_ray with OpenCV 3.4.2's BundleAdjusterReproj restated in place of BundleAdjusterRay: 7 parameters a camera (focal, ppx,
 * ppy, aspect and a Rodrigues vector), 2 residuals an inlier match.  The same kernel compiled a second time (512 threads a workgroup: a
 * thread per row of the 7 n <= 448 unknowns), the same edges and inliers, CvLevMarq, lambda table, Cholesky solve with the trace rule,
 * tiles of ISX_BUNDLE_TILE matches, status bits, validation, error codes, host-or-device mats, capture rule, ONE launch and per-thread
 * scratch (isx_bundle_release frees it).  tests/helpers/bundle_reproj_np.py is the specification (UNPINNED, DESIGN.md §8 "Reprojection
 * adjuster"), to which every output agrees bit for bit.  What differs:
 *   the parameters   focal, ppx, ppy, aspect from cameras_in columns 0, 2, 3, 1; rvec as for Ray (float32 R, polar factor, Rodrigues, float32).
 *   calcError        per edge (i, j): H = ((K_j * R_j.inv()) * R_i) * K_i.inv(), K = [[f, 0, ppx], [0, f * aspect, ppy], [0, 0, 1]]; per
 *                    inlier match (x, y, z) = H (p_i.x, p_i.y, 1); the residuals p_j.x - x / z and p_j.y - y / z.  A z of 0 gives what
 *                    IEEE division gives.  image_sizes_wh is checked and not read.
 *   calcJacobian     central differences, step 1e-4.
 *   refine_flags     OpenCV's refinement mask as bits: 1 (0,0) focal, 2 (0,1) unused, 4 (0,2) ppx, 8 (1,1) aspect, 16 (1,2) ppy; 31 in
 *                    OpenCV; outside [0, 31] -> ISX_ERR_INVALID.  The rotation is always refined.  The Jacobian column of a parameter whose
 *                    bit is clear stays zero: its pivot then falls under the trace rule, its step is 0 - the parameter keeps its input
 *                    value - and ISX_BUNDLE_DROPPED is set, as for any other dropped pivot.
 *   after the loop   focal, ppx, ppy, aspect of cameras_out and K of kr32_out are the refined parameters; R as for Ray.                  */
int isx_bundle_adjust_reproj(int num_images, const int* image_sizes_wh, const isx_mat* keypoints, int num_pairs, const int* pairs_from_to,
                             const isx_mat* matches, const isx_mat* inlier_masks, const isx_mat* counts, const isx_mat* stats, const isx_mat* conf,
                             int num_rigs, const int* rig_first, const isx_mat* est_rig_stats, const isx_mat* cameras_in, double conf_thresh,
                             int max_iter, double eps, int refine_flags, isx_mat* cameras_out, isx_mat* kr32_out,
                             isx_mat* rig_stats_out /* CV_32SC1 rigs x 8 */, isx_mat* rig_err_out /* CV_64FC1 rigs x 2 */, int* info, int device,
                             void* hip_stream);

/* ---- waveCorrect (commented out at C:355-361, W:198; the default of cv::Stitcher and of stitching_detailed --wave_correct horiz) --------- */
enum { ISX_WAVE_CORRECT_HORIZ = 0, ISX_WAVE_CORRECT_VERT = 1 };
/* status bits of rig_stats_out column 0: the rig's cameras pass through */
enum { ISX_WAVE_DEGENERATE = 1,     /* norm(rg0) <= DBL_MIN, where waveCorrect returns                                                   */
       ISX_WAVE_SINGLE = 2          /* a rig of one image, where waveCorrect returns (rmats.size() <= 1)                                 */ };
/* waveCorrect(rmats, kind) of OpenCV 3.4.2 restated (UNPINNED; tests/helpers/bundle_reproj_np.py wave_correct is the specification, to which
 * every output agrees bit for bit) for every rig in ONE launch, a workgroup a rig, so that the cameras reach the warper in stream order.
 * All arithmetic is float32 on R rounded to float32: moment = sum of col0 col0^T in image order; eigen(moment) by the restated Jacobi
 * (eigenvalues descending, eigenvectors as rows, threshold FLT_EPSILON); rg1 = row 2 (HORIZ) or row 0 (VERT); img_k = sum of col2;
 * rg0 = rg1 x img_k, divided by its norm; rg2 = rg0 x rg1; conf = sum of rg0 . col0 (HORIZ) or minus the sum of rg1 . col0 (VERT), and
 * conf < 0 negates rg0 and rg1; R_i = [rg0; rg1; rg2] * R_i.
 *   rig_first       num_rigs + 1 increasing image offsets from 0 to num_images; NULL = one rig.  A rig has at least 1 image.
 *   cameras_in      CV_64FC1, at least num_images x 16: focal, aspect, ppx, ppy, R[9], t[3] - an adjuster's or the estimator's cameras.
 *   kind            ISX_WAVE_CORRECT_HORIZ or ISX_WAVE_CORRECT_VERT, else ISX_ERR_INVALID.
 *   cameras_out     CV_64FC1, at least num_images x 16: cameras_in with R replaced (float32 values); a rig that passes through is copied.
 *                   It may be cameras_in itself.
 *   kr32_out        CV_32FC1, at least num_images x 18: K()[9], then R[9].
 *   rig_stats_out   CV_32SC1, at least num_rigs x 2: status bits, images.
 *   info            NULL, or 2 ints: the rigs processed and the kernel launches of this call - ONE.
 * Mats are host or device mats, aligned as for isx_bundle_adjust_ray; the checks (null pointers, rig_first, kind -> ISX_ERR_INVALID; type ->
 * ISX_ERR_TYPE; rows or columns -> ISX_ERR_SIZE), the capture rule (ISX_ERR_STATE) and the scratch (isx_bundle_release) are its too.      */
int isx_wave_correct(int num_images, int num_rigs, const int* rig_first, const isx_mat* cameras_in, int kind, isx_mat* cameras_out,
                     isx_mat* kr32_out, isx_mat* rig_stats_out /* CV_32SC1 rigs x 2 */, int* info, int device, void* hip_stream);

/* ---- on-disk format either side of the path: .bmp (W:166 imread, W:155-156,315 imwrite) ----------- */
/* Reading: uncompressed Windows bitmaps only (the reference's inputs and committed artefacts are BMPs).
 * isx_bmp_read = cv::imread(path) with IMREAD_COLOR: `out` is a CV_8UC3 mat (host or device) of the size
 * isx_bmp_size reports; 8-bit paletted files are expanded through their palette.  isx_bmp_write = cv::imwrite
 * for CV_8UC3 (24-bit) and CV_8UC1 (8-bit, grey palette), host or device mats.                              */
int isx_bmp_size(const char* path, int* rows, int* cols);
int isx_bmp_read(const char* path, isx_mat* out);
int isx_bmp_write(const char* path, const isx_mat* img);
/* cv::imwrite("pano.jpg", result) (B:1132, S:1282): baseline sequential JFIF, 8-bit, the Annex K Huffman tables, 4:2:0
 * chroma for CV_8UC3 (BGR), one component for CV_8UC1; quality 1..100 scales the Annex K quantisation tables as libjpeg does
 * (OpenCV's default is 95).  Any JPEG decoder reads the file; it is not libjpeg's byte stream.  Host or device mats.   */
int isx_jpeg_write(const char* path, const isx_mat* img, int quality);
/* cv::imread(path) (IMREAD_COLOR) for .jpg: baseline / extended-sequential / progressive Huffman JPEG, 8-bit, grey or YCbCr (any integer
 * sampling; 4:4:4, 4:2:2 and 4:2:0 with libjpeg's "fancy" upsampling), restart intervals, interleaved or one scan per component.  The
 * arithmetic is libjpeg's (accurate integer IDCT, its upsampling and colour conversion): what cv::imread hands back.  Arithmetic-coded,
 * lossless, 12-bit and CMYK files, and progressive files whose scans stop short of full precision (libjpeg would smooth those):
 * ISX_ERR_UNSUPPORTED.  `out` is a CV_8UC3 mat (host or device) of the size isx_jpeg_size reports.                                     */
int isx_jpeg_size(const char* path, int* rows, int* cols);
int isx_jpeg_read(const char* path, isx_mat* out);

/* ---- the reference's in-tree single-band seam-ramp blend (B:141-717) --------------------- */
/* images1/images2: CV_32FC3 warped tiles (B:143-145), tl1/tl2 their corners (B:148-149),
 * pano: caller-allocated CV_32FC3 of isx_blend_pair_linear_size().  seam_x (optional, may be
 * NULL) receives the greedy seam's x per row (B:268-307), panoHe_ entries.                    */
int isx_blend_pair_linear_size(int rows1, int cols1, int rows2, int cols2,
                               int tl1_x, int tl1_y, int tl2_x, int tl2_y,
                               int* pano_rows, int* pano_cols);
int isx_blend_pair_linear(const isx_mat* images1, const isx_mat* images2,
                          int tl1_x, int tl1_y, int tl2_x, int tl2_y,
                          isx_mat* pano, int* seam_x, int device, void* hip_stream);
/* isx_blend_pair_linear keeps its work buffers (cost map, chunk maps, seam, weight maps: 41 MB for a 4K pair) per calling thread
 * between calls; this returns them.  PER THREAD, and not freed at thread exit: call it on every worker thread that made the call
 * before that thread ends (see isx_dp_seam_release). */
int isx_blend_pair_linear_release(void);

/* ---- assembling a batch of mosaics across the GPUs of a node (no counterpart in the reference; BASELINE config 4) ---------------- */
/* One process per GPU.  The independent pairs of a batch are partitioned across the ranks (no collective while blending); each rank
 * writes its blended mosaics into ONE packed send block, and every rank ends up with all blocks: an all-gather over RCCL (xGMI).
 * The library loads librccl.so.1 at the first of these calls (dlopen; inside a torch process that is torch's own copy).
 *   isx_gather_unique_id : rank 0 creates the 128-byte rendezvous id and hands it to the other ranks by any means it has (a file,
 *                          a socket, MPI_Bcast, torch.distributed.broadcast_object_list).
 *   isx_gather_create    : collective over all ranks; `device` is this rank's GPU.  id == NULL: no RCCL communicator is created (no
 *                          collective call needed) and only the direct schedule below is available.
 *   isx_gather_all       : ONE all-gather of `bytes` bytes from `send` into recv[rank * bytes ...) on `hip_stream`.
 *   isx_gather_chunk     : the same block gathered chunk by chunk (a chunk = one pair's mosaic, [offset, offset + bytes) of the send
 *                          block): enqueued on the handle's own communication stream behind `ready_event` (a hipEvent_t the caller
 *                          recorded after enqueueing that pair's blend; NULL = now), so the transfer of pair p runs under the blends
 *                          of the pairs after it.  Chunks land rank-major PER CHUNK: isx_gather_chunk_ptr gives the address of
 *                          (rank, chunk) inside recv_base, which must hold world * block_bytes bytes.  Every rank must post the
 *                          same chunks in the same order.
 *   isx_gather_wait      : makes `hip_stream` wait (without blocking the host) for every chunk enqueued so far;
 *   isx_gather_synchronize blocks the host until they are done.                                                             */
typedef struct isx_gather isx_gather;
int isx_gather_unique_id(unsigned char id[128]);
int isx_gather_create(int world, int rank, const unsigned char id[128], int device, isx_gather** out);
/* isx_gather_destroy frees the p2p receive buffer (isx_gather_p2p_alloc) and unmaps the peers': no other rank may still be copying into
 * this rank's buffer - barrier across the ranks first, as after any one-sided put - and no view of the buffer may be used afterwards. */
int isx_gather_destroy(isx_gather* g);
int isx_gather_info(const isx_gather* g, int* world, int* rank);
int isx_gather_all(isx_gather* g, const void* send, size_t bytes, void* recv, void* hip_stream);
int isx_gather_chunk(isx_gather* g, const void* send_base, size_t block_bytes, size_t offset, size_t bytes, void* recv_base,
                     void* ready_event);
int isx_gather_chunk_ptr(const isx_gather* g, void* recv_base, size_t offset, size_t bytes, int rank, void** ptr);
int isx_gather_wait(isx_gather* g, void* hip_stream);
int isx_gather_synchronize(isx_gather* g);
/* The direct schedule beside the collective (xGMI is point to point: a rank's block crosses each of its world - 1 links once whatever
 * the schedule; here the rank issues the world - 1 device-to-device copies itself, one stream per destination, instead of leaving rings
 * and channels to RCCL - bench.py --gather-backend p2p against torch / isx tells the schedule from the links):
 *   isx_gather_p2p_alloc : this rank's receive buffer (world x block bytes, its own hipMalloc) and its 64-byte HIP IPC handle, which
 *                          travels to the other ranks by whatever the caller has (as the unique id does);
 *   isx_gather_p2p_open  : maps every rank's buffer (handles: world x 64 bytes, in rank order), creates the per-destination streams;
 *                          a failure part of the way is rolled back (mappings closed, streams destroyed): the call can be repeated;
 *   isx_gather_p2p_chunk : bytes [offset, offset + bytes) of the send block copied into every rank's buffer (this rank's own
 *                          included) behind `ready_event`, same layout as isx_gather_chunk (isx_gather_chunk_ptr applies);
 *   isx_gather_p2p_wait  : makes `hip_stream` wait for this rank's copies enqueued so far (its send block may then be rewritten);
 *                          arrival on the destination ranks is the callers' to establish, as after any one-sided put.                 */
int isx_gather_p2p_alloc(isx_gather* g, size_t bytes, void** ptr, unsigned char handle[64]);
int isx_gather_p2p_open(isx_gather* g, const unsigned char* handles);
int isx_gather_p2p_chunk(isx_gather* g, const void* send_base, size_t block_bytes, size_t offset, size_t bytes, void* ready_event);
int isx_gather_p2p_wait(isx_gather* g, void* hip_stream);
int isx_gather_p2p_synchronize(isx_gather* g);

/* ---- self-test --------------------------------------------------------------------------------- */
/* The fused warp kernel divides x / z and y / z with one shared reciprocal and the hardware division's own recurrence
 * written out in packed FMAs (csrc/warp.hip, k_warp_tile).  This compares that recurrence with the compiler's IEEE division
 * on n pseudo-random operand pairs of the range the kernel admits to it; *mismatches must come back 0.              */
int isx_selftest_division(int device, int n, unsigned long long seed, int* mismatches);
/* The dense solver of isx_blocks_gain_feed alone: x = solve(A, b, DECOMP_LU) for a caller's n x n row-major A and b in double, by hal::LU's
 * arithmetic on the device (where = 0; *swaps, may be NULL, gets the number of row exchanges) or by the host's scalar code that
 * isx_gain_compensator_feed solves with (where = 1; *swaps = -1).  n from 1 to 16384.  ISX_ERR_INTERNAL for a pivot below 100 DBL_EPSILON
 * (cv::solve returns false there); x is then untouched.  Uses the null stream and synchronises it.                          (W:238-244) */
int isx_selftest_lu_solve(int n, const double* A, const double* b, double* x, int* swaps, int where, int device);
/* detectResultRoi (W:64-88; SphericalWarper's border form) computed on the host alone - what isx_warper_roi returns for the cameras whose
 * extrema provably lie on the source's border (every spherical camera; a cylindrical one with the image in front of the camera and no pole
 * of the cylinder near it: every rig of the reference): the 2 (W + H) border pixels ranked on the caller's thread by two monotone stand-ins
 * (csrc/roihost.cpp, AVX2), the pixels within a tolerance of the four extrema evaluated with mapForward (W:36-45) and the host's libm.
 * Needs no device: the CPU test-suite compares it with the oracle's scan of every source pixel.  isa: 0 = the code isx_warper_roi runs
 * (AVX-512F where the CPU has it, else AVX2, else scalar), 1 = its scalar form, 2 = its AVX2 form.  ISX_ERR_UNSUPPORTED for a cylindrical camera outside that proof (isx_warper_roi scans every pixel on the GPU there). */
int isx_selftest_roi_host(int kind, float scale, const float K[9], const float R[9], int src_w, int src_h, int isa, int roi[4], float minmax[4]);
/* isx_warper_warp_point (RotationWarper::warpPoint, B:91-95, W:217-222) without a handle, which needs a device: mapForward of (x, y) under
 * (K, R) and, for ISX_WARP_PLANE, the translation T (NULL = zeros; a non-zero T is ISX_ERR_UNSUPPORTED for the other kinds).  Host code,
 * the same functions the handle's entry calls: the CPU test-suite compares it with the plane model and the oracle's mapForward.        */
int isx_selftest_warp_point(int kind, float scale, const float K[9], const float R[9], const float T[3], float x, float y, float out_uv[2]);
/* The host compilation of csrc/bundle_math.hpp, the arithmetic isx_bundle_adjust_ray runs per camera on the device, for n items: fn 0 sin,
 * 1 cos, 2 acos (1 double in, 1 out); 3 Rodrigues vector -> matrix (3 in, 9 out); 4 matrix -> vector (9 in, 3 out); 5 the polar factor (9 in,
 * 9 and a 1.0 / 0.0 "ok" out); 6 R K^-1 (f, rvec[3], width, height in, 9 out); 7 the ray (H[9], x, y in, 3 out); 8 the float32 Jacobi of the
 * wave correction (A[9] as doubles that hold float32 values in; V[9], the eigenvectors as rows, then W[3] descending out); 9 the float64
 * Jacobi (the same); 10 BundleAdjusterReproj's edge matrix (the seven parameters of camera 1, then of camera 2 in, 9 out); 11 its two
 * residuals (H[9], x1, y1, x2, y2 in, 2 out).  Needs no device: the CPU test-suite compares it with tests/helpers/bundle_np.py and
 * bundle_reproj_np.py bit for bit.  Its device twin is isx_selftest_bundle_math_device.                                               */
int isx_selftest_bundle_math(int fn, int n, const double* in, double* out);
/* The device compilation of the same header on the same items: `in` (host memory) is copied to the current device, one kernel runs a
 * thread per item that calls the same function, `out` (host memory) is copied back.  Uses the null stream and synchronises it.
 * tests/test_gpu_bundle_math.py holds the two entries and the model to the same bits.                                                 */
int isx_selftest_bundle_math_device(int fn, int n, const double* in, double* out);
/* The host compilation of csrc/proj_math.hpp, the float32 transcendentals of the fisheye and stereographic projectors, on n items: fn 0 sinf,
 * 1 cosf, 2 atan2f(in, in2), 3 atanf, 4 acosf; in2 is read by atan2f only (NULL otherwise).  Needs no device: the CPU test-suite compares it
 * with tests/helpers/polar_np.py bit for bit.                                                                                          */
int isx_selftest_proj_math(int fn, int n, const float* in, const float* in2, float* out);
/* The device compilation of the same header on the same items (host pointers; one thread per item).  Uses the null stream and synchronises it. */
int isx_selftest_proj_math_device(int fn, int n, const float* in, const float* in2, float* out);
/* The host compilation of csrc/sift_math.hpp, the two float32 exponentials of the SIFT finder, on n items: fn 0 expf, 1 exp2f.  Needs no
 * device: the CPU test-suite compares it with tests/helpers/sift_np.py bit for bit.                                                    */
int isx_selftest_sift_math(int fn, int n, const float* in, float* out);
/* The device compilation of the same header on the same items (host pointers; one thread per item).  Uses the null stream and synchronises it. */
int isx_selftest_sift_math_device(int fn, int n, const float* in, float* out);
/* Every entry of this header is a function-try-block: a C++ exception raised underneath it (std::bad_alloc of a host container, a
 * std::length_error, anything a future change throws) is stopped there and comes back as a status - ISX_ERR_NOMEM for the two allocation
 * failures, ISX_ERR_INTERNAL otherwise, the text in isx_last_error() - never as an exception in the caller's frames (the
 * reference's own errors are cv::Exceptions, W:94-96).  This entry throws `kind` from inside such a block so that the barrier can be
 * tested without a GPU: 0 std::bad_alloc, 1 std::length_error (vector::reserve), 2 a failing 2^62-byte allocation, 3 std::runtime_error,
 * 4 a thrown int, 5 std::out_of_range; any other kind returns ISX_OK.                                                            */
int isx_selftest_exception_barrier(int kind);

/* ---- per-kernel HIP-event timing (feeds bench.py's roofline object) ----------------------- */
/* When enabled every kernel launch is bracketed by hipEvents on its own stream.               */
int isx_profile_enable(int on);
int isx_profile_reset(void);
/* restrict the bracketing to one kernel name (NULL / "" = all): lets bench.py time the dominant
 * kernel inside the timed region without perturbing the other launches.                          */
int isx_profile_filter(const char* kernel_name);
/* bracket only every `every`-th launch that passes the filter (1 = all): a bracketed launch (start / stop events on the
 * kernel's own dispatch) is serialised against its neighbours, which a benchmark's timed region should pay on a sample,
 * not on every step.  launches / total_ms / alg_bytes then count the bracketed launches only.                          */
int isx_profile_sample(int every);
/* number of distinct kernel names seen; then name / launches / total milliseconds by index.
 * isx_profile_collect() synchronises the device and folds pending events into the totals.     */
int isx_profile_collect(void);
int isx_profile_count(int* n);
int isx_profile_entry(int index, const char** name, long long* launches, double* total_ms,
                      double* alg_bytes /* algorithmic bytes summed over launches */);

#ifdef __cplusplus
}
#endif
#endif /* IMAGESTITCH_HIP_H */
