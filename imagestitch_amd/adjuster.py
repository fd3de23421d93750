"""The reference's bundle adjuster (W = its cylindrical-projection demo, W:183-194; the same lines stand in its other demos):
adjuster = new detail::BundleAdjusterRay(); adjuster->setConfThresh(1); (*adjuster)(features, pairwise_matches, cameras) on the GPU
(isx_bundle_adjust_ray, DESIGN.md §8 "Bundle adjuster"): focal and rotation of every camera refined over the inlier matches, for every rig of
a matcher call in one launch, reading the mats of the matcher, the homography stage and the estimator where they lie.  OpenCV's
BundleAdjusterBase::estimate, CvLevMarq and cvRodrigues2 are restated; the solve is a Cholesky factorisation with SVBkSb's truncation rule,
sin / cos / acos are restated and the summation orders fixed, so parity with OpenCV is not pinned (tests/helpers/bundle_np.py is the
specification).

BundleAdjusterReproj (isx_bundle_adjust_reproj; tests/helpers/bundle_reproj_np.py) is the same call with OpenCV's reprojection cost - focal,
ppx, ppy, aspect and rotation of every camera, setRefinementMask - and waveCorrect (isx_wave_correct) straightens the refined rotations.
The reference comments both out (W:190, W:198); cv::Stitcher and stitching_detailed run them by default."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import as_mat, check
from .cameras import CameraList, CameraParams
from .matcher import _allocator, _is_device, _mat, _mats, _synchronize

# limits, the tile of the accumulation, status bits and rig_stats columns (ISX_BUNDLE_* of include/imagestitch_hip.h)
MAX_IMAGES, TILE = 64, 64
ST_NAN, ST_NO_EDGES, ST_EST_ASSERT, ST_SINGULAR_R, ST_DROPPED = 1, 2, 4, 8, 16
RIG_STATUS, RIG_ITERS, RIG_JAC_EVALS, RIG_ERR_EVALS, RIG_LAMBDA_LG10, RIG_EDGES, RIG_MATCHES = range(7)
DBL_EPSILON = 2.220446049250313e-16
# refine_flags of isx_bundle_adjust_reproj: OpenCV's refinement mask (0,0), (0,2), (1,1), (1,2) as bits; the rotation is always refined
REFINE_FOCAL, REFINE_PPX, REFINE_ASPECT, REFINE_PPY, REFINE_ALL = 1, 4, 8, 16, 31
WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT = 0, 1
WAVE_DEGENERATE, WAVE_SINGLE = 1, 2           # status bits of isx_wave_correct's rig_stats column 0: the rig passed through


def _adjust(who, refine_flags, img_sizes, keypoints, pairs, matches, masks, counts, stats, conf, est_rig_stats, cameras_in, cameras_out, kr32_out,
            rig_stats_out, rig_err_out, rig_first, conf_thresh, max_iter, eps, device, stream):
    """The call both adjusters share; refine_flags is None for isx_bundle_adjust_ray, which has no such argument."""
    n, npairs = len(img_sizes), len(pairs)
    if len(keypoints) != n or len(matches) != npairs or len(masks) != npairs:
        raise _lib.IsxError(1, who + ": keypoints, matches or masks differ in length from img_sizes / pairs")
    sizes = (C.c_int * max(2 * n, 1))(*[int(v) for s in img_sizes for v in s])
    pij = (C.c_int * max(2 * npairs, 1))(*[int(v) for p in pairs for v in p])
    nrigs = 1 if rig_first is None else len(rig_first) - 1
    first = None if rig_first is None else (C.c_int * len(rig_first))(*[int(v) for v in rig_first])
    info = (C.c_int * 2)()
    ptr = getattr(stream, "cuda_stream", stream)
    flags = () if refine_flags is None else (int(refine_flags),)
    check(getattr(_lib.load(), "isx_" + who)(
        n, sizes, _mats(keypoints), npairs, pij, _mats(matches), _mats(masks), C.byref(_mat(counts)), C.byref(_mat(stats)), C.byref(_mat(conf)),
        nrigs, first, C.byref(as_mat(est_rig_stats)), C.byref(as_mat(cameras_in)), float(conf_thresh), int(max_iter), float(eps), *flags,
        C.byref(as_mat(cameras_out)), C.byref(as_mat(kr32_out)), C.byref(as_mat(rig_stats_out)), C.byref(as_mat(rig_err_out)), info, int(device),
        C.c_void_p(ptr or 0)))
    return info[0], info[1]


def bundle_adjust_ray(img_sizes, keypoints, pairs, matches, masks, counts, stats, conf, est_rig_stats, cameras_in, cameras_out, kr32_out,
                      rig_stats_out, rig_err_out, rig_first=None, conf_thresh=1.0, max_iter=1000, eps=DBL_EPSILON, device=0, stream=None):
    """isx_bundle_adjust_ray on caller-allocated outputs.  img_sizes: (width, height) per image; keypoints: per image float32 n_i x 2; pairs:
    (from, to) with from < to inside one rig; matches, masks: per pair the matcher's int32 rows x 3 and the homography stage's uint8 rows x 1;
    counts, stats, conf: int32 1 x len(pairs), int32 len(pairs) x >= 2, float64 1 x len(pairs); est_rig_stats, cameras_in: the estimator's
    int32 rigs x 8 and float64 n x 16; cameras_out: float64 n x 16; kr32_out: float32 n x 18; rig_stats_out: int32 rigs x 8; rig_err_out:
    float64 rigs x 2.  NumPy arrays or CUDA tensors.  Returns (rigs processed, kernel launches)."""
    return _adjust("bundle_adjust_ray", None, img_sizes, keypoints, pairs, matches, masks, counts, stats, conf, est_rig_stats, cameras_in, cameras_out,
                   kr32_out, rig_stats_out, rig_err_out, rig_first, conf_thresh, max_iter, eps, device, stream)


def refine_flags_of(mask):
    """OpenCV's 3 x 3 refinement mask (setRefinementMask) or the flags themselves -> refine_flags.  IsxError(1) for another shape or flags
    outside [0, 31]."""
    m = np.asarray(mask)
    if m.shape == (3, 3):
        m = m != 0
        return (int(m[0, 0]) * 1) | (int(m[0, 1]) * 2) | (int(m[0, 2]) * 4) | (int(m[1, 1]) * 8) | (int(m[1, 2]) * 16)
    if m.shape != () or m.dtype.kind not in "iu" or not 0 <= int(m) <= 31:
        raise _lib.IsxError(1, "bundle_adjust_reproj: the refinement mask is neither 3 x 3 nor flags in [0, 31]")
    return int(m)


def bundle_adjust_reproj(img_sizes, keypoints, pairs, matches, masks, counts, stats, conf, est_rig_stats, cameras_in, cameras_out, kr32_out,
                         rig_stats_out, rig_err_out, rig_first=None, conf_thresh=1.0, max_iter=1000, eps=DBL_EPSILON, refine_flags=REFINE_ALL,
                         device=0, stream=None):
    """isx_bundle_adjust_reproj on caller-allocated outputs: bundle_adjust_ray's arguments and outputs, and refine_flags (REFINE_*; the
    rotation is always refined).  Returns (rigs processed, kernel launches)."""
    if isinstance(refine_flags, bool) or not isinstance(refine_flags, (int, np.integer)):
        raise _lib.IsxError(1, "bundle_adjust_reproj: refine_flags is not an integer")
    return _adjust("bundle_adjust_reproj", refine_flags, img_sizes, keypoints, pairs, matches, masks, counts, stats, conf, est_rig_stats, cameras_in,
                   cameras_out, kr32_out, rig_stats_out, rig_err_out, rig_first, conf_thresh, max_iter, eps, device, stream)


def wave_correct(cameras_in, cameras_out, kr32_out, rig_stats_out, rig_first=None, kind=WAVE_CORRECT_HORIZ, device=0, stream=None):
    """isx_wave_correct on caller-allocated outputs.  cameras_in, cameras_out: float64 n x 16; kr32_out: float32 n x 18; rig_stats_out: int32
    rigs x 2 (status bits WAVE_*, images).  NumPy arrays or CUDA tensors.  Returns (rigs processed, kernel launches)."""
    n = int(cameras_in.shape[0])
    nrigs = 1 if rig_first is None else len(rig_first) - 1
    first = None if rig_first is None else (C.c_int * len(rig_first))(*[int(v) for v in rig_first])
    info = (C.c_int * 2)()
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_wave_correct(n, nrigs, first, C.byref(as_mat(cameras_in)), int(kind), C.byref(as_mat(cameras_out)), C.byref(as_mat(kr32_out)),
                                       C.byref(as_mat(rig_stats_out)), info, int(device), C.c_void_p(ptr or 0)))
    return info[0], info[1]


def _camera_list(cams, kr, n, source=None):
    out = CameraList()
    for i in range(n):
        c = CameraParams(cams[i, 0], cams[i, 1], cams[i, 2], cams[i, 3], cams[i, 4:13].copy(), cams[i, 13:16].copy())
        c.K32, c.R32 = kr[i, 0:9].reshape(3, 3).copy(), kr[i, 9:18].reshape(3, 3).copy()
        if source is not None:
            c.parent, c.depth = source[i].parent, source[i].depth
        out.append(c)
    return out


_KINDS = {"horiz": WAVE_CORRECT_HORIZ, "vert": WAVE_CORRECT_VERT, WAVE_CORRECT_HORIZ: WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT: WAVE_CORRECT_VERT}


def waveCorrect(cameras, kind="horiz", rigs=None, device=0, stream=None):
    """detail::waveCorrect(rmats, kind) on the GPU for the cameras of an adjuster: `cameras` is a BundleAdjusterRay / BundleAdjusterReproj /
    HomographyBasedEstimator after its call - its last_outputs are read on the device, in stream order, with no host mat - or a CameraList.
    kind: "horiz", "vert" or WAVE_CORRECT_*; rigs: the number of images of each rig in order (None: one rig).  Returns a CameraList whose
    rig_stats holds isx_wave_correct's int32 rigs x 2 and whose last_outputs the raw mats (cameras, kr32, rig_stats)."""
    if kind not in _KINDS:
        raise _lib.IsxError(1, "waveCorrect: kind %r is neither 'horiz' nor 'vert'" % (kind,))
    source = None
    if hasattr(cameras, "last_outputs"):
        if cameras.last_outputs is None:
            raise _lib.IsxError(3, "waveCorrect: the adjuster has not run yet")
        cams_in = cameras.last_outputs[0]
    else:
        source = cameras
        cams_in = np.zeros((len(cameras), 16))
        for i, c in enumerate(cameras):
            cams_in[i, 0:4] = [c.focal, c.aspect, c.ppx, c.ppy]
            cams_in[i, 4:13], cams_in[i, 13:16] = np.asarray(c.R, np.float64).ravel(), np.asarray(c.t, np.float64).ravel()
    n = int(cams_in.shape[0])
    rig_first = None if rigs is None else [int(v) for v in np.concatenate([[0], np.cumsum([int(r) for r in rigs])])]
    nrigs = 1 if rigs is None else len(rigs)
    alloc = _allocator(cams_in.device if _is_device(cams_in) else None)
    cams, kr, rs = alloc(n, 16, np.float64), alloc(n, 18, np.float32), alloc(nrigs, 2, np.int32)
    info = wave_correct(cams_in, cams, kr, rs, rig_first, _KINDS[kind], device, stream)
    raw = (cams, kr, rs)
    if _is_device(cams):
        _synchronize(stream, device)
        cams, kr, rs = (a.cpu().numpy() for a in raw)
    out = _camera_list(cams, kr, n, source)
    out.rig_stats, out.last_outputs, out.last_info = rs, raw, info
    return out


def release():
    """Return the scratch the adjusters and isx_wave_correct keep per calling thread between calls (isx_bundle_release)."""
    check(_lib.load().isx_bundle_release())


class _BundleAdjusterBase:
    """What BundleAdjusterRay and BundleAdjusterReproj share: the parameters, setConfThresh, the call on a matcher and an estimator, last_*."""
    _name = None

    def _run(self, *args):
        raise NotImplementedError

    def __init__(self, conf_thresh=1.0, max_iter=1000, eps=DBL_EPSILON, device=0, stream=None):
        self.conf_thresh, self.max_iter, self.eps, self.device, self.stream = float(conf_thresh), int(max_iter), float(eps), device, stream
        self.last_rig_stats = self.last_rig_err = self.last_info = self.last_outputs = None

    def setConfThresh(self, conf_thresh):
        self.conf_thresh = float(conf_thresh)

    def __call__(self, img_sizes, keypoints, matcher, cameras, rigs=None):
        """img_sizes: (width, height) per image; keypoints: per image n_i x 2 float32 (what the matcher was given); matcher: a
        BestOf2NearestMatcher after match() - its mats are read where they lie; cameras: the HomographyBasedEstimator after its call - its
        last_outputs are read on the device - or the CameraList it returned (then est_rig_stats is the list's rig_stats); rigs: the number
        of images of each rig in order (None: one rig)."""
        lo = getattr(matcher, "last_outputs", None)
        if not lo or "H" not in lo or "matches" not in lo:
            raise _lib.IsxError(3, self._name + ": the matcher has not run a homography stage yet")
        n = len(img_sizes)
        on_device = _is_device(lo["conf"])
        if hasattr(cameras, "last_outputs"):
            if cameras.last_outputs is None:
                raise _lib.IsxError(3, self._name + ": the estimator has not run yet")
            cams_in, est_rs = cameras.last_outputs[0], cameras.last_outputs[3]
        else:
            cams_in = np.zeros((n, 16))
            for i, c in enumerate(cameras):
                cams_in[i, 0:4] = [c.focal, c.aspect, c.ppx, c.ppy]
                cams_in[i, 4:13], cams_in[i, 13:16] = np.asarray(c.R, np.float64).ravel(), np.asarray(c.t, np.float64).ravel()
            est_rs = np.ascontiguousarray(cameras.rig_stats, np.int32)
            if on_device:
                import torch
                cams_in, est_rs = torch.from_numpy(cams_in).to(lo["conf"].device), torch.from_numpy(est_rs).to(lo["conf"].device)
        rig_first = None if rigs is None else [int(v) for v in np.concatenate([[0], np.cumsum([int(r) for r in rigs])])]
        nrigs = 1 if rigs is None else len(rigs)
        alloc = _allocator(lo["conf"].device if on_device else None)
        cams, kr, rs, re = alloc(n, 16, np.float64), alloc(n, 18, np.float32), alloc(nrigs, 8, np.int32), alloc(nrigs, 2, np.float64)
        self.last_info = self._run(img_sizes, keypoints, lo["pairs"], lo["matches"], lo["masks"], lo["counts"], lo["stats"], lo["conf"], est_rs,
                                   cams_in, cams, kr, rs, re, rig_first)
        self.last_outputs = (cams, kr, rs, re)
        if _is_device(cams):       # the one small read-back, which the warper's host-side ROI needs
            _synchronize(self.stream, self.device)
            cams, kr, rs, re = (a.cpu().numpy() for a in (cams, kr, rs, re))
        self.last_rig_stats, self.last_rig_err = rs, re
        out = _camera_list(cams, kr, n, None if hasattr(cameras, "last_outputs") else cameras)
        out.rig_stats = rs
        return out

    @staticmethod
    def release():
        """Return the scratch the stage keeps per calling thread (isx_bundle_release)."""
        release()


class BundleAdjusterRay(_BundleAdjusterBase):
    """detail::BundleAdjusterRay (W:189-194).  adjuster(img_sizes, keypoints, matcher, cameras) returns a CameraList whose rig_stats
    attribute holds the int32 rigs x 8 stats of the adjuster (also kept as last_rig_stats, beside last_rig_err: the first and last |err| per
    rig); last_info is (rigs, launches) and last_outputs the raw mats (cameras, kr32, rig_stats, rig_err: CUDA tensors where the inputs
    were)."""
    _name = "BundleAdjusterRay"

    def _run(self, *args):
        return bundle_adjust_ray(*args, self.conf_thresh, self.max_iter, self.eps, self.device, self.stream)


class BundleAdjusterReproj(_BundleAdjusterBase):
    """detail::BundleAdjusterReproj (commented out at W:190; cv::Stitcher's default): BundleAdjusterRay's call, results and last_*, with
    focal, ppx, ppy, aspect and rotation refined over the reprojection error.  setRefinementMask takes OpenCV's 3 x 3 mask or REFINE_* flags."""
    _name = "BundleAdjusterReproj"

    def __init__(self, conf_thresh=1.0, max_iter=1000, eps=DBL_EPSILON, device=0, stream=None, refine_flags=REFINE_ALL):
        super().__init__(conf_thresh, max_iter, eps, device, stream)
        self.refine_flags = refine_flags_of(refine_flags)

    def setRefinementMask(self, mask):
        self.refine_flags = refine_flags_of(mask)

    def _run(self, *args):
        return bundle_adjust_reproj(*args, self.conf_thresh, self.max_iter, self.eps, self.refine_flags, self.device, self.stream)
