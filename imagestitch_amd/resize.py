"""Seam finding at reduced scale: cv::resize and the compose loop's mask stage of OpenCV's stitching_detailed / Stitcher::composePanorama
(isx_resize, isx_mask_dilate_resize_and; between W:264 and W:302 of the reference's flow)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import INTER_LINEAR, IsxError, as_mat, check
from .warper import _empty_like_kind


def resize_dsize(src_w, src_h, fx, fy):
    """The dsize cv::resize derives from fx / fy: (cvRound(src_w * fx), cvRound(src_h * fy)), ties to even."""
    return int(round(float(src_w) * float(fx))), int(round(float(src_h) * float(fy)))


def resize(src, dsize=None, fx=0, fy=0, interpolation=INTER_LINEAR, dst=None, device=0, stream=None):
    """cv::resize(src, dst, dsize, fx, fy, interpolation): INTER_NEAREST or INTER_LINEAR on uint8 / float32 arrays of 1 or 3 channels.
    dsize is (width, height); None takes it from fx, fy.  Returns dst (same kind as src: numpy array or torch tensor)."""
    if dsize is None:
        if not (fx > 0 and fy > 0):
            raise IsxError(1, "resize: dsize is None and fx, fy are not both positive")
        dsize = resize_dsize(src.shape[1], src.shape[0], fx, fy)
    w, h = int(dsize[0]), int(dsize[1])
    if w <= 0 or h <= 0:
        raise IsxError(7, "resize: empty dsize %d x %d" % (w, h))
    if dst is None:
        dst = _empty_like_kind(src, (h, w) + tuple(src.shape[2:]), np.dtype(str(src.dtype).replace("torch.", "")))
    ms, md = as_mat(src), as_mat(dst)
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_resize(C.byref(ms), C.byref(md), int(interpolation), int(device), C.c_void_p(ptr or 0)))
    return dst


def dilate_resize_and(seam_mask, out_size_or_warped_mask, kw=3, kh=3, other=None, out=None, device=0, stream=None):
    """resize(dilate(seam_mask, MORPH_RECT kw x kh), size, INTER_LINEAR) [& warped_mask] in one launch: the compose loop's
    dilate(masks_warped[i], dilated_mask, Mat()); resize(dilated_mask, seam_mask, mask_warped.size()); mask_warped = seam_mask & mask_warped.
    The second argument is the full-size warped mask (the result has its size) or a (width, height); with a size, `other` may name the
    mask to AND with.  Returns out."""
    if isinstance(out_size_or_warped_mask, (tuple, list)):
        w, h = int(out_size_or_warped_mask[0]), int(out_size_or_warped_mask[1])
        warped = other
    else:
        if other is not None:
            raise IsxError(1, "dilate_resize_and: a warped mask and `other` are both given")
        warped = out_size_or_warped_mask
        h, w = int(warped.shape[0]), int(warped.shape[1])
    if w <= 0 or h <= 0:
        raise IsxError(7, "dilate_resize_and: empty size %d x %d" % (w, h))
    if out is None:
        out = _empty_like_kind(seam_mask, (h, w), np.uint8)
    mm, mo = as_mat(seam_mask), as_mat(out)
    mt = as_mat(warped) if warped is not None else None
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_mask_dilate_resize_and(C.byref(mm), C.byref(mt) if mt is not None else None, int(kw), int(kh), C.byref(mo), int(device),
                                                 C.c_void_p(ptr or 0)))
    return out
