"""Exposure compensation of the reference's main() (W:238-244): cv::detail::GainCompensator, what
ExposureCompensator::createDefault(ExposureCompensator::GAIN) returns - feed() estimates one gain per tile on the GPU
(isx_gain_compensator_feed), apply() multiplies a tile by its gain (isx_gain_apply)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, tile_args
from .blender import gain_apply


class GainCompensator:
    """compensator->feed(corners, images_warped, masks_warped) then compensator->apply(i, corners[i], images_warped[i], masks_warped[i])."""

    def __init__(self, device=0, stream=None):
        self.device, self.stream = device, stream
        self._gains = None
        self.N = None       # n x n int64: OpenCV's N (overlap pixel counts, at least 1), after feed()
        self.I = None       # n x n float64: OpenCV's I (mean intensity of image i over its overlap with j; diagonal 0), after feed()

    def feed(self, corners, images, masks):
        """corners: n (x, y); images: n CV_8UC3 (HxWx3 uint8) arrays or tensors; masks: n CV_8U masks of the images' sizes (255 = in)."""
        n, mats_i, c, mats_m, ptr = tile_args(images, corners, masks, self.stream, who="feed")
        gains = np.zeros(max(n, 1), np.float64)
        N = np.zeros((n, n), np.int64)
        I = np.zeros((n, n), np.float64)
        check(_lib.load().isx_gain_compensator_feed(n, c, mats_i, mats_m, gains.ctypes.data_as(C.POINTER(C.c_double)),
                                                    N.ctypes.data_as(C.POINTER(C.c_longlong)), I.ctypes.data_as(C.POINTER(C.c_double)),
                                                    int(self.device), ptr))
        self._gains, self.N, self.I = gains[:n], N, I
        return self

    def gains(self):
        """The gains feed() estimated (gains_ of GainCompensator), one float64 per tile."""
        if self._gains is None:
            raise _lib.IsxError(3, "gains: feed() has not run")
        return self._gains.copy()

    def apply(self, index, corner, image, mask=None):
        """GainCompensator::apply: multiply(image, gains_(index, 0), image) in place; corner and mask are unused, as in OpenCV."""
        del corner, mask
        if self._gains is None:
            raise _lib.IsxError(3, "apply: feed() has not run")
        return gain_apply(image, float(self._gains[index]), self.device, self.stream)
