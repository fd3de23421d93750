"""Exposure compensation of the reference's main() (W:238-244): cv::detail::GainCompensator, what
ExposureCompensator::createDefault(ExposureCompensator::GAIN) returns - feed() estimates one gain per tile on the GPU
(isx_gain_compensator_feed), apply() multiplies a tile by its gain (isx_gain_apply) - and cv::detail::BlocksGainCompensator, what
createDefault(ExposureCompensator::GAIN_BLOCKS) returns: one gain per block of every tile, solved on the GPU (isx_blocks_gain_feed), applied
as a smoothed gain map resized to the tile (isx_blocks_gain_apply)."""
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


class IsxBlockPair(C.Structure):
    """isx_block_pair: the statistics of one pair of blocks of different images whose rectangles meet."""
    _fields_ = [("block_i", C.c_int), ("block_j", C.c_int), ("n", C.c_longlong), ("i_ij", C.c_double), ("i_ji", C.c_double)]


BLOCK_PAIR_DTYPE = np.dtype([("block_i", np.int32), ("block_j", np.int32), ("n", np.int64), ("i_ij", np.float64), ("i_ji", np.float64)])


class BlocksGainCompensator:
    """cv::detail::BlocksGainCompensator(bl_width, bl_height): feed(corners, images_warped, masks_warped) then
    apply(i, corners[i], images_warped[i], masks_warped[i]) (W:238-244).  The gain maps live on the device in the handle."""

    def __init__(self, bl_width=32, bl_height=32, device=0, stream=None):
        self.device, self.stream = device, stream
        self._h = C.c_void_p()
        check(_lib.load().isx_blocks_gain_create(int(bl_width), int(bl_height), int(device), C.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:       # (at interpreter exit the module may be gone already)
            _lib._lib.isx_blocks_gain_destroy(h)

    def _stream(self):
        return C.c_void_p(getattr(self.stream, "cuda_stream", self.stream) or 0)

    def feed(self, corners, images, masks):
        """corners: n (x, y); images: n CV_8UC3 (HxWx3 uint8) arrays or tensors; masks: n CV_8U masks of the images' sizes (255 = in)."""
        n, mats_i, c, mats_m, ptr = tile_args(images, corners, masks, self.stream, who="feed")
        check(_lib.load().isx_blocks_gain_feed(self._h, n, c, mats_i, mats_m, ptr))
        return self

    def apply(self, index, corner, image, mask=None):
        """BlocksGainCompensator::apply: the image times its gain map resized to it, in place; corner and mask are unused, as in OpenCV."""
        del corner, mask
        mi = _lib.as_mat(image)
        check(_lib.load().isx_blocks_gain_apply(self._h, int(index), C.byref(mi), self._stream()))
        return image

    def _counts(self):
        n, nb = C.c_int(), C.c_int()
        check(_lib.load().isx_blocks_gain_num_images(self._h, C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def block_counts(self):
        """(nx, ny) of every image fed."""
        n, _ = self._counts()
        out = (C.c_int * (2 * n))()
        check(_lib.load().isx_blocks_gain_block_counts(self._h, out))
        return [(out[2 * i], out[2 * i + 1]) for i in range(n)]

    def gains(self):
        """The raw gains of the solve, one float64 per block (blocks numbered image by image, rows of blocks outer)."""
        _, nb = self._counts()
        g = np.zeros(nb, np.float64)
        check(_lib.load().isx_blocks_gain_gains(self._h, g.ctypes.data_as(C.POINTER(C.c_double))))
        return g

    def gain_maps(self):
        """The smoothed gain map of every image: ny x nx float32 (gain_map_ of BlocksGainCompensator)."""
        maps = []
        for i, (nx, ny) in enumerate(self.block_counts()):
            m = np.zeros((ny, nx), np.float32)
            mm = _lib.as_mat(m)
            check(_lib.load().isx_blocks_gain_map(self._h, i, C.byref(mm), self._stream()))
            maps.append(m)
        return maps

    def block_stats(self):
        """(pairs, diag_n): the off-diagonal statistics as a structured array (block_i, block_j, n, i_ij, i_ji), one record per pair of
        blocks of different images that meet, and N(k, k) per block (int64).  Never a blocks x blocks array."""
        _, nb = self._counts()
        cnt = C.c_longlong()
        check(_lib.load().isx_blocks_gain_stats(self._h, C.byref(cnt), None, 0, None))
        pairs = np.zeros(cnt.value, BLOCK_PAIR_DTYPE)
        diag = np.zeros(nb, np.int64)
        check(_lib.load().isx_blocks_gain_stats(self._h, C.byref(cnt), C.c_void_p(pairs.ctypes.data), cnt.value, diag.ctypes.data_as(C.POINTER(C.c_longlong))))
        return pairs, diag

    def feed_times(self):
        """Host wall-clock milliseconds of the last feed: statistics, assembly, LU, back substitution."""
        ms = (C.c_double * 4)()
        check(_lib.load().isx_blocks_gain_feed_times(self._h, ms))
        return dict(zip(("statistics", "assembly", "lu", "back_substitution"), ms))


def lu_solve(A, b, where="device", device=0):
    """isx_selftest_lu_solve: (x, swaps) of the dense solver alone, on the device or by the host's scalar code."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    n = b.size
    assert A.shape == (n, n)
    x = np.zeros(n, np.float64)
    swaps = C.c_int()
    dp = C.POINTER(C.c_double)
    check(_lib.load().isx_selftest_lu_solve(n, A.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp), C.byref(swaps),
                                            {"device": 0, "host": 1}[where], int(device)))
    return x, swaps.value
