"""The reference's features finder (F = its 特征点检测 demo): OrbFeaturesFinder(grid_size, n_features, scaleFactor, nlevels) and
find(image, features) (F:40-44, F:948-1017) on the GPU (isx_orb_find, DESIGN.md §8 "Features finder").  The sampling pattern is an input: the
default is makeRandomPattern(31) (F:709-718); a caller who has OpenCV's learned table passes it through set_pattern.
SurfFeaturesFinder is the finder every main of the reference comments out (isx_surf_find, DESIGN.md §8 "Features finder, SURF"): 64 float32
a keypoint, which FeaturesMatcher sends to the L2 entry.  SiftFeaturesFinder is the finder cv::Stitcher and stitching_detailed --features sift
offer beside them (isx_sift_find, DESIGN.md §8 "Features finder, SIFT"): 128 float32 a keypoint, the same entry."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import IsxMat, as_mat, check
from .matcher import _allocator, _is_device, _synchronize

# ISX_ORB_* of include/imagestitch_hip.h
MAX_LEVELS, CAND_TIE_ROOM, KEEP_TIE_ROOM, MAX_CANDIDATES = 8, 256, 32, 4096
TRUNCATED, BAD_PATTERN = 1, 2
HARRIS_SCORE, FAST_SCORE = 0, 1


class OrbParams(C.Structure):
    """isx_orb_params"""
    _fields_ = [("grid_width", C.c_int), ("grid_height", C.c_int), ("n_features", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("edge_threshold", C.c_int), ("first_level", C.c_int), ("wta_k", C.c_int), ("score_type", C.c_int), ("patch_size", C.c_int),
                ("fast_threshold", C.c_int)]


def default_params():
    p = OrbParams()
    check(_lib.load().isx_orb_default_params(C.byref(p)))
    return p


def capacity(params):
    """isx_orb_capacity: the rows the outputs of a find need"""
    n = C.c_int()
    check(_lib.load().isx_orb_capacity(C.byref(params), C.byref(n)))
    return n.value


def default_pattern():
    """isx_orb_default_pattern: the 512 x 2 int32 points a None pattern means"""
    out = np.empty((512, 2), np.int32)
    check(_lib.load().isx_orb_default_pattern(C.byref(as_mat(out))))
    return out


def orb_find(image, params, keypoints, meta, descriptors, count_status, pattern=None, device=0, stream=None):
    """isx_orb_find on caller-allocated outputs: keypoints cap x 2 and meta cap x 4 float32, descriptors cap x 32 uint8, count_status 1 x 2
    int32, NumPy arrays or CUDA tensors; image: uint8 HxW, HxWx3 or HxWx4."""
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_orb_find(C.byref(as_mat(image)), C.byref(params), None if pattern is None else C.byref(as_mat(pattern)),
                                   C.byref(as_mat(keypoints)), C.byref(as_mat(meta)), C.byref(as_mat(descriptors)), C.byref(as_mat(count_status)),
                                   int(device), C.c_void_p(ptr or 0)))


def orb_reserve(params, width, height, device=0):
    """isx_orb_reserve: size the calling thread's scratch (and upload the default pattern) ahead of a stream capture"""
    check(_lib.load().isx_orb_reserve(C.byref(params), int(width), int(height), int(device)))


class ImageFeatures:
    """detail::ImageFeatures as find fills it: img_idx, img_size (width, height), keypoints n x 2 float32 (pt.x, pt.y), meta n x 4 float32
    (size, angle, response, octave), descriptors n x 32 uint8 - row-sliced views of the finder's mats, in canonical order (cell, level, y, x) -
    and status (ISX_ORB_TRUNCATED | ISX_ORB_BAD_PATTERN).  From SurfFeaturesFinder: meta n x 5 (laplacian last), descriptors n x 64 float32,
    strongest first, status (ISX_SURF_TRUNCATED | ISX_SURF_CANDIDATES_DROPPED).  From SiftFeaturesFinder: meta n x 5 (octave from -1, then the
    layer), descriptors n x 128 float32, strongest first, status (ISX_SIFT_TRUNCATED | ISX_SIFT_CANDIDATES_DROPPED)."""

    def __init__(self, img_idx, img_size, keypoints, meta, descriptors, status):
        self.img_idx, self.img_size, self.keypoints, self.meta, self.descriptors, self.status = img_idx, img_size, keypoints, meta, descriptors, status


class OrbFeaturesFinder:
    """OrbFeaturesFinder(Size grid_size = Size(3, 1), int nfeatures = 1500, float scaleFactor = 1.3f, int nlevels = 5) (F:40-54)."""

    def __init__(self, grid=(3, 1), n_features=1500, scale_factor=1.3, nlevels=5, device=0, stream=None):
        p = default_params()
        p.grid_width, p.grid_height, p.n_features, p.scale_factor, p.nlevels = int(grid[0]), int(grid[1]), int(n_features), float(scale_factor), int(nlevels)
        self.params, self.device, self.stream = p, device, stream
        self.pattern = None
        self.capacity = capacity(p)

    def set_pattern(self, pattern):
        """A 512 x 2 int32 array or CUDA tensor of (x, y) points inside the 31 x 31 patch (OpenCV's bit_pattern_31_, say); None: the default."""
        self.pattern = pattern

    def find(self, images):
        """find(image, features) for every image (uint8 HxW, HxWx3 or HxWx4; NumPy arrays or CUDA tensors): one ImageFeatures each.  With a
        CUDA image the outputs are CUDA tensors.  All counts are read back in one synchronisation."""
        out = []
        for i, img in enumerate(images):
            alloc = _allocator("cuda:%d" % int(self.device) if _is_device(img) else None)
            cap = max(self.capacity, 1)
            kp, meta, desc, cs = alloc(cap, 2, np.float32), alloc(cap, 4, np.float32), alloc(cap, 32, np.uint8), alloc(1, 2, np.int32)
            orb_find(img, self.params, kp, meta, desc, cs, self.pattern, self.device, self.stream)
            out.append((i, (int(img.shape[1]), int(img.shape[0])), kp, meta, desc, cs))
        if any(_is_device(o[5]) for o in out):
            _synchronize(self.stream, self.device)
        feats = []
        for i, size, kp, meta, desc, cs in out:
            c = cs.cpu().numpy()[0] if _is_device(cs) else cs[0]
            n = int(c[0])
            feats.append(ImageFeatures(i, size, kp[:n], meta[:n], desc[:n], int(c[1])))
        return feats

    __call__ = find

    def reserve(self, width, height):
        orb_reserve(self.params, width, height, self.device)

    @staticmethod
    def release():
        """Return the scratch the finder keeps per calling thread between calls (isx_orb_release)."""
        check(_lib.load().isx_orb_release())


# ISX_SURF_* of include/imagestitch_hip.h
SURF_MAX_CANDIDATES, SURF_MAX_SIDE, SURF_MAX_PIXELS = 32768, 16384, 1 << 24
SURF_TRUNCATED, SURF_CANDIDATES_DROPPED = 1, 2


class SurfParams(C.Structure):
    """isx_surf_params"""
    _fields_ = [("hess_thresh", C.c_double), ("num_octaves", C.c_int), ("num_layers", C.c_int), ("num_octaves_descr", C.c_int),
                ("num_layers_descr", C.c_int), ("extended", C.c_int), ("upright", C.c_int)]


def surf_default_params():
    p = SurfParams()
    check(_lib.load().isx_surf_default_params(C.byref(p)))
    return p


def surf_find(image, params, keypoints, meta, descriptors, count_status, device=0, stream=None):
    """isx_surf_find on caller-allocated outputs: keypoints cap x 2, meta cap x 5 and descriptors cap x 64 float32, count_status 1 x 2 int32,
    NumPy arrays or CUDA tensors; cap is the smallest of the three row counts; image: uint8 HxW, HxWx3 or HxWx4."""
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_surf_find(C.byref(as_mat(image)), C.byref(params), C.byref(as_mat(keypoints)), C.byref(as_mat(meta)),
                                    C.byref(as_mat(descriptors)), C.byref(as_mat(count_status)), int(device), C.c_void_p(ptr or 0)))


def surf_reserve(params, width, height, cap, device=0):
    """isx_surf_reserve: size the calling thread's scratch ahead of a stream capture"""
    check(_lib.load().isx_surf_reserve(C.byref(params), int(width), int(height), int(cap), int(device)))


class SurfFeaturesFinder:
    """SurfFeaturesFinder(double hess_thresh = 300., int num_octaves = 3, int num_layers = 4, int num_octaves_descr = 3,
    int num_layers_descr = 4) of OpenCV 3.4.2's stitching module.  max_keypoints is the row count of the outputs (cap): the strongest
    max_keypoints keypoints are returned and ISX_SURF_TRUNCATED says that there were more."""

    def __init__(self, hess_thresh=300., num_octaves=3, num_layers=4, num_octaves_descr=3, num_layers_descr=4, max_keypoints=4096, device=0,
                 stream=None):
        p = surf_default_params()
        p.hess_thresh, p.num_octaves, p.num_layers = float(hess_thresh), int(num_octaves), int(num_layers)
        p.num_octaves_descr, p.num_layers_descr = int(num_octaves_descr), int(num_layers_descr)
        self.params, self.device, self.stream, self.capacity = p, device, stream, int(max_keypoints)

    def find(self, images):
        """find(image, features) for every image (uint8 HxW, HxWx3 or HxWx4; NumPy arrays or CUDA tensors): one ImageFeatures each.  With a
        CUDA image the outputs are CUDA tensors.  All counts are read back in one synchronisation."""
        out = []
        for i, img in enumerate(images):
            alloc = _allocator("cuda:%d" % int(self.device) if _is_device(img) else None)
            cap = self.capacity
            kp, meta, desc, cs = alloc(cap, 2, np.float32), alloc(cap, 5, np.float32), alloc(cap, 64, np.float32), alloc(1, 2, np.int32)
            surf_find(img, self.params, kp, meta, desc, cs, self.device, self.stream)
            out.append((i, (int(img.shape[1]), int(img.shape[0])), kp, meta, desc, cs))
        if any(_is_device(o[5]) for o in out):
            _synchronize(self.stream, self.device)
        feats = []
        for i, size, kp, meta, desc, cs in out:
            c = cs.cpu().numpy()[0] if _is_device(cs) else cs[0]
            n = int(c[0])
            feats.append(ImageFeatures(i, size, kp[:n], meta[:n], desc[:n], int(c[1])))
        return feats

    __call__ = find

    def reserve(self, width, height):
        surf_reserve(self.params, width, height, self.capacity, self.device)

    @staticmethod
    def release():
        """Return the scratch the finder keeps per calling thread between calls (isx_surf_release)."""
        check(_lib.load().isx_surf_release())


# ISX_SIFT_* of include/imagestitch_hip.h
SIFT_MAX_CANDIDATES, SIFT_MAX_SIDE, SIFT_MAX_PIXELS = 32768, 8192, 1 << 23
SIFT_TRUNCATED, SIFT_CANDIDATES_DROPPED = 1, 2


class SiftParams(C.Structure):
    """isx_sift_params"""
    _fields_ = [("nfeatures", C.c_int), ("n_octave_layers", C.c_int), ("contrast_threshold", C.c_double), ("edge_threshold", C.c_double),
                ("sigma", C.c_double)]


def sift_default_params():
    p = SiftParams()
    check(_lib.load().isx_sift_default_params(C.byref(p)))
    return p


def sift_find(image, params, keypoints, meta, descriptors, count_status, device=0, stream=None):
    """isx_sift_find on caller-allocated outputs: keypoints cap x 2, meta cap x 5 and descriptors cap x 128 float32, count_status 1 x 2 int32,
    NumPy arrays or CUDA tensors; cap is the smallest of the three row counts; image: uint8 HxW, HxWx3 or HxWx4."""
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_sift_find(C.byref(as_mat(image)), C.byref(params), C.byref(as_mat(keypoints)), C.byref(as_mat(meta)),
                                    C.byref(as_mat(descriptors)), C.byref(as_mat(count_status)), int(device), C.c_void_p(ptr or 0)))


def sift_reserve(params, width, height, cap, device=0):
    """isx_sift_reserve: size the calling thread's scratch ahead of a stream capture"""
    check(_lib.load().isx_sift_reserve(C.byref(params), int(width), int(height), int(cap), int(device)))


class SiftFeaturesFinder:
    """SIFT::create(int nfeatures = 0, int nOctaveLayers = 3, double contrastThreshold = 0.04, double edgeThreshold = 10, double sigma = 1.6)
    of OpenCV 4.x, the finder cv::Stitcher and stitching_detailed --features sift offer.  max_keypoints is the row count of the outputs (cap):
    the strongest max_keypoints keypoints are returned and ISX_SIFT_TRUNCATED says that there were more.  ImageFeatures: meta n x 5 (size,
    angle, response, octave from -1, layer), descriptors n x 128 float32, strongest first."""

    def __init__(self, nfeatures=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10, sigma=1.6, max_keypoints=4096, device=0, stream=None):
        p = sift_default_params()
        p.nfeatures, p.n_octave_layers = int(nfeatures), int(n_octave_layers)
        p.contrast_threshold, p.edge_threshold, p.sigma = float(contrast_threshold), float(edge_threshold), float(sigma)
        self.params, self.device, self.stream, self.capacity = p, device, stream, int(max_keypoints)

    def find(self, images):
        """find(image, features) for every image (uint8 HxW, HxWx3 or HxWx4; NumPy arrays or CUDA tensors): one ImageFeatures each.  With a
        CUDA image the outputs are CUDA tensors.  All counts are read back in one synchronisation."""
        out = []
        for i, img in enumerate(images):
            alloc = _allocator("cuda:%d" % int(self.device) if _is_device(img) else None)
            cap = self.capacity
            kp, meta, desc, cs = alloc(cap, 2, np.float32), alloc(cap, 5, np.float32), alloc(cap, 128, np.float32), alloc(1, 2, np.int32)
            sift_find(img, self.params, kp, meta, desc, cs, self.device, self.stream)
            out.append((i, (int(img.shape[1]), int(img.shape[0])), kp, meta, desc, cs))
        if any(_is_device(o[5]) for o in out):
            _synchronize(self.stream, self.device)
        feats = []
        for i, size, kp, meta, desc, cs in out:
            c = cs.cpu().numpy()[0] if _is_device(cs) else cs[0]
            n = int(c[0])
            feats.append(ImageFeatures(i, size, kp[:n], meta[:n], desc[:n], int(c[1])))
        return feats

    __call__ = find

    def reserve(self, width, height):
        sift_reserve(self.params, width, height, self.capacity, self.device)

    @staticmethod
    def release():
        """Return the scratch the finder keeps per calling thread between calls (isx_sift_release)."""
        check(_lib.load().isx_sift_release())
