"""The reference's HomographyBasedEstimator1 (C = its 恢复相机内参数 demo, C:26-105, C:145-284, C:313-321): a focal per rig from the pairwise
homographies, a maximum spanning tree over the inlier counts and the rotations along it, on the GPU (isx_estimate_cameras, DESIGN.md §8
"Camera estimator").  It reads H and stats where the homography stage left them; Mat::inv(), Mat * Mat, CameraParams and
Graph::walkBreadthFirst are restated and the order of equal-weight edges is fixed (weight descending, then i * n + j), so parity with OpenCV
is not pinned (tests/helpers/estimator_np.py is the specification)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import as_mat, check
from .matcher import _allocator, _is_device, _mat, _synchronize

# limits, status bits and rig_stats columns (ISX_ESTIMATOR_* of include/imagestitch_hip.h)
MAX_IMAGES = 64
ST_MEDIAN, ST_ASSERT, ST_UNREACHED = 1, 2, 4
RIG_STATUS, RIG_CANDIDATES, RIG_CENTER0, RIG_CENTER1, RIG_TREE_EDGES, RIG_REACHED, RIG_NUM_CENTERS, RIG_MIN_MAX_DIST = range(8)


def estimate_cameras(img_sizes, pairs, H, stats, conf, cameras, kr32, tree, rig_stats, rig_first=None, focals_in=None, device=0, stream=None):
    """isx_estimate_cameras on caller-allocated outputs.  img_sizes: (width, height) per image; pairs: (from, to) with from < to inside one
    rig; H, stats, conf: the homography stage's mats (float64 3 len(pairs) x 3, int32 len(pairs) x >= 2, float64 1 x len(pairs)); rig_first:
    len(rigs) + 1 image offsets, None = one rig; focals_in: None, or float64 n x 4 (focal, aspect, ppx, ppy: is_focals_estimated); cameras:
    float64 n x 16; kr32: float32 n x 18; tree: int32 n x 2; rig_stats: int32 rigs x 8.  NumPy arrays or CUDA tensors.  Returns (rigs
    processed, kernel launches)."""
    n, npairs = len(img_sizes), len(pairs)
    sizes = (C.c_int * max(2 * n, 1))(*[int(v) for s in img_sizes for v in s])
    pij = (C.c_int * max(2 * npairs, 1))(*[int(v) for p in pairs for v in p])
    nrigs = 1 if rig_first is None else len(rig_first) - 1
    first = None if rig_first is None else (C.c_int * len(rig_first))(*[int(v) for v in rig_first])
    info = (C.c_int * 2)()
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_estimate_cameras(
        n, sizes, npairs, pij, nrigs, first, C.byref(_mat(H)), C.byref(_mat(stats)), C.byref(_mat(conf)),
        None if focals_in is None else C.byref(as_mat(focals_in)), C.byref(as_mat(cameras)), C.byref(as_mat(kr32)), C.byref(as_mat(tree)),
        C.byref(as_mat(rig_stats)), info, int(device), C.c_void_p(ptr or 0)))
    return info[0], info[1]


def release():
    """Return the scratch isx_estimate_cameras keeps per calling thread between calls (isx_estimator_release)."""
    check(_lib.load().isx_estimator_release())


class CameraParams:
    """detail::CameraParams: focal, aspect, ppx, ppy, R (3 x 3 float64), t (3 x 1 float64), K(); K32 and R32 are K() and R as
    convertTo(CV_32F) gives them (C:329-334, C:385-386) - what RotationWarper takes.  parent and depth: the camera's place in the walk from
    the tree's center (-1 the root, -2 not reached; an index inside the rig)."""

    def __init__(self, focal=1.0, aspect=1.0, ppx=0.0, ppy=0.0, R=None, t=None):
        self.focal, self.aspect, self.ppx, self.ppy = float(focal), float(aspect), float(ppx), float(ppy)
        self.R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
        self.t = np.zeros((3, 1)) if t is None else np.asarray(t, np.float64).reshape(3, 1)
        self.K32, self.R32, self.parent, self.depth = None, None, -2, -1

    def K(self):
        """CameraParams::K()."""
        k = np.eye(3)
        k[0, 0], k[0, 2], k[1, 1], k[1, 2] = self.focal, self.ppx, self.focal * self.aspect, self.ppy
        return k


class CameraList(list):
    """The list of CameraParams a HomographyBasedEstimator call returns, with the call's per-rig stats: rig_stats, int32 rigs x 8 (the
    RIG_* columns; column 0 the ST_* bits)."""
    rig_stats = None


class HomographyBasedEstimator:
    """HomographyBasedEstimator1(is_focals_estimated) (C:132-144, C:246-284).  estimator(img_sizes, matcher_or_mats, cameras=None, rigs=None)
    returns a list of CameraParams whose rig_stats attribute holds the int32 rigs x 8 stats (also kept as last_rig_stats); last_info is
    (rigs, launches) and last_outputs the raw mats (cameras, kr32, tree, rig_stats: CUDA tensors where the inputs were)."""

    def __init__(self, is_focals_estimated=False, device=0, stream=None):
        self.is_focals_estimated, self.device, self.stream = bool(is_focals_estimated), device, stream
        self.last_rig_stats = self.last_info = self.last_outputs = None

    def __call__(self, img_sizes, matcher_or_mats, cameras=None, rigs=None):
        """img_sizes: (width, height) per image.  matcher_or_mats: a BestOf2NearestMatcher after match() - its device (or host) mats are
        read where they lie - or the tuple (pairs, H, stats, conf).  cameras: with is_focals_estimated the CameraParams (or an n x 4 array of
        focal, aspect, ppx, ppy) that come in.  rigs: the number of images of each rig in order (None: one rig); the matcher's mask must have
        kept every pair inside one rig."""
        if hasattr(matcher_or_mats, "last_outputs"):
            lo = matcher_or_mats.last_outputs
            if not lo or "H" not in lo:
                raise _lib.IsxError(3, "HomographyBasedEstimator: the matcher has not run a homography stage yet")
            pairs, H, stats, conf = lo["pairs"], lo["H"], lo["stats"], lo["conf"]
        else:
            pairs, H, stats, conf = matcher_or_mats
        n = len(img_sizes)
        rig_first = None if rigs is None else [int(v) for v in np.concatenate([[0], np.cumsum([int(r) for r in rigs])])]
        nrigs = 1 if rigs is None else len(rigs)
        fin = None
        if self.is_focals_estimated:
            if cameras is None:
                raise _lib.IsxError(1, "HomographyBasedEstimator: is_focals_estimated needs the cameras")
            fin = np.ascontiguousarray([[c.focal, c.aspect, c.ppx, c.ppy] for c in cameras] if isinstance(cameras[0], CameraParams)
                                       else cameras, np.float64).reshape(n, 4)
        alloc = _allocator(H.device if _is_device(H) else None)
        if fin is not None and _is_device(H):
            import torch
            fin = torch.from_numpy(fin).to(H.device)
        cams, kr, tree, rs = alloc(n, 16, np.float64), alloc(n, 18, np.float32), alloc(n, 2, np.int32), alloc(nrigs, 8, np.int32)
        self.last_info = estimate_cameras(img_sizes, pairs, H, stats, conf, cams, kr, tree, rs, rig_first, fin, self.device, self.stream)
        self.last_outputs = (cams, kr, tree, rs)
        if _is_device(cams):       # the one small read-back, which the warper's host-side ROI needs
            _synchronize(self.stream, self.device)
            cams, kr, tree, rs = (a.cpu().numpy() for a in (cams, kr, tree, rs))
        self.last_rig_stats = rs
        out = CameraList()
        out.rig_stats = rs
        for i in range(n):
            c = CameraParams(cams[i, 0], cams[i, 1], cams[i, 2], cams[i, 3], cams[i, 4:13].copy(), cams[i, 13:16].copy())
            c.K32, c.R32 = kr[i, 0:9].reshape(3, 3).copy(), kr[i, 9:18].reshape(3, 3).copy()
            c.parent, c.depth = int(tree[i, 0]), int(tree[i, 1])
            out.append(c)
        return out

    @staticmethod
    def release():
        """Return the scratch the stage keeps per calling thread (isx_estimator_release)."""
        release()
