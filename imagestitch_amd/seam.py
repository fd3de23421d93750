"""The data-parallel part of the reference's in-tree DP seam finder: estimateSeam S:806-957 with
computeCosts S:733-803 (both cost functions, S:71; COLOR_GRAD with computeGradients S:549-572) — gradient maps, cost maps and dynamic
programme on the GPU.  The component analysis around it stays with the caller."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import as_mat, check, tile_args


DP_COLOR, DP_COLOR_GRAD = 0, 1           # DpSeamFinder::CostFunction (S:71)


def seam_estimate(image1, image2, tl1, tl2, union_tl, labels, label, roi, p1, p2, device=0, stream=None, cost_func=DP_COLOR):
    """estimateSeam(image1, image2, tl1, tl2, comp, p1, p2, seam, isHorizontal).  labels = labels_ (HxW int32, union-sized),
    label = comp + 1, roi = (x, y, width, height) of Rect(tls_[comp], brs_[comp]); points are (x, y) in union coordinates.
    cost_func = DP_COLOR or DP_COLOR_GRAD (costFunc_, S:765-772 / S:790-797).
    Returns (seam as an (N, 2) int32 array, p1 first — empty when p2 is not reachable —, is_horizontal)."""
    m1, m2, ml = as_mat(image1), as_mat(image2), as_mat(labels)
    cap = int(roi[2]) + int(roi[3]) + 2
    out = np.zeros((cap, 2), np.int32)
    n, horiz = C.c_int(0), C.c_int(0)
    r = (C.c_int * 4)(*[int(v) for v in roi])
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_seam_estimate_cost(C.byref(m1), C.byref(m2), int(tl1[0]), int(tl1[1]), int(tl2[0]), int(tl2[1]), int(union_tl[0]), int(union_tl[1]),
                                             C.byref(ml), int(label), r, int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1]),
                                             out.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n), C.byref(horiz), int(cost_func), int(device),
                                             C.c_void_p(ptr or 0)))
    return out[: n.value].copy(), bool(horiz.value)


def seam_gradients(image, rect=None, device=0, stream=None, out=None):
    """The gradient maps of computeGradients S:549-572 as magnitudes: (|Sobel(gray, CV_32F, 1, 0)|, |Sobel(gray, CV_32F, 0, 1)|) of
    gray = cvtColor(image, COLOR_BGR2GRAY) over rect = (x, y, width, height) of the image (default: all of it); the values are those of
    the whole image's maps.  image: CV_32FC3 or CV_8UC3 array / tensor.  Returns two float32 maps of the rectangle's size: tensors on the
    image's device for a device image, NumPy arrays otherwise - or the pair given as `out`, filled."""
    m = as_mat(image)
    if rect is None:
        rect = (0, 0, m.cols, m.rows)
    w, h = int(rect[2]), int(rect[3])
    if out is None:
        if m.device >= 0:
            import torch
            out = tuple(torch.empty((max(h, 0), max(w, 0)), dtype=torch.float32, device=image.device) for _ in range(2))
        else:
            out = tuple(np.empty((max(h, 0), max(w, 0)), np.float32) for _ in range(2))
    gx, gy = as_mat(out[0]), as_mat(out[1])
    r = (C.c_int * 4)(*[int(v) for v in rect])
    ptr = getattr(stream, "cuda_stream", stream)
    check(_lib.load().isx_seam_gradients(C.byref(m), r, C.byref(gx), C.byref(gy), int(device), C.c_void_p(ptr or 0)))
    return out[0], out[1]


class DpSeamFinder:
    """The reference's in-tree DP seam finder (S:60-1093, `find` as called at S:1192): DpSeamFinder(DP_COLOR), the default (W:253), or
    DpSeamFinder(DP_COLOR_GRAD), the alternative every demo lists (W:255, S:1183)."""

    def __init__(self, cost_func=DP_COLOR, device=0, stream=None):
        self.cost_func, self.device, self.stream = int(cost_func), device, stream

    def costFunction(self):
        return self.cost_func

    def find(self, src, corners, masks):
        """find(src, corners, masks): src = CV_32FC3 (or CV_8UC3) images, masks = CV_8U arrays / tensors edited in place."""
        n, mats_i, c, mats_m, ptr = tile_args(src, corners, masks, self.stream)
        check(_lib.load().isx_dp_seam_find_cost(n, mats_i, c, mats_m, self.cost_func, int(self.device), ptr))
        return masks

    @staticmethod
    def release():
        """Return the work images the finder keeps per calling thread between find() calls (isx_dp_seam_release)."""
        check(_lib.load().isx_dp_seam_release())


COST_COLOR, COST_COLOR_GRAD = 0, 1       # GraphCutSeamFinder::CostType


class GraphCutSeamFinder:
    """The stock seam finder of the reference's main(): GraphCutSeamFinder(GraphCutSeamFinder::COST_COLOR) (W:257), find at W:264, or
    GraphCutSeamFinder(COST_COLOR_GRAD), the other graph cut every demo lists (W:258; CV_32FC3 tiles only).
    Every pair's max-flow runs on the GPU (isx_graphcut_seam_find); the cut is the maximal minimum cut."""

    FLOW_SHIFT = 23                      # COST_COLOR_GRAD flows and residuals are in units of 2^-23

    def __init__(self, cost_type=COST_COLOR, device=0, stream=None):
        self.cost_type, self.device, self.stream = int(cost_type), device, stream

    def find(self, src, corners, masks):
        """find(src, corners, masks): src = CV_32FC3 tiles holding integers in [0, 255] (W:261) or, with COST_COLOR only, CV_8UC3 tiles;
        masks = CV_8U arrays / tensors edited in place."""
        n, mats_i, c, mats_m, ptr = tile_args(src, corners, masks, self.stream)
        check(_lib.load().isx_graphcut_seam_find(n, mats_i, c, mats_m, self.cost_type, int(self.device), ptr))
        return masks

    def find_pair(self, image1, image2, tl1, tl2, mask1, mask2, certificate=False, wide=False):
        """One pair as find() treats it (masks edited in place).  Returns a dict: flow, flow_scale (1, or 1 << 23 with COST_COLOR_GRAD:
        flow and residuals are multiples of 1 / flow_scale), rows, cols, rounds, launches and, with certificate=True, residuals (rows x
        cols x 6: right, left, down, up, source link, sink link; int32 from isx_graphcut_seam_find_pair, int64 from
        isx_graphcut_seam_find_pair64 with COST_COLOR_GRAD or wide=True) and labels (rows x cols uint8, 1 = source side)."""
        wide = bool(wide) or self.cost_type == COST_COLOR_GRAD
        m1, m2, k1, k2 = as_mat(image1), as_mat(image2), as_mat(mask1), as_mat(mask2)
        c = (C.c_int * 4)(int(tl1[0]), int(tl1[1]), int(tl2[0]), int(tl2[1]))
        x0, y0 = max(tl1[0], tl2[0]), max(tl1[1], tl2[1])
        x1, y1 = min(tl1[0] + m1.cols, tl2[0] + m2.cols), min(tl1[1] + m1.rows, tl2[1] + m2.rows)
        nodes = max(0, y1 - y0 + 20) * max(0, x1 - x0 + 20) if (x0 < x1 and y0 < y1) else 0
        res = np.zeros((max(nodes, 1), 6), np.int64 if wide else np.int32) if certificate else None
        lab = np.zeros(max(nodes, 1), np.uint8) if certificate else None
        flow, info = C.c_longlong(0), (C.c_int * 4)()
        ptr = getattr(self.stream, "cuda_stream", self.stream)
        entry = _lib.load().isx_graphcut_seam_find_pair64 if wide else _lib.load().isx_graphcut_seam_find_pair
        check(entry(
            C.byref(m1), C.byref(m2), c, C.byref(k1), C.byref(k2), self.cost_type, C.byref(flow),
            res.ctypes.data_as(C.POINTER(C.c_longlong if wide else C.c_int)) if certificate else None,
            lab.ctypes.data_as(C.POINTER(C.c_ubyte)) if certificate else None, nodes, info, int(self.device), C.c_void_p(ptr or 0)))
        out = dict(flow=flow.value, flow_scale=1 << self.FLOW_SHIFT if self.cost_type == COST_COLOR_GRAD else 1, rows=info[0], cols=info[1],
                   rounds=info[2], launches=info[3])
        if certificate:
            out["residuals"] = res[: info[0] * info[1]].reshape(info[0], info[1], 6)
            out["labels"] = lab[: info[0] * info[1]].reshape(info[0], info[1])
        return out

    @staticmethod
    def release():
        """Return the graph and staging buffers the finder keeps per calling thread between calls (isx_graphcut_seam_release)."""
        check(_lib.load().isx_graphcut_seam_release())


class VoronoiSeamFinder:
    """The S demo's seam finder: makePtr<detail::VoronoiSeamFinder>() (S:1180), find at S:1192.  Masks only - two city-block distance
    transforms and a compare per overlapping pair (isx_voronoi_seam_find).  On device masks nothing is synchronised, so find
    can be captured into a hipGraph on `stream` once reserve() has sized the scratch."""

    def __init__(self, device=0, stream=None):
        self.device, self.stream = device, stream

    def find(self, src_or_sizes, corners, masks):
        """find(src, corners, masks) or find(sizes, corners, masks): the images are never read, only their sizes ((width, height) pairs,
        or anything with a .shape of rows x cols [x channels]); masks = CV_8U arrays / tensors edited in place."""
        n, _, c, mats_m, ptr = tile_args(src_or_sizes, corners, masks, self.stream, images=False)
        sizes = [(int(a.shape[1]), int(a.shape[0])) if hasattr(a, "shape") else (int(a[0]), int(a[1])) for a in src_or_sizes]
        sz = (C.c_int * max(2 * n, 1))(*[v for s in sizes for v in s])
        check(_lib.load().isx_voronoi_seam_find(n, sz, c, mats_m, int(self.device), ptr))
        return masks

    def reserve(self, max_roi_width, max_roi_height):
        """Size the calling thread's scratch for overlaps of up to max_roi_width x max_roi_height before a capture
        (isx_voronoi_seam_reserve); it must then stay as it is while the captured graph exists."""
        check(_lib.load().isx_voronoi_seam_reserve(int(max_roi_width), int(max_roi_height), int(self.device)))
        return self

    @staticmethod
    def release():
        """Return the scratch the finder keeps per calling thread between find() calls (isx_voronoi_seam_release)."""
        check(_lib.load().isx_voronoi_seam_release())
