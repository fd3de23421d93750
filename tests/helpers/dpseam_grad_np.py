"""NumPy model of the in-tree DP seam finder with BOTH cost functions (S = 动态规划法寻找最佳缝合线.cpp, `enum CostFunction { COLOR,
COLOR_GRAD }` S:71): the specification isx_dp_seam_find_cost / isx_seam_estimate_cost / isx_seam_gradients are compared with, bit for bit.

TEST INFRASTRUCTURE ONLY.  oracle/dpseam_np.py restates everything of `find` around estimateSeam and hands estimateSeam itself to the C
oracle, which knows COLOR only; this subclass replaces that one step by a NumPy restatement of computeGradients S:549-572, computeCosts
S:733-803 and estimateSeam S:806-957.  Written from S and the evaluation order DESIGN.md §8 fixes, not from the kernels:

  gray   cvtColor(COLOR_BGR2GRAY): CV_32FC3 (b * 0.114f + g * 0.587f) + r * 0.299f; CV_8UC3 (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14
  Sobel  3 x 3, scale 1, delta 0, BORDER_REFLECT_101 at the image's edges (a dimension of size 1 reads index 0), row pass then column pass:
         gradx: d(y, x) = g(y, x + 1) - g(y, x - 1),                        then (d(y - 1, x) + d(y + 1, x)) + (d(y, x) + d(y, x))
         grady: s(y, x) = (g(y, x - 1) + g(y, x + 1)) + (g(y, x) + g(y, x)), then s(y + 1, x) - s(y - 1, x)
  cost   COLOR_GRAD: costColor / costGrad, costGrad = |g(., x)| + |g(., x - 1)| of image 1, then of image 2, + 1.f, added left to right

Every float operation is one NumPy float32 ufunc call, so nothing is fused and every result is rounded once, as in S."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import dpseam_np  # noqa: E402

COLOR, COLOR_GRAD = 0, 1
F = np.float32
BAD_REGION_COST = F(3.0 * 255.0 * 255.0)        # normL2(Point3f(255, 255, 255), Point3f(0, 0, 0)), S:754


def gray(image):
    """cvtColor(image, gray, COLOR_BGR2GRAY) S:558, S:566 -> float32 (for CV_8UC3 the byte, exactly)"""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        b, g, r = (image[..., k].astype(np.int64) for k in range(3))
        return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(F)
    assert image.dtype == np.float32
    b, g, r = image[..., 0], image[..., 1], image[..., 2]
    return (b * F(0.114) + g * F(0.587)) + r * F(0.299)


def _reflect101(n):
    """source index of positions -1 .. n under BORDER_REFLECT_101"""
    i = np.abs(np.arange(-1, n + 1))
    i = np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)                  # n == 1


def sobel_xy(g):
    """Sobel(gray, gradx, CV_32F, 1, 0) and Sobel(gray, grady, CV_32F, 0, 1) S:562-563 of a float32 image, signed"""
    g = np.asarray(g, F)
    h, w = g.shape
    p = g[np.ix_(_reflect101(h), _reflect101(w))]                       # (h + 2) x (w + 2)
    left, mid, right = p[:, :-2], p[:, 1:-1], p[:, 2:]
    d = right - left
    s = (left + right) + (mid + mid)
    gradx = (d[:-2] + d[2:]) + (d[1:-1] + d[1:-1])
    grady = s[2:] - s[:-2]
    return gradx, grady


def gradients(image):
    """computeGradients S:549-572 for one image -> (gradx, grady), whole image, signed"""
    return sobel_xy(gray(image))


def _diff(img1, y1, x1, img2, y2, x2):
    """diffL2Square3<T> S:712-718 at index arrays"""
    if img1.dtype == np.uint8:
        d = img1[y1, x1].astype(np.int64) - img2[y2, x2].astype(np.int64)
        return (d * d).sum(-1).astype(F)
    d = img1[y1, x1] - img2[y2, x2]
    q = d * d
    return (q[:, 0] + q[:, 1]) + q[:, 2]


def compute_costs(image1, image2, tl1, tl2, union_tl, labels, label, roi, cost_func=COLOR, grads=None):
    """computeCosts S:733-803 -> costV (rh x (rw + 1)), costH ((rh + 1) x rw).  grads = ((gradx1, grady1), (gradx2, grady2)) of the whole
    images (computed here when None and the cost function asks for them).  A labels_ read outside the label image is "not this component"."""
    rx, ry, rw, rh = (int(v) for v in roi)
    dx1, dy1 = union_tl[0] - tl1[0], union_tl[1] - tl1[1]
    dx2, dy2 = union_tl[0] - tl2[0], union_tl[1] - tl2[1]
    uh, uw = labels.shape
    # is(y, x) = labels_(y, x) == l over [ry - 1, ry + rh] x [rx - 1, rx + rw], False outside the label image
    win = np.zeros((rh + 2, rw + 2), bool)
    y0, y1, x0, x1 = max(ry - 1, 0), min(ry + rh + 1, uh), max(rx - 1, 0), min(rx + rw + 1, uw)
    win[y0 - (ry - 1):y1 - (ry - 1), x0 - (rx - 1):x1 - (rx - 1)] = labels[y0:y1, x0:x1] == label
    if cost_func == COLOR_GRAD and grads is None:
        grads = (gradients(image1), gradients(image2))
    out = []
    for vertical in (True, False):
        if vertical:                                                     # S:756-777: x in [rx, rx + rw], the neighbour is (y, x - 1)
            here, there = win[1:-1, 1:], win[1:-1, :-1]
            ox, oy = 1, 0
        else:                                                            # S:780-802: y in [ry, ry + rh], the neighbour is (y - 1, x)
            here, there = win[1:, 1:-1], win[:-1, 1:-1]
            ox, oy = 0, 1
        cost = np.full(here.shape, BAD_REGION_COST, F)
        cy, cx = np.nonzero(here & there)
        y, x = cy + ry, cx + rx
        keep = (x > 0) if vertical else (y > 0)
        cy, cx, y, x = cy[keep], cx[keep], y[keep], x[keep]
        c = (_diff(image1, y + dy1 - oy, x + dx1 - ox, image2, y + dy2, x + dx2) + _diff(image1, y + dy1, x + dx1, image2, y + dy2 - oy, x + dx2 - ox)) / F(2)
        if cost_func == COLOR_GRAD:
            g1, g2 = grads[0][0 if vertical else 1], grads[1][0 if vertical else 1]
            cg = np.abs(g1[y + dy1, x + dx1]) + np.abs(g1[y + dy1 - oy, x + dx1 - ox])
            cg = cg + np.abs(g2[y + dy2, x + dx2])
            cg = cg + np.abs(g2[y + dy2 - oy, x + dx2 - ox])
            cg = cg + F(1)
            c = c / cg
        else:
            assert cost_func == COLOR
        cost[cy, cx] = c.astype(F)
        out.append(cost)
    return out[0], out[1]


def seam_estimate(image1, image2, tl1, tl2, union_tl, labels, label, roi, p1, p2, cost_func=COLOR, grads=None):
    """estimateSeam S:806-957 -> (seam (N, 2) int32 with p1 first; empty when p2 is not reachable, isHorizontal)"""
    costV, costH = compute_costs(image1, image2, tl1, tl2, union_tl, labels, label, roi, cost_func, grads)
    rx, ry, rw, rh = (int(v) for v in roi)
    src = (int(p1[0]) - rx, int(p1[1]) - ry)
    dst = (int(p2[0]) - rx, int(p2[1]) - ry)
    swapped = False
    horiz = abs(dst[0] - src[0]) > abs(dst[1] - src[1])                  # S:828
    if (src[0] > dst[0]) if horiz else (src[1] > dst[1]):               # S:830-842
        src, dst = dst, src
        swapped = True
    is_l = labels[ry:ry + rh, rx:rx + rw] == label
    control = np.zeros((rh, rw), np.uint8)
    if horiz:                                                            # the walk along x on the transposed problem
        is_l, control_w = is_l.T, control.T
        a, b = costH.T, costV.T                                          # a[s, i]: along the walk; b[s, i]: across it
        s0, i0, s1, i1 = src[0], src[1], dst[0], dst[1]
    else:
        control_w = control
        a, b = costV, costH
        s0, i0, s1, i1 = src[1], src[0], dst[1], dst[0]
    n = is_l.shape[1]
    cost = np.zeros(n, F)
    reach = np.zeros(n, bool)
    reach[i0] = True                                                     # S:850-851
    inf = F(np.inf)
    for s in range(s0 + 1, s1 + 1):                                      # S:859-885 / S:889-915
        # vertical: (1) cost(y-1, x) + costV(y-1, x); (2) cost(y-1, x-1) + costV(y-1, x-1) + costH(y, x-1); (3) cost(y-1, x+1) + costV(y-1, x+1) + costH(y, x)
        # horizontal: the same with x and y, costV and costH exchanged
        c1 = np.where(reach, cost + a[s - 1, :n], inf)
        c2 = np.full(n, inf, F)
        c2[1:] = np.where(reach[:-1], (cost[:-1] + a[s - 1, :n - 1]) + b[s, :n - 1], inf)
        c3 = np.full(n, inf, F)
        c3[:-1] = np.where(reach[1:], (cost[1:] + a[s - 1, 1:n]) + b[s, :n - 1], inf)
        cand = np.stack([c1, c2, c3])
        nsteps = np.stack([reach, np.r_[False, reach[:-1]], np.r_[reach[1:], False]]).any(0) & is_l[s]
        code = cand.argmin(0)                                            # min_element over pair<float, int>: the first minimum, S:879
        best = cand[code, np.arange(n)]
        assert np.isfinite(best[nsteps]).all()
        cost = np.where(nsteps, best, F(0)).astype(F)
        reach = nsteps
        control_w[s, nsteps] = (code + 1)[nsteps]
    if not reach[i1]:                                                    # S:918
        return np.zeros((0, 2), np.int32), horiz
    pts = []
    px, py = dst
    pts.append((px + rx, py + ry))
    if horiz:                                                            # S:930-947
        while px != src[0]:
            c = control[py, px]
            py += -1 if c == 2 else (1 if c == 3 else 0)
            px -= 1
            pts.append((px + rx, py + ry))
    else:
        while py != src[1]:
            c = control[py, px]
            px += -1 if c == 2 else (1 if c == 3 else 0)
            py -= 1
            pts.append((px + rx, py + ry))
    if not swapped:
        pts.reverse()
    assert pts[0] == (int(p1[0]), int(p1[1])) and pts[-1] == (int(p2[0]), int(p2[1]))   # S:953-954
    return np.array(pts, np.int32).reshape(-1, 2), horiz


class DpSeamFinder(dpseam_np.DpSeamFinder):
    """DpSeamFinder(costFunc) S:60-72: oracle/dpseam_np.py's finder with estimateSeam restated here for both cost functions; the gradient
    maps are those of the whole images, computed once per process call (S:398-399)."""

    def __init__(self, cost_func=COLOR):
        assert cost_func in (COLOR, COLOR_GRAD)
        self.cost_func = cost_func
        self.grads = None

    def process(self, image1, image2, tl1, tl2, mask1, mask2):
        self.grads = (gradients(image1), gradients(image2)) if self.cost_func == COLOR_GRAD else None
        super().process(image1, image2, tl1, tl2, mask1, mask2)

    def estimate_seam(self, image1, image2, tl1, tl2, comp, p1, p2):
        roi = (self.tls[comp][0], self.tls[comp][1], self.brs[comp][0] - self.tls[comp][0], self.brs[comp][1] - self.tls[comp][1])
        seam, horiz = seam_estimate(image1, image2, tl1, tl2, self.utl, self.labels, comp + 1, roi, p1, p2, self.cost_func, self.grads)
        return [tuple(int(v) for v in p) for p in seam], horiz
