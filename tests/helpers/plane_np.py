"""cv::detail::PlaneWarper (OpenCV 3.4.x warpers_inl.hpp / warpers.cpp, PlaneProjector) restated in NumPy float32.

TEST INFRASTRUCTURE ONLY.  Every operation is its own rounded float32 operation, evaluated left to right as the C++ is written, with no
fused multiply-add.  The source is in neither tree, so the parity of this model with OpenCV is unpinned (like the spherical projector,
SURVEY §8(a)); what the GPU is held to is THIS restatement, bit for bit.

    p = Plane(scale); p.set_camera(r_kinv, k_rinv, T)      # r_kinv, k_rinv from oracle.camera(K, R)
    u, v = p.map_forward(x, y);  x, y = p.map_backward(u, v)
    roi, mm = p.detect_roi(w, h);  xmap, ymap = p.build_maps(roi);  corner, dst, roi = p.warp(src, interp, border)
"""
import numpy as np

F = np.float32
_FLT_MAX = np.finfo(np.float32).max
INT_MIN = -2147483648


def f2i(v):
    """static_cast<int>(float) as x86 does it (cvttss2si): truncation toward zero; NaN and out-of-range give INT_MIN."""
    v = float(v)
    return int(v) if abs(v) < 2147483648.0 else INT_MIN


class Plane:
    def __init__(self, scale):
        self.scale = F(scale)
        self.r_kinv = np.zeros(9, F)
        self.k_rinv = np.zeros(9, F)
        self.t = np.zeros(3, F)

    def set_camera(self, r_kinv, k_rinv, T=None):
        """setCameraParams(K, R, T): r_kinv = R K^-1, k_rinv = K R^T as oracle.camera computes them; t = T (zeros without one)."""
        self.r_kinv = np.asarray(r_kinv, F).reshape(9).copy()
        self.k_rinv = np.asarray(k_rinv, F).reshape(9).copy()
        self.t = np.zeros(3, F) if T is None else np.asarray(T, F).reshape(3).copy()
        return self

    def map_forward(self, x, y):
        r, t = self.r_kinv, self.t
        x, y = np.asarray(x, F), np.asarray(y, F)
        with np.errstate(all="ignore"):
            x_ = r[0] * x + r[1] * y + r[2]
            y_ = r[3] * x + r[4] * y + r[5]
            z_ = r[6] * x + r[7] * y + r[8]
            tz = F(1) - t[2]
            x_ = t[0] + x_ / z_ * tz
            y_ = t[1] + y_ / z_ * tz
            return self.scale * x_, self.scale * y_

    def map_backward(self, u, v):
        k, t = self.k_rinv, self.t
        u, v = np.asarray(u, F), np.asarray(v, F)
        with np.errstate(all="ignore"):
            u = u / self.scale - t[0]
            v = v / self.scale - t[1]
            tz = F(1) - t[2]
            x = k[0] * u + k[1] * v + k[2] * tz
            y = k[3] * u + k[4] * v + k[5] * tz
            z = k[6] * u + k[7] * v + k[8] * tz
            return x / z, y / z          # no z > 0 test, no (-1, -1) sentinel

    def detect_roi(self, w, h):
        """mapForward of the four source corners, min / max ((std::min)(tl, u): a NaN never wins), static_cast<int>."""
        tl_u = tl_v = F(_FLT_MAX)
        br_u = br_v = F(-_FLT_MAX)
        for x in (0, w - 1):
            for y in (0, h - 1):
                u, v = self.map_forward(F(x), F(y))
                tl_u = u if u < tl_u else tl_u
                tl_v = v if v < tl_v else tl_v
                br_u = u if br_u < u else br_u
                br_v = v if br_v < v else br_v
        mm = np.array([tl_u, tl_v, br_u, br_v], F)
        return np.array([f2i(m) for m in mm], np.int64), mm

    def build_maps(self, roi):
        """The base class's buildMaps over (tl.x, tl.y, br.x, br.y): maps of (br - tl + 1) a side (W:128-141)."""
        u = np.arange(int(roi[0]), int(roi[2]) + 1, dtype=np.int64).astype(F)[None, :]
        v = np.arange(int(roi[1]), int(roi[3]) + 1, dtype=np.int64).astype(F)[:, None]
        x, y = self.map_backward(u, v)
        return np.ascontiguousarray(np.broadcast_to(x, (v.shape[0], u.shape[1])), F), np.ascontiguousarray(np.broadcast_to(y, (v.shape[0], u.shape[1])), F)

    def warp(self, src, interp, border, roi=None):
        """RotationWarper::warp (W:145-161): oracle.remap of this model's own maps -> (corner, dst, roi)."""
        from oracle import capi as O
        if roi is None:
            roi, _ = self.detect_roi(src.shape[1], src.shape[0])
        xm, ym = self.build_maps(roi)
        return (int(roi[0]), int(roi[1])), O.remap(src, xm, ym, interp, border), roi


def from_rig(oracle, scale, K, R, T=None):
    """A Plane with the camera of (K, R[, T]) as the oracle's setCameraParams computes it."""
    _, _, r_kinv, k_rinv = oracle.camera(K, R)
    return Plane(scale).set_camera(r_kinv, k_rinv, T)
