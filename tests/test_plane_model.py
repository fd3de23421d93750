"""The plane projector (cv::detail::PlaneWarper, with translation): closed forms for the NumPy model tests/helpers/plane_np.py - the
specification isx_warper_create(ISX_WARP_PLANE) is held to bit for bit on the GPU - and the parts of the library that need no device:
the four-corner ROI (isx_selftest_roi_host) against the model on random rigs, and warpPoint against the model / the oracle's mapForward.

isx_warper_warp_point takes a warper handle, and a handle cannot be created without a device (tests/test_abi_and_host.py pins that): the
comparison here goes through isx_selftest_warp_point, the same host functions without a handle; tests/test_gpu_plane_warp.py repeats it
through the handle's entry."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import plane_np as P  # noqa: E402

from imagestitch_amd import _lib, synth  # noqa: E402

PLANE = 2
F = np.float32


def _rot(yaw, pitch, roll):
    return (synth._rot("y", yaw) @ synth._rot("x", pitch) @ synth._rot("z", roll)).astype(np.float32)


def _K(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float32)


def _src(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_identity_rig_is_the_identity(oracle):
    """scale = f = 1024 (a power of two), integral cx / cy, R = I, T = 0: every operation of the model is exact."""
    w, h, cx, cy = 37, 23, 17, 9
    p = P.from_rig(oracle, 1024.0, _K(1024.0, cx, cy), np.eye(3, dtype=np.float32))
    roi, mm = p.detect_roi(w, h)
    assert tuple(roi) == (-cx, -cy, w - 1 - cx, h - 1 - cy)
    assert np.array_equal(mm, np.array([-cx, -cy, w - 1 - cx, h - 1 - cy], F))
    xm, ym = p.build_maps(roi)
    assert xm.shape == (h, w) and xm.dtype == np.float32
    u = np.arange(roi[0], roi[2] + 1, dtype=np.float32)[None, :]
    v = np.arange(roi[1], roi[3] + 1, dtype=np.float32)[:, None]
    assert np.array_equal(xm, np.broadcast_to(u + cx, (h, w))) and np.array_equal(ym, np.broadcast_to(v + cy, (h, w)))
    src = _src(h, w)
    corner, dst, _ = p.warp(src, oracle.LINEAR, oracle.BORDER_REFLECT)
    assert corner == (-cx, -cy) and np.array_equal(dst, src)
    msk = np.random.default_rng(1).integers(0, 2, (h, w), dtype=np.uint8) * 255
    _, dm, _ = p.warp(msk, oracle.NEAREST, oracle.BORDER_CONSTANT)
    assert np.array_equal(dm, msk)


def test_translation_moves_the_roi_and_not_the_pixels(oracle):
    w, h, cx, cy = 41, 29, 20, 14
    K, R = _K(1024.0, cx, cy), np.eye(3, dtype=np.float32)
    p0 = P.from_rig(oracle, 1024.0, K, R)
    roi0, _ = p0.detect_roi(w, h)
    src = _src(h, w, 3)
    _, d0, _ = p0.warp(src, oracle.LINEAR, oracle.BORDER_REFLECT)
    # scale * a = 256, scale * b = -128: integral, the ROI moves by exactly that and the pixels stay
    p1 = P.from_rig(oracle, 1024.0, K, R, (0.25, -0.125, 0.0))
    roi1, _ = p1.detect_roi(w, h)
    assert tuple(roi1) == (roi0[0] + 256, roi0[1] - 128, roi0[2] + 256, roi0[3] - 128)
    c1, d1, _ = p1.warp(src, oracle.LINEAR, oracle.BORDER_REFLECT)
    assert c1 == (roi0[0] + 256, roi0[1] - 128) and np.array_equal(d1, d0)
    # a fractional shift: every bound is the truncation (toward zero) of the shifted extremum.  1024 * 0.2998046875 = 307 exactly, so the
    # translation below shifts u by 307.5 and v by -100.25
    p2 = P.from_rig(oracle, 1024.0, K, R, (307.5 / 1024.0, -100.25 / 1024.0, 0.0))
    roi2, mm2 = p2.detect_roi(w, h)
    want = np.array([-cx + 307.5, -cy - 100.25, w - 1 - cx + 307.5, h - 1 - cy - 100.25])
    assert np.array_equal(mm2.astype(np.float64), want)
    assert tuple(roi2) == tuple(int(np.trunc(x)) for x in want)


def test_the_roi_truncates_toward_zero(oracle):
    """cx = 100.5 puts the minimum at u = -100.5: static_cast<int> gives -100 (floor would give -101); the maximum 99.5 gives 99."""
    p = P.from_rig(oracle, 1024.0, _K(1024.0, 100.5, 50.25), np.eye(3, dtype=np.float32))
    roi, mm = p.detect_roi(201, 101)
    assert np.array_equal(mm, np.array([-100.5, -50.25, 99.5, 49.75], F))
    assert tuple(roi) == (-100, -50, 99, 49)
    assert P.f2i(F(-0.75)) == 0 and P.f2i(F("nan")) == P.INT_MIN and P.f2i(F(3e9)) == P.INT_MIN


def test_backward_of_forward_is_the_point(oracle):
    rng = np.random.default_rng(5)
    for _ in range(50):
        w, h = int(rng.integers(40, 2000)), int(rng.integers(40, 1500))
        f = float(rng.uniform(0.8, 2.0) * max(w, h))
        K = _K(f, w / 2 + rng.uniform(-10, 10), h / 2 + rng.uniform(-10, 10))
        R = _rot(*rng.uniform(-0.5, 0.5, 3))
        T = rng.uniform(-0.2, 0.2, 3) if rng.integers(0, 2) else None
        p = P.from_rig(oracle, float(f * rng.uniform(0.7, 1.4)), K, R, T)
        x, y = rng.uniform(0, w - 1, 64).astype(F), rng.uniform(0, h - 1, 64).astype(F)
        u, v = p.map_forward(x, y)
        bx, by = p.map_backward(u, v)
        assert np.allclose(bx, x, atol=2e-2) and np.allclose(by, y, atol=2e-2), (np.abs(bx - x).max(), np.abs(by - y).max())


def test_a_corner_behind_the_camera_has_no_sentinel(oracle):
    """A bounding box that reaches z <= 0: the model divides all the same (a cylindrical / spherical map holds (-1, -1) there, W:61), and the
    warped pixel is what cv::remap makes of the quotient's bits."""
    w, h = 64, 48
    K = _K(60.0, 32.0, 24.0)
    p = P.from_rig(oracle, 60.0, K, _rot(0.5, 0.1, 0.0))
    roi = np.array([-400, -60, 40, 60])          # tan(yaw + atan(u / scale)) has its pole inside: columns left of it have z < 0
    xm, ym = p.build_maps(roi)
    k = p.k_rinv
    u, v = F(roi[0]) / F(60.0), F(roi[1]) / F(60.0)
    x = k[0] * u + k[1] * v + k[2] * F(1)
    y = k[3] * u + k[4] * v + k[5] * F(1)
    z = k[6] * u + k[7] * v + k[8] * F(1)
    assert z < 0
    assert xm[0, 0] == x / z and ym[0, 0] == y / z and (xm[0, 0], ym[0, 0]) != (-1.0, -1.0)
    assert (xm == -1).sum() == 0
    src = _src(h, w, 9)
    _, dst, _ = p.warp(src, oracle.LINEAR, oracle.BORDER_REFLECT, roi)
    assert np.array_equal(dst, oracle.remap(src, xm, ym, oracle.LINEAR, oracle.BORDER_REFLECT))
    # ... and a pixel whose z is exactly 0 divides by it: (+-inf or NaN) goes into cv::remap as it is
    p.set_camera(p.r_kinv, np.array([1, 0, 0, 0, 1, 0, 1, 0, 0], F))
    bx, by = p.map_backward(F(0), F(60.0))
    assert np.isnan(bx) and np.isinf(by)


def _roi_host(lib, scale, K, R, w, h):
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    R = np.ascontiguousarray(R, np.float32).reshape(9)
    roi = np.zeros(4, np.int32)
    mm = np.zeros(4, np.float32)
    fp = C.POINTER(C.c_float)
    rc = lib.isx_selftest_roi_host(PLANE, C.c_float(scale), K.ctypes.data_as(fp), R.ctypes.data_as(fp), w, h, 0,
                                   roi.ctypes.data_as(C.POINTER(C.c_int)), mm.ctypes.data_as(fp))
    return rc, roi, mm


def test_the_library_roi_is_the_four_corner_rule(oracle):
    """isx_selftest_roi_host(ISX_WARP_PLANE): what isx_warper_roi returns for a plane handle (T = 0), without a device - ROI and float
    extrema equal the model's on 200 random rigs."""
    lib = _lib.load()
    rng = np.random.default_rng(20261017)
    for i in range(200):
        w, h = int(rng.integers(3, 4200)), int(rng.integers(3, 2400))
        f = float(rng.uniform(0.4, 3.0) * max(w, h))
        K = np.array([[f, 0, w / 2 + rng.uniform(-20, 20)], [0, f * rng.uniform(0.9, 1.1), h / 2 + rng.uniform(-20, 20)], [0, 0, 1]], np.float32)
        R = _rot(*rng.uniform(-0.5, 0.5, 3))
        scale = float(f * rng.uniform(0.5, 2.0))
        rc, roi, mm = _roi_host(lib, scale, K, R, w, h)
        assert rc == 0, lib.isx_last_error()
        mroi, mmm = P.from_rig(oracle, scale, K, R).detect_roi(w, h)
        assert np.array_equal(roi, mroi), (i, roi, mroi)
        assert np.array_equal(mm, mmm), (i, mm, mmm)
    assert _lib.WARP_PLANE == PLANE


def _warp_point(lib, kind, scale, K, R, T, x, y):
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    R = np.ascontiguousarray(R, np.float32).reshape(9)
    fp = C.POINTER(C.c_float)
    t = None if T is None else np.ascontiguousarray(T, np.float32).reshape(3)
    uv = np.zeros(2, np.float32)
    rc = lib.isx_selftest_warp_point(kind, C.c_float(scale), K.ctypes.data_as(fp), R.ctypes.data_as(fp), None if t is None else t.ctypes.data_as(fp),
                                     C.c_float(x), C.c_float(y), uv.ctypes.data_as(fp))
    return rc, uv[0], uv[1]


def test_warp_point_is_map_forward(oracle):
    """The host code behind isx_warper_warp_point: the model for the plane kind (T zero and non-zero), the oracle's mapForward for the
    cylindrical and the spherical kind, bit for bit."""
    lib = _lib.load()
    rng = np.random.default_rng(31)
    for _ in range(40):
        w, h = int(rng.integers(40, 4000)), int(rng.integers(40, 2200))
        f = float(rng.uniform(0.8, 2.0) * max(w, h))
        K = _K(f, w / 2 + rng.uniform(-10, 10), h / 2 + rng.uniform(-10, 10))
        R = _rot(*rng.uniform(-0.5, 0.5, 3))
        scale = float(f * rng.uniform(0.7, 1.4))
        T = rng.uniform(-0.3, 0.3, 3).astype(F)
        pts = [(0.0, 0.0), (w - 1.0, h - 1.0)] + [(float(rng.uniform(0, w)), float(rng.uniform(0, h))) for _ in range(6)]
        _, _, r_kinv, k_rinv = oracle.camera(K, R)
        for Tm in (None, T):
            m = P.Plane(scale).set_camera(r_kinv, k_rinv, Tm)
            for x, y in pts:
                rc, u, v = _warp_point(lib, PLANE, scale, K, R, Tm, x, y)
                mu, mv = m.map_forward(F(x), F(y))
                assert rc == 0 and u == mu and v == mv, (x, y, u, mu, v, mv)
        for kind in (oracle.CYL, oracle.SPH):
            for x, y in pts:
                rc, u, v = _warp_point(lib, kind, scale, K, R, None, x, y)
                ou, ov = oracle.map_forward(kind, scale, r_kinv, F(x), F(y))
                assert rc == 0 and u == ou and v == ov, (kind, x, y, u, ou, v, ov)
            assert _warp_point(lib, kind, scale, K, R, T, 1.0, 1.0)[0] == 6      # ISX_ERR_UNSUPPORTED: no translation on these kinds
