"""The fisheye and stereographic projectors (ISX_WARP_FISHEYE, ISX_WARP_STEREOGRAPHIC) without a GPU: the host compilation of
csrc/proj_math.hpp against the NumPy model tests/helpers/polar_np.py bit for bit, the accuracy of the five restated functions, the closed
form mapBackward(mapForward(p)) = p, and the host-only entries isx_selftest_roi_host / isx_selftest_warp_point on every rig of the suite.
(The parent of the change that added the two kinds refuses them: every test here that calls the library fails there.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402

from imagestitch_amd import _lib  # noqa: E402

F = np.float32
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def run_math(entry, fn, a, b):
    out = np.full(a.shape, -7777.25, F)
    a = np.ascontiguousarray(a, F)
    b = np.ascontiguousarray(b, F) if b is not None else None
    _lib.check(getattr(_lib.load(), entry)(fn, a.size, _fp(a), _fp(b), _fp(out)))
    return out


def _model(fn, a, b):
    f = P.FUNCS[fn][1]
    return f(a, b) if b is not None else f(a)


@pytest.mark.parametrize("fn", sorted(PC.NAMES))
def test_host_math_equals_the_model_bit_for_bit(fn):
    a, b = PC.sweep(fn)
    got, want = run_math("isx_selftest_proj_math", fn, a, b), _model(fn, a, b)
    bad = np.flatnonzero(~((got.view(np.uint32) == np.asarray(want, F).view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (PC.NAMES[fn], a[bad[:4]], None if b is None else b[bad[:4]], got[bad[:4]], want[bad[:4]])


def test_the_rules_for_special_values():
    inf, nan = F(np.inf), F(np.nan)
    pi, h = P.PI_F, F(np.pi / 2)
    y = np.array([0.0, -0.0, 0.0, -0.0, 1, -1, inf, inf, -inf, 1, 1, nan, 1], F)
    x = np.array([0.0, 0.0, -0.0, -0.0, 0, 0, inf, -inf, -inf, inf, -inf, 1, nan], F)
    want = np.array([0.0, -0.0, pi, -pi, h, -h, F(np.pi / 4), F(3 * np.pi / 4), F(-3 * np.pi / 4), 0.0, pi, nan, nan], F)
    assert PC.same_bits(run_math("isx_selftest_proj_math", PC.ATAN2, y, x), want)
    assert PC.same_bits(run_math("isx_selftest_proj_math", PC.ATAN, np.array([inf, -inf, 0.0, -0.0, nan], F), None), np.array([h, -h, 0.0, -0.0, nan], F))
    assert PC.same_bits(run_math("isx_selftest_proj_math", PC.ACOS, np.array([1, -1, np.nextafter(F(1), F(2)), -2, nan, inf], F), None),
                        np.array([0.0, pi, nan, nan, nan, nan], F))
    big = np.array([2.0 ** 28, -2.0 ** 28, np.nextafter(F(2.0 ** 28), inf), inf, -inf, nan], F)
    for fn in (PC.SIN, PC.COS):
        got = run_math("isx_selftest_proj_math", fn, big, None)
        assert np.isfinite(got[:2]).all() and np.isnan(got[2:]).all()
    assert PC.same_bits(run_math("isx_selftest_proj_math", PC.COS, np.array([0.0, -0.0], F), None), np.array([1, 1], F))
    assert (run_math("isx_selftest_proj_math", PC.SIN, np.array([0.0, -0.0], F), None) == 0).all()


def test_math_entry_checks_its_arguments():
    lib = _lib.load()
    a = np.zeros(4, F)
    assert lib.isx_selftest_proj_math(5, 4, _fp(a), None, _fp(a)) == 1 and lib.isx_selftest_proj_math(-1, 4, _fp(a), None, _fp(a)) == 1
    assert lib.isx_selftest_proj_math(PC.ATAN2, 4, _fp(a), None, _fp(a)) == 1            # atan2f without its second operand
    assert lib.isx_selftest_proj_math(0, 4, None, None, _fp(a)) == 1 and lib.isx_selftest_proj_math(0, 0, None, None, None) == 0


# The restated functions are deterministic, so the maxima over the fixed sweep are asserted exactly (DESIGN.md §8 tabulates them): distance
# in float32 steps from NumPy's float64 function rounded to float32.  Measured, not chosen.
MAX_ULP = {PC.SIN: 1, PC.COS: 1, PC.ATAN2: 0, PC.ATAN: 0, PC.ACOS: 0}
_REF = {PC.SIN: np.sin, PC.COS: np.cos, PC.ATAN: np.arctan, PC.ACOS: np.arccos}


@pytest.mark.parametrize("fn", sorted(PC.NAMES))
def test_accuracy_is_the_measured_one(fn):
    a, b = PC.accuracy_sweep(fn)
    got = run_math("isx_selftest_proj_math", fn, a, b)
    ref = np.arctan2(a.astype(np.float64), b.astype(np.float64)) if fn == PC.ATAN2 else _REF[fn](a.astype(np.float64))
    d = PC.ulp_distance(got, ref)
    print("max ulp distance of", PC.NAMES[fn], "=", d)
    assert d == MAX_ULP[fn], (PC.NAMES[fn], d)


RIGS = [(s, r) for s in P.SIZES for r in P.ROTATIONS]


def _ids(v):
    return "%dx%d" % v[:2] if isinstance(v, tuple) else str(v)


def _f64_round_trip(kind, scale, r_kinv, k_rinv, x, y):
    """mapBackward(mapForward(x, y)) by the same formulas in float64 with NumPy's functions -> (x', y', z of the forward transform)"""
    r, k, s = r_kinv.astype(np.float64), k_rinv.astype(np.float64), float(scale)
    with np.errstate(all="ignore"):
        x_, y_, z_ = r[0] * x + r[1] * y + r[2], r[3] * x + r[4] * y + r[5], r[6] * x + r[7] * y + r[8]
        u_ = np.arctan2(x_, z_)
        v_ = np.pi - np.arccos(y_ / np.sqrt(x_ * x_ + y_ * y_ + z_ * z_))
        rr = v_ if kind == P.FISHEYE else np.sin(v_) / (1 - np.cos(v_))
        u, v = s * rr * np.cos(u_), s * rr * np.sin(u_)
        u, v = u / s, v / s
        a = np.arctan2(v, u)
        rad = np.sqrt(u * u + v * v)
        vb = rad if kind == P.FISHEYE else 2 * np.arctan(1 / rad)
        sinv = np.sin(np.pi - vb)
        bx, by, bz = sinv * np.sin(a), np.cos(np.pi - vb), sinv * np.cos(a)
        X, Y, Z = k[0] * bx + k[1] * by + k[2] * bz, k[3] * bx + k[4] * by + k[5] * bz, k[6] * bx + k[7] * by + k[8] * bz
        return X / Z, Y / Z, z_


# mapBackward(mapForward(p)) against p, in source pixels, over the source pixels in front of the camera (z > 0 in the forward transform, no
# (-1, -1) sentinel).  Origin of the bound: the float32 model against the float64 evaluation of the same formulas with the same float32
# matrices (_f64_round_trip, which itself returns p to 2.5e-5 px: r_kinv and k_rinv are rounded, not exact inverses).  The worst case over the
# 36 rigs with such pixels is 2.304e-4 px (stereographic, 64 x 48, pitch +pi/3); the bound is twice that.  The model's own distance from p is
# 2.31e-4 px at worst.
ROUND_TRIP_WORST = 2.304e-4
ROUND_TRIP_TOL = 2 * ROUND_TRIP_WORST


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size,rname", RIGS, ids=_ids)
def test_backward_of_forward_returns_to_the_pixel(kind, size, rname):
    w, h, f, K, R = P.rig(size, rname)
    m = P.from_rig(kind, f, K, R)
    xs, ys = np.meshgrid(np.arange(w).astype(F), np.arange(h).astype(F))
    u, v = m.map_forward(xs, ys)
    bx, by = m.map_backward(u, v)
    rx, ry, z = _f64_round_trip(kind, f, m.r_kinv, m.k_rinv, xs.astype(np.float64), ys.astype(np.float64))
    ok = (z > 0) & np.isfinite(u) & np.isfinite(v) & ~((bx == -1) & (by == -1))
    assert ok.any() == (rname != "yaw2.97")          # (yaw 2.97 looks backwards: z <= 0 everywhere)
    if not ok.any():
        return
    err = max(np.abs(bx - xs)[ok].max(), np.abs(by - ys)[ok].max())
    vs64 = max(np.abs(bx - rx)[ok].max(), np.abs(by - ry)[ok].max())
    print("round trip", kind, size, rname, "from p", err, "from the float64 evaluation", vs64, "px over", int(ok.sum()), "pixels")
    assert err <= ROUND_TRIP_TOL and vs64 <= ROUND_TRIP_TOL, (err, vs64)


def _roi_host(kind, f, K, R, w, h):
    Kp, Rp = _lib.f9(K), _lib.f9(R)
    roi, mm = (C.c_int * 4)(), (C.c_float * 4)()
    _lib.check(_lib.load().isx_selftest_roi_host(kind, float(f), Kp[1], Rp[1], w, h, 0, roi, mm))
    return tuple(roi), np.array(list(mm), F)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size,rname", RIGS, ids=_ids)
def test_roi_host_and_warp_point_equal_the_model(kind, size, rname):
    w, h, f, K, R = P.rig(size, rname)
    m = P.from_rig(kind, f, K, R)
    roi, mm = _roi_host(kind, f, K, R, w, h)
    mroi, mmm = m.detect_roi(w, h)
    assert roi == tuple(int(v) for v in mroi) and np.array_equal(mm, mmm), (roi, mroi, mm, mmm)
    lib = _lib.load()
    Kp, Rp = _lib.f9(K), _lib.f9(R)
    rng = np.random.default_rng(w)
    pts = [(0, 0), (w - 1, h - 1), (w / 2, h / 2)] + [tuple(p) for p in rng.uniform(-5, max(w, h) + 5, (24, 2))]
    for x, y in pts:
        uv = (C.c_float * 2)()
        _lib.check(lib.isx_selftest_warp_point(kind, float(f), Kp[1], Rp[1], None, F(x), F(y), uv))
        mu, mv = m.map_forward(F(x), F(y))
        assert PC.same_bits(np.array([uv[0], uv[1]], F), np.array([mu, mv], F)), (x, y, uv[0], uv[1], mu, mv)


def test_the_issue_table_at_64x48():
    """The ROIs the rigs were chosen for: the poles inside the destination, the blown-up stereographic rig with its NaN pixel."""
    want = {("identity", P.FISHEYE): (35, -49, 83, 48), ("identity", P.STEREOGRAPHIC): (20, -39, 70, 38),
            ("pitch+pi/2", P.FISHEYE): (-21, -26, 20, 26), ("pitch+pi/2", P.STEREOGRAPHIC): (-3200, -3200, 3200, 3200),
            ("pitch-pi/2", P.STEREOGRAPHIC): (-10, -14, 11, 13)}
    for (rname, kind), roi in want.items():
        w, h, f, K, R = P.rig(P.SIZES[1], rname)
        assert _roi_host(kind, f, K, R, w, h)[0] == roi, (rname, kind)
    w, h, f, K, R = P.rig(P.SIZES[1], "pitch-pi/2")                   # the antipole: the disc of radius pi * scale
    roi = _roi_host(P.FISHEYE, f, K, R, w, h)[0]
    assert max(abs(v) for v in roi) in (int(np.pi * f), int(np.pi * f) - 1), roi
    m = P.from_rig(P.STEREOGRAPHIC, *P.rig(P.SIZES[1], "pitch+pi/2")[2:])
    xs, ys = np.meshgrid(np.arange(w).astype(F), np.arange(h).astype(F))
    assert int(np.isnan(m.map_forward(xs, ys)[0]).sum()) == 1          # the 0 / 0 pixel that min / max must ignore


def test_roi_just_under_the_limit_at_261x67():
    """The blown-up stereographic ROI at 261 x 67: 32 394 a side, under the 32 767 of cv::remap's short coordinates."""
    w, h, f, K, R = P.rig(P.SIZES[2], "pitch+pi/2")
    roi, _ = _roi_host(P.STEREOGRAPHIC, f, K, R, w, h)
    assert roi == tuple(int(v) for v in P.from_rig(P.STEREOGRAPHIC, f, K, R).detect_roi(w, h)[0])
    assert roi[2] - roi[0] == 32394 and roi[3] - roi[1] == 32394, roi


def test_a_translation_is_refused_and_the_kinds_are_exported():
    lib = _lib.load()
    K, R = _lib.f9(np.eye(3)), _lib.f9(np.eye(3))
    uv = (C.c_float * 2)()
    for kind in KINDS:
        t = (C.c_float * 3)(0.1, 0, 0)
        assert lib.isx_selftest_warp_point(kind, 10.0, K[1], R[1], t, 1.0, 1.0, uv) == 6             # ISX_ERR_UNSUPPORTED
        assert lib.isx_selftest_warp_point(kind, 10.0, K[1], R[1], (C.c_float * 3)(0, 0, 0), 1.0, 1.0, uv) == 0
    assert lib.isx_selftest_warp_point(5, 10.0, K[1], R[1], None, 1.0, 1.0, uv) == 1
    import imagestitch_amd as I
    from imagestitch_amd import warper
    assert (I.WARP_FISHEYE, I.WARP_STEREOGRAPHIC) == (3, 4) and I.FisheyeWarper.kind == 3 and I.StereographicWarper.kind == 4
    assert warper.CREATORS["fisheye"] is I.FisheyeWarper and warper.CREATORS["stereographic"] is I.StereographicWarper
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "..", "include", "imagestitch_hip.h")).read()
    assert "ISX_WARP_FISHEYE = 3" in src and "ISX_WARP_STEREOGRAPHIC = 4" in src
