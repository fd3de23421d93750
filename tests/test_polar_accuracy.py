"""What DESIGN.md claims about the accuracy of the fisheye and stereographic maps, held against mpmath (no GPU; tests/test_polar_model.py
measures sinf / cosf on [-2 pi, 2 pi] against NumPy's float64 and mapBackward only as mapBackward(mapForward(p)) inside the image):

- sinf / cosf over the whole range they serve, |x| <= 2^28, and at the floats nearest to the multiples of pi / 2 (where the reduction cancels),
  in float32 steps from the CORRECTLY ROUNDED value (mpmath at 200 bits, rounded once to 24 bits);
- mapBackward over the whole window of every named rig and both kinds against the same formulas in float64 (NumPy, itself spot-checked
  against mpmath): the (-1, -1) sentinel set, and the distance in source pixels where the ray is safely in front of the camera."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402
from test_polar_model import run_math  # noqa: E402

F, D = np.float32, np.float64
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]
PREC = 200          # bits: 2^28 has 29 of them before the point, the result keeps 170 after the cancellation of the reduction


def _order(v):
    i = np.asarray(v, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _round32(x):
    """an mpf rounded ONCE to float32's 24 bits (the values here are far from float32's subnormals)"""
    with mp.workprec(24):
        return float(+x)


def wide_sweeps():
    """'log': 12 000 floats, log-uniform in magnitude over [1e-6, 2^28], either sign.  'near': for 2 000 multiples k pi / 2 - every k up to
    600 and a log-uniform draw up to 2^28 / (pi / 2) - the nearest float32 and its two neighbours, either sign."""
    rng = np.random.default_rng(4242)
    log = (rng.choice([-1, 1], 12000) * np.exp(rng.uniform(np.log(1e-6), np.log(2.0 ** 28), 12000))).astype(F)
    ks = np.unique(np.concatenate([np.arange(1, 601), np.round(np.exp(rng.uniform(np.log(600), np.log(2.0 ** 28 / (np.pi / 2)), 1400))).astype(np.int64)]))
    with mp.workprec(PREC):
        near = np.array([float(mp.mpf(int(k)) * mp.pi / 2) for k in ks]).astype(F)
    near = np.concatenate([near, np.nextafter(near, F(np.inf)), np.nextafter(near, F(-np.inf))])
    near = np.concatenate([near, -near])
    return {"log": log, "near": near[np.abs(near) <= P.TRIG_MAX]}


# Measured, not chosen: the functions are deterministic, so the maxima over the fixed sweeps are asserted exactly (DESIGN.md §8 tabulates
# them beside tests/test_polar_model.py's MAX_ULP).  float32 steps from the correctly rounded value.
WIDE_MAX_ULP = {("log", PC.SIN): 0, ("log", PC.COS): 1, ("near", PC.SIN): 0, ("near", PC.COS): 0}


@pytest.mark.parametrize("fn", [PC.SIN, PC.COS])
@pytest.mark.parametrize("which", ["log", "near"])
def test_sinf_cosf_over_the_whole_served_range(which, fn):
    x = wide_sweeps()[which]
    assert x.size > 11000 and np.abs(x).max() > 2.0 ** 27 and (np.abs(x) <= P.TRIG_MAX).all()
    got = run_math("isx_selftest_proj_math", fn, x, None)
    assert PC.same_bits(got, P.FUNCS[fn][1](x))
    f = mp.sin if fn == PC.SIN else mp.cos
    with mp.workprec(PREC):
        ref = np.array([_round32(f(mp.mpf(float(v)))) for v in x], F)
    d = np.abs(_order(got) - _order(ref))
    print("max ulp distance of", PC.NAMES[fn], "on the", which, "sweep =", int(d.max()), "at", x[int(np.argmax(d))], "-", int((d > 0).sum()), "of", x.size, "differ")
    assert int(d.max()) == WIDE_MAX_ULP[(which, fn)], (which, PC.NAMES[fn], int(d.max()))


# ---- mapBackward over whole windows -----------------------------------------------------------------------------------------------------------
def backward_f64(m, u, v):
    """mapBackward up to its division by the same formulas in float64 with NumPy's functions: the same float32 matrix, scale and
    static_cast<float>(CV_PI), widened exactly -> (x, y, z)"""
    k, s = m.k_rinv.astype(D), D(m.scale)
    u, v = np.broadcast_arrays(np.asarray(u, D), np.asarray(v, D))
    with np.errstate(all="ignore"):
        u, v = u / s, v / s
        u_ = np.arctan2(v, u)
        r = np.sqrt(u * u + v * v)
        a = D(P.PI_F) - (r if m.kind == P.FISHEYE else 2 * np.arctan(1 / r))
        sinv, cosv = np.sin(a), np.cos(a)
        x_, y_, z_ = sinv * np.sin(u_), cosv, sinv * np.cos(u_)
        return k[0] * x_ + k[1] * y_ + k[2] * z_, k[3] * x_ + k[4] * y_ + k[5] * z_, k[6] * x_ + k[7] * y_ + k[8] * z_


def backward_mp(m, u, v):
    """the same for one destination pixel in mpmath -> (x, y, z) as mpf"""
    with mp.workprec(PREC):
        k, s = [mp.mpf(float(t)) for t in m.k_rinv], mp.mpf(float(m.scale))
        u, v = mp.mpf(int(u)) / s, mp.mpf(int(v)) / s
        u_ = mp.atan2(v, u)
        r = mp.sqrt(u * u + v * v)
        if m.kind == P.FISHEYE:
            vb = r
        else:
            vb = 2 * mp.atan(1 / r) if r != 0 else mp.pi          # atanf(1.f / 0) = atanf(inf) = pi / 2
        a = mp.mpf(float(P.PI_F)) - vb
        x_, y_, z_ = mp.sin(a) * mp.sin(u_), mp.cos(a), mp.sin(a) * mp.cos(u_)
        return k[0] * x_ + k[1] * y_ + k[2] * z_, k[3] * x_ + k[4] * y_ + k[5] * z_, k[6] * x_ + k[7] * y_ + k[8] * z_


# z is the cosine of the angle between the ray and the optical axis (K's third row is (0, 0, 1), so k_rinv's is R^T's), and the source pixel
# is (x / z, y / z): its error grows as 1 / z^2 and has no bound towards the horizon.  All figures below are measured over the 42 windows
# (21 named rigs, both kinds), the float32 model against backward_f64; bounds are twice the worst case, as ROUND_TRIP_TOL is.
#  - z itself: the float32 z is within Z_WORST of the float64 one.  Where |z| in float64 exceeds Z_MARGIN the two evaluations must agree on
#    the sign of z, i.e. on the (-1, -1) sentinel, pixel for pixel.
#  - "safely in front": z > Z_SAFE = 1 / 8, rays within 82.8 degrees of the axis.  There the model is within BACKWARD_WORST source pixels of
#    the float64 evaluation (fisheye, 261 x 67, pitch -pi/3, at z just above 1 / 8; 2.3e-4 px for z > 1 / 4).
#  - excluded from the distance (not from the sentinel check): pixels with |z| <= Z_MARGIN (none on these rigs) and grazing rays 0 < z <=
#    Z_SAFE - at most EXCLUDED_WORST of a window (stereographic, 64 x 48, pitch +pi/2: 1472 of 12288), capped at EXCLUDED_CAP.
Z_WORST = 3.8802e-7
Z_MARGIN = 2 * Z_WORST
Z_SAFE = 0.125
BACKWARD_WORST = 7.591e-4
BACKWARD_TOL = 2 * BACKWARD_WORST
EXCLUDED_WORST = 0.1198
EXCLUDED_CAP = 0.15
F64_VS_MP_TOL = 1e-9          # px: backward_f64 against mpmath on the 24 sampled pixels a window (measured 8.0e-13 px and 4.5e-16 in z at worst:
                              # six orders below BACKWARD_WORST, so float64 stands for the exact value here)
RIGS = [(s, r) for s in P.SIZES for r in P.ROTATIONS]


def _ids(v):
    return "%dx%d" % v[:2] if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size,rname", RIGS, ids=_ids)
def test_backward_map_over_the_whole_window(kind, size, rname):
    w, h, f, K, R = P.rig(size, rname)
    m = P.from_rig(kind, f, K, R)
    win = PC.window_of(m.detect_roi(w, h)[0])
    u = np.arange(win[0], win[2] + 1, dtype=np.int64)[None, :]
    v = np.arange(win[1], win[3] + 1, dtype=np.int64)[:, None]
    xm, ym = m.build_maps(win)
    z32 = m.backward_xyz(u.astype(F), v.astype(F))[2]
    x64, y64, z64 = backward_f64(m, u, v)
    assert not (np.isnan(xm).any() or np.isnan(ym).any() or np.isnan(z64).any())
    dz = float(np.abs(z32.astype(D) - z64).max())
    sentinel = (xm == -1) & (ym == -1)
    decided, safe = np.abs(z64) > Z_MARGIN, z64 > Z_SAFE
    near_zero, grazing = int((~decided).sum()), int(((z64 > Z_MARGIN) & ~safe).sum())
    share = (near_zero + grazing) / xm.size
    err = float(max(np.abs(xm.astype(D) - x64 / z64)[safe].max(), np.abs(ym.astype(D) - y64 / z64)[safe].max())) if safe.any() else 0.0
    print("backward", PC.KIND_NAMES[kind], _ids(size), rname, "window", win, "%d px:" % xm.size, "z off by %.3e," % dz, int(sentinel.sum()), "sentinels,",
          "excluded %d with |z| <= %.2e and %d grazing (0 < z <= %g) = %.4f of the window," % (near_zero, Z_MARGIN, grazing, Z_SAFE, share),
          "%.3e px over the other %d" % (err, int(safe.sum())))
    assert dz <= Z_MARGIN, dz
    assert np.array_equal(sentinel[decided], (z64 <= 0)[decided]), "the sentinel set differs where z is decided"
    assert share <= EXCLUDED_CAP, share
    assert err <= BACKWARD_TOL, err
    # backward_f64 itself against mpmath, on 24 pixels of the window spread over it (the origin included where the window holds it)
    rng = np.random.default_rng(xm.size)
    pts = [(int(rng.integers(win[0], win[2] + 1)), int(rng.integers(win[1], win[3] + 1))) for _ in range(23)]
    pts.append((0, 0) if win[0] <= 0 <= win[2] and win[1] <= 0 <= win[3] else (win[0], win[1]))
    for pu, pv in pts:
        X, Y, Z = backward_mp(m, pu, pv)
        iy, ix = pv - win[1], pu - win[0]
        assert abs(float(Z) - z64[iy, ix]) <= 1e-12, (pu, pv, float(Z), z64[iy, ix])
        if z64[iy, ix] > Z_SAFE:
            assert abs(float(X / Z) - x64[iy, ix] / z64[iy, ix]) <= F64_VS_MP_TOL and abs(float(Y / Z) - y64[iy, ix] / z64[iy, ix]) <= F64_VS_MP_TOL, (pu, pv)


def test_the_recorded_worst_cases_are_the_measured_ones():
    """Z_WORST, BACKWARD_WORST and EXCLUDED_WORST are what the 42 windows give (to the digits written): a bound is twice a MEASURED figure."""
    dz, err, share = 0.0, 0.0, 0.0
    for kind in KINDS:
        for size, rname in RIGS:
            w, h, f, K, R = P.rig(size, rname)
            m = P.from_rig(kind, f, K, R)
            win = PC.window_of(m.detect_roi(w, h)[0])
            u = np.arange(win[0], win[2] + 1, dtype=np.int64)[None, :]
            v = np.arange(win[1], win[3] + 1, dtype=np.int64)[:, None]
            xm, ym = m.build_maps(win)
            x64, y64, z64 = backward_f64(m, u, v)
            dz = max(dz, float(np.abs(m.backward_xyz(u.astype(F), v.astype(F))[2].astype(D) - z64).max()))
            safe = z64 > Z_SAFE
            share = max(share, float(((z64 <= Z_SAFE) & (z64 > -Z_MARGIN)).sum()) / xm.size)
            if safe.any():
                err = max(err, float(np.abs(xm.astype(D) - x64 / z64)[safe].max()), float(np.abs(ym.astype(D) - y64 / z64)[safe].max()))
    print("worst over the 42 windows: z off by %.5e, %.4e px, excluded share %.4f" % (dz, err, share))
    assert 0.995 * Z_WORST <= dz <= Z_WORST and 0.995 * BACKWARD_WORST <= err <= BACKWARD_WORST and 0.995 * EXCLUDED_WORST <= share <= EXCLUDED_WORST, (dz, err, share)
