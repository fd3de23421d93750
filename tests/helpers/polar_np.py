"""cv::detail::FisheyeWarper and cv::detail::StereographicWarper (OpenCV 3.4.x warpers_inl.hpp: FisheyeProjector, StereographicProjector,
RotationWarperBase::detectResultRoi) restated in NumPy, with the five transcendentals of imagestitch_amd/csrc/proj_math.hpp.

TEST INFRASTRUCTURE ONLY.  OpenCV's source is in neither tree: the projector formulas are recalled, parity with OpenCV is UNPINNED (as for
the spherical and plane projectors), and what the host and the GPU are held to is THIS restatement, bit for bit.

The maps are float32: every + - * / sqrt is its own rounded float32 operation, left to right as the C++ is written, no fused multiply-add.
The five library calls (sinf, cosf, atan2f, atanf, acosf) take a float32 and return a float32; inside, each widens its argument to float64
(exact), evaluates a fixed sequence of float64 + - * / sqrt operations - one rounded operation per parenthesis, written out below - and
rounds the result to float32 once.  float64 arithmetic is IEEE on the host, on the device and in NumPy, so the three agree bit for bit.

    sinf, cosf   |x| <= 2^28: k = rint(x * 2 / pi); r = (x - k * P1) - k * P1T with P1 the first 25 bits of pi / 2 (k * P1 is exact for
                 |k| < 2^28), then the degree-7 / degree-8 polynomials of FreeBSD's k_sinf.c / k_cosf.c on |r| <= pi / 4, chosen by k mod 4.
                 |x| > 2^28, an infinity or a NaN: NaN (the defined fallback; mapBackward then takes its (-1, -1) branch).
    atanf        fdlibm's s_atan.c: four break points (7/16, 11/16, 19/16, 39/16), one division, the 11-term polynomial.  atanf(+-inf) =
                 +-(float)(pi / 2); NaN -> NaN; the sign is copied from x (atanf(-0) = -0).
    atan2f       NaN -> NaN; y == 0: +-0 for x with a clear sign bit, +-(float)pi otherwise (atan2f(+-0, -0) = +-pi, atan2f(+-0, +0) = +-0);
                 x == 0: +-pi / 2; both infinite: +-pi / 4 or +-3 pi / 4; otherwise atan(|y / x|) (the quotient in float64), pi - that for
                 x < 0, the sign of y.
    acosf        |x| > 1 or NaN: NaN; otherwise bundle_math.hpp's bm_acos (fdlibm's e_acos.c, tests/helpers/bundle_np.py) rounded to float32.
"""
import numpy as np

F = np.float32
D = np.float64
INT_MIN = -2147483648
_FLT_MAX = np.finfo(np.float32).max
PI_F = F(3.1415926535897932384626433832795)
FISHEYE, STEREOGRAPHIC = 3, 4

# ---- proj_math.hpp, operation for operation (float64 arrays) --------------------------------------------------------------------------------
RND = D(6755399441055744.0)                 # 1.5 * 2^52
INVPIO2 = D(6.36619772367581382433e-01)
PIO2_1 = D(1.57079631090164184570e+00)      # the first 25 bits of pi / 2
PIO2_1T = D(1.58932547735281966916e-08)     # pi / 2 - PIO2_1
TRIG_MAX = F(268435456.0)                   # 2^28
S1, S2, S3, S4 = D(-0.166666666416265235595), D(0.0083333293858894631756), D(-0.000198393348360966317347), D(0.0000027183114939898219064)
C0, C1, C2, C3 = D(-0.499999997251031003120), D(0.0416666233237390631894), D(-0.00138867637746099294692), D(0.0000243904487962774090654)
PI_D, PIO2_D, PIO4_D, PI3O4_D = D(3.14159265358979311600e+00), D(1.57079632679489655800e+00), D(7.85398163397448278999e-01), D(2.35619449019234483700e+00)
ATAN_BREAKS = (D(0.4375), D(0.6875), D(1.1875), D(2.4375))
ATAN_HI = (D(0.0), D(4.63647609000806093515e-01), D(7.85398163397448278999e-01), D(9.82793723247329054082e-01), D(1.57079632679489655800e+00))
AT = [D(v) for v in (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                     9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                     4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)]
NAN_F = F(np.nan)


def _ksin(r):
    z = r * r
    w = z * z
    t = S3 + (z * S4)
    s = z * r
    return (r + (s * (S1 + (z * S2)))) + ((s * w) * t)


def _kcos(r):
    z = r * r
    w = z * z
    t = C2 + (z * C3)
    return ((D(1.0) + (z * C0)) + (w * C1)) + ((w * z) * t)


def _sincos_d(x):
    """(sin, cos) of a float64 array with |x| <= 2^28, in float64."""
    k = ((x * INVPIO2) + RND) - RND
    r = (x - (k * PIO2_1)) - (k * PIO2_1T)
    q = k - (D(4.0) * (((k * D(0.25)) + RND) - RND))
    s, c = _ksin(r), _kcos(r)
    sn = np.where(q == 0.0, s, np.where(q == 1.0, c, np.where(q == -1.0, -c, -s)))
    cs = np.where(q == 0.0, c, np.where(q == 1.0, -s, np.where(q == -1.0, s, -c)))
    return sn, cs


def sincosf(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        ok = np.abs(x) <= TRIG_MAX                     # false for a NaN
        s, c = _sincos_d(np.where(ok, x, F(0)).astype(D))
        return np.where(ok, s.astype(F), NAN_F), np.where(ok, c.astype(F), NAN_F)


def sinf(x):
    return sincosf(x)[0]


def cosf(x):
    return sincosf(x)[1]


def _atan_d(a):
    """atan of a float64 array of non-negative values (an infinity included), in float64."""
    b0, b1, b2, b3 = ATAN_BREAKS
    with np.errstate(all="ignore"):
        i = (a >= b0).astype(int) + (a >= b1) + (a >= b2) + (a >= b3)
        n = np.choose(i, [a, (D(2.0) * a) - D(1.0), a - D(1.0), a - D(1.5), np.full_like(a, -1.0)])
        d = np.choose(i, [np.ones_like(a), D(2.0) + a, a + D(1.0), D(1.0) + (D(1.5) * a), a])
        hi = np.choose(i, [np.full_like(a, h) for h in ATAN_HI])
        t = n / d
        z = t * t
        w = z * z
        s1 = z * (AT[0] + (w * (AT[2] + (w * (AT[4] + (w * (AT[6] + (w * (AT[8] + (w * AT[10]))))))))))
        s2 = w * (AT[1] + (w * (AT[3] + (w * (AT[5] + (w * (AT[7] + (w * AT[9]))))))))
        return hi - ((t * (s1 + s2)) - t)


def atanf(x):
    x = np.asarray(x, F)
    nan = np.isnan(x)
    r = _atan_d(np.abs(np.where(nan, F(0), x)).astype(D))
    return np.where(nan, NAN_F, np.copysign(r, x.astype(D)).astype(F))


def atan2f(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, F), np.asarray(x, F))
    nan = np.isnan(x) | np.isnan(y)
    yd, xd = np.where(nan, F(1), y).astype(D), np.where(nan, F(1), x).astype(D)
    with np.errstate(all="ignore"):
        t = _atan_d(np.abs(yd / xd))
        gen = np.where(xd < 0.0, PI_D - t, t)
        both_inf = np.isinf(xd) & np.isinf(yd)
        r = np.where(yd == 0.0, np.where(np.signbit(xd), PI_D, D(0.0)),
                     np.where(xd == 0.0, PIO2_D, np.where(both_inf, np.where(xd > 0.0, PIO4_D, PI3O4_D), gen)))
    return np.where(nan, NAN_F, np.copysign(r, yd).astype(F))


def _asin_r(z):
    p = z * (1.66666666666666657415e-01 + (z * (-3.25565818622400915405e-01 + (z * (2.01212532134862925881e-01 + (z * (-4.00555345006794114027e-02 + (
        z * (7.91534994289814532176e-04 + (z * 3.47933107596021167570e-05))))))))))
    q = 1.0 + (z * (-2.40339491173441421878e+00 + (z * (2.02094576023350569471e+00 + (z * (-6.88283971605453293030e-01 + (z * 7.70381505559019352791e-02)))))))
    return p / q


def _acos_d(x):
    """bundle_math.hpp's bm_acos (tests/helpers/bundle_np.py: acos) on a float64 array in [-1, 1]."""
    lo, pi = D(6.12323399573676603587e-17), D(3.14159265358979311600e+00)
    mid = PIO2_D - (x - (lo - (x * _asin_r(x * x))))
    zn = (D(1.0) + x) * D(0.5)
    sn = np.sqrt(zn)
    neg = pi - (D(2.0) * (sn + ((_asin_r(zn) * sn) - lo)))
    zp = (D(1.0) - x) * D(0.5)
    sp = np.sqrt(zp)
    pos = D(2.0) * (sp + (_asin_r(zp) * sp))
    return np.where((x < 0.5) & (x > -0.5), mid, np.where(x < 0.0, neg, pos))


def acosf(x):
    x = np.asarray(x, F)
    ok = np.abs(x) <= F(1)                             # false for a NaN
    with np.errstate(all="ignore"):
        return np.where(ok, _acos_d(np.where(ok, x, F(0)).astype(D)).astype(F), NAN_F)


FUNCS = {0: ("sinf", sinf), 1: ("cosf", cosf), 2: ("atan2f", atan2f), 3: ("atanf", atanf), 4: ("acosf", acosf)}     # isx_selftest_proj_math's fn


def f2i(v):
    """static_cast<int>(float) as x86 does it (cvttss2si): truncation toward zero; NaN and out-of-range give INT_MIN."""
    v = float(v)
    return int(v) if abs(v) < 2147483648.0 else INT_MIN


class Polar:
    """One of the two projectors with a camera: kind FISHEYE or STEREOGRAPHIC."""

    def __init__(self, kind, scale):
        assert kind in (FISHEYE, STEREOGRAPHIC)
        self.kind, self.scale = kind, F(scale)
        self.r_kinv = np.zeros(9, F)
        self.k_rinv = np.zeros(9, F)

    def set_camera(self, r_kinv, k_rinv):
        self.r_kinv = np.asarray(r_kinv, F).reshape(9).copy()
        self.k_rinv = np.asarray(k_rinv, F).reshape(9).copy()
        return self

    def map_forward(self, x, y):
        r = self.r_kinv
        x, y = np.asarray(x, F), np.asarray(y, F)
        with np.errstate(all="ignore"):
            x_ = r[0] * x + r[1] * y + r[2]
            y_ = r[3] * x + r[4] * y + r[5]
            z_ = r[6] * x + r[7] * y + r[8]
            u_ = atan2f(x_, z_)
            v_ = PI_F - acosf(y_ / np.sqrt(x_ * x_ + y_ * y_ + z_ * z_))
            su, cu = sincosf(u_)
            if self.kind == FISHEYE:
                return self.scale * v_ * cu, self.scale * v_ * su
            sv, cv = sincosf(v_)
            rr = sv / (F(1) - cv)
            return self.scale * rr * cu, self.scale * rr * su

    def backward_xyz(self, u, v):
        """mapBackward up to its division: (x, y, z) of k_rinv times the ray, float32 (tests/test_polar_accuracy.py measures z)"""
        k = self.k_rinv
        u, v = np.broadcast_arrays(np.asarray(u, F), np.asarray(v, F))
        with np.errstate(all="ignore"):
            u = u / self.scale
            v = v / self.scale
            u_ = atan2f(v, u)
            r = np.sqrt(u * u + v * v)
            v_ = r if self.kind == FISHEYE else F(2) * atanf(F(1) / r)
            sinv, cosv = sincosf(PI_F - v_)
            su, cu = sincosf(u_)
            x_ = sinv * su
            y_ = cosv
            z_ = sinv * cu
            x = k[0] * x_ + k[1] * y_ + k[2] * z_
            y = k[3] * x_ + k[4] * y_ + k[5] * z_
            z = k[6] * x_ + k[7] * y_ + k[8] * z_
            return x, y, z

    def map_backward(self, u, v):
        x, y, z = self.backward_xyz(u, v)
        with np.errstate(all="ignore"):
            front = z > 0
            return np.where(front, x / z, F(-1)).astype(F), np.where(front, y / z, F(-1)).astype(F)

    def detect_roi(self, w, h):
        """RotationWarperBase::detectResultRoi: mapForward of every source pixel, (std::min)(tl, u) / (std::max)(br, u) from +-FLT_MAX (a NaN
        never replaces a value), four static_cast<int>."""
        xs, ys = np.meshgrid(np.arange(w, dtype=np.int64).astype(F), np.arange(h, dtype=np.int64).astype(F))
        u, v = self.map_forward(xs, ys)
        mm = []
        with np.errstate(all="ignore"):
            for a, is_min in ((u, True), (v, True), (u, False), (v, False)):
                a = a[~np.isnan(a)]
                if is_min:
                    m = F(min(_FLT_MAX, a.min())) if a.size else F(_FLT_MAX)
                else:
                    m = F(max(-_FLT_MAX, a.max())) if a.size else F(-_FLT_MAX)
                mm.append(m)
        mm = np.array(mm, F)
        return np.array([f2i(m) for m in mm], np.int64), mm

    def build_maps(self, roi):
        u = np.arange(int(roi[0]), int(roi[2]) + 1, dtype=np.int64).astype(F)[None, :]
        v = np.arange(int(roi[1]), int(roi[3]) + 1, dtype=np.int64).astype(F)[:, None]
        x, y = self.map_backward(u, v)
        return np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)


def camera(K, R):
    """setCameraParams as warp.hip's make_proj and the oracle compute it: K^-1 in closed form in float64 rounded once, the two 3 x 3
    products accumulated in float64 and rounded once -> (r_kinv, k_rinv) as float32[9]."""
    K = np.asarray(K, F).reshape(3, 3).astype(D)
    R = np.asarray(R, F).reshape(3, 3).astype(D)
    S = K
    det = S[0, 0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) - S[0, 1] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0]) + S[0, 2] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0])
    i = 1.0 / det
    kinv = np.array([[(S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) * i, (S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]) * i, (S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]) * i],
                     [(S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]) * i, (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) * i, (S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]) * i],
                     [(S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]) * i, (S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]) * i, (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) * i]], D).astype(F).astype(D)

    def mul(a, b):
        out = np.zeros((3, 3), D)
        for r in range(3):
            for c in range(3):
                s = D(0.0)
                for k in range(3):
                    s = s + a[r, k] * b[k, c]
                out[r, c] = s
        return out.astype(F).reshape(9)
    return mul(R, kinv), mul(K, R.T.copy())


def from_rig(kind, scale, K, R):
    r_kinv, k_rinv = camera(K, R)
    return Polar(kind, scale).set_camera(r_kinv, k_rinv)


# ---- the rigs of the tests: K = [[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], scale = f ---------------------------------------------------------
SIZES = [(37, 29, 25.0), (64, 48, 40.0), (261, 67, 90.0)]


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


ROTATIONS = {"identity": np.eye(3), "yaw0.52": rot("y", 0.52), "yaw2.97": rot("y", 2.97), "pitch+pi/3": rot("x", np.pi / 3), "pitch-pi/3": rot("x", -np.pi / 3),
             "pitch+pi/2": rot("x", np.pi / 2), "pitch-pi/2": rot("x", -np.pi / 2)}


def rig(size, rname):
    w, h, f = size
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F)
    return w, h, F(f), K, ROTATIONS[rname].astype(F)
