"""The contract of the planned warp's ROI verification, as a three-valued NumPy model (float64).  Imports nothing from the library.

A planned warp carries a ROI (tl.u, tl.v, br.u, br.v) that the caller computed earlier.  detectResultRoi truncates four float extrema towards
zero (W:83-86), so the plan is right exactly when every extremum lies in the truncation interval of its planned bound.  The device cannot
afford atan2f / acosf per pixel; it compares monotone stand-ins of the extrema with the stand-ins of the interval's ends:

    u = scale * atan2(x_, z_)            ~  the diamond angle d of (x_, z_), in [-2, 2]
    v = scale * y_ / |(x_, z_)|   (cyl)  ~  q = v / scale
    v = scale * (pi - acos w)     (sph)  ~  w = -cos(v / scale), in [-1, 1]

and allows 4e-6 * max(1, |stand-in of either end|) for the stand-ins' rounding.  What the model claims per bound, with
t = 2 * 4e-6 * max(1, |p_lo|, |p_hi|) (the documented allowance once for the interval and once more for the device's own v_rcp / v_rsq
error of about 1e-7 relative):

    MUST_FLAG   the extremum's stand-in lies outside [p_lo, p_hi] by more than t
    MUST_PASS   it lies inside by more than t
    NO_CLAIM    otherwise

A plan MUST_FLAG if any bound does, MUST_PASS if all four do, NO_CLAIM otherwise.  Two rules need no scan and are exact (MUST_FLAG):

    a planned u bound beyond +-(int)(scale * pi_f): mapForward's atan2f never leaves [-pi_f, pi_f];
    with a pole of the sphere inside the image (OpenCV's two pole tests), a planned value for the bound that pole dictates
    (north: br.v = (int)(float)(pi * scale); south: tl.v = 0) that is not the pole's own.

A pole inside the image also enters the other bounds as OpenCV has it (min / max with u = 0 and with the pole's v): the model applies
them to the border's extrema (truth), so a planned tl.u above 0 or br.u below 0 beside a pole MUST_FLAG by the interval rule.
"""
import math

import numpy as np

CYL, SPH = 0, 1
MUST_PASS, NO_CLAIM, MUST_FLAG = "must_pass", "no_claim", "must_flag"
ALLOWANCE = 4e-6
PI_F = float(np.float32(math.pi))


# ---------------------------------------------------------------- the stand-ins
def d_of_u(u, scale):
    """The diamond angle of the direction u / scale, clamped to [-pi, pi]: increasing from -2 to 2."""
    th = float(u) / float(scale)
    if abs(th) >= math.pi:
        return math.copysign(2.0, th)
    s, c = abs(math.sin(th)), abs(math.cos(th))
    t = s / (s + c)
    d = t if math.cos(th) >= 0.0 else 2.0 - t
    return -d if th < 0.0 else d


def q_of_v(v, scale):
    return float(v) / float(scale)


def w_of_v(v, scale):
    """-cos(v / scale) with v / scale clamped to [0, pi]: increasing from -1 (south pole, v = 0) to 1 (north pole, v = pi scale)."""
    return -math.cos(max(0.0, min(math.pi, float(v) / float(scale))))


def stand_in(kind, k, value, scale):
    if k in (0, 2):
        return d_of_u(value, scale)
    return w_of_v(value, scale) if kind == SPH else q_of_v(value, scale)


def trunc_interval(bound):
    """(int)x == bound  <=>  x in (bound - 1, bound] / (-1, 1) / [bound, bound + 1)"""
    if bound < 0:
        return bound - 1.0, float(bound)
    if bound > 0:
        return float(bound), bound + 1.0
    return -1.0, 1.0


def f2i(x):
    return int(np.float32(x)) if abs(float(x)) < 2147483648.0 else -2147483648


# ---------------------------------------------------------------- poles, scan kind
def _f32(x):
    return np.float32(x)


def sph_poles(K, R, sw, sh, margin=0.0):
    """OpenCV SphericalWarper::detectResultRoi's two pole tests in its own float arithmetic (the south test negates y only)."""
    K = np.asarray(K, np.float32).reshape(3, 3)
    R = np.asarray(R, np.float32).reshape(3, 3)
    out = []
    for sign in (1.0, -1.0):
        x, y, z = R[1, 0], _f32(sign) * R[1, 1], R[1, 2]
        inside = False
        if y > 0:
            with np.errstate(all="ignore"):
                x_ = (K[0, 0] * x + K[0, 1] * y) / z + K[0, 2]
                y_ = K[1, 1] * y / z + K[1, 2]
            inside = bool(x_ > -margin and x_ < sw + margin and y_ > -margin and y_ < sh + margin)
        out.append(inside)
    return out[0], out[1]


def scan_kind(kind, K, R, r_kinv, sw, sh):
    """The launch a verification takes: 'roi_border_sph' (every spherical camera), 'roi_border' (a cylindrical camera whose extrema are
    provably on the image's border: the four corners in front of it, R[1][1] > 0, no pole of the cylinder within 2 px of the image) or
    'roi_scan' (every pixel), and for the last the reason."""
    if kind == SPH:
        return "roi_border_sph", None
    r = np.asarray(r_kinv, np.float32).reshape(9)
    for x in (0.0, sw - 1.0):
        for y in (0.0, sh - 1.0):
            z_ = r[6] * _f32(x) + r[7] * _f32(y) + r[8]
            if not z_ > np.float32(1e-6):
                return "roi_scan", "corner_behind"
    if not np.asarray(R, np.float32).reshape(3, 3)[1, 1] > 0:
        return "roi_scan", "rolled"
    north, south = sph_poles(K, R, sw, sh, 2.0)
    if north or south:
        return "roi_scan", "cyl_pole"
    return "roi_border", None


# ---------------------------------------------------------------- the truth, from the oracle
def truth(oracle, kind, scale, K, R, sw, sh):
    """-> dict(roi, extrema (float64, before truncation; a pole's min / max applied), north, south, r_kinv).  Cylindrical: the oracle's scan of
    every pixel.  Spherical: the oracle's mapForward over the 2 (W + H) border pixels, then OpenCV's truncation and pole rules, which must
    give the oracle's own ROI."""
    _k, _rinv, r_kinv, _ = oracle.camera(K, R)
    roi, mm = oracle.detect_roi(kind, scale, K, R, sw, sh)
    roi = [int(v) for v in roi]
    if kind == CYL:
        return dict(roi=roi, extrema=[float(v) for v in mm], north=False, south=False, r_kinv=r_kinv)
    pts = [(x, y) for x in range(sw) for y in (0, sh - 1)] + [(x, y) for y in range(sh) for x in (0, sw - 1)]
    uv = np.array([oracle.map_forward(kind, scale, r_kinv, float(x), float(y)) for x, y in pts], np.float64)
    e = [uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()]
    north, south = sph_poles(K, R, sw, sh)
    pv = float(np.float32(math.pi * float(np.float32(scale))))
    if north:
        e = [min(e[0], 0.0), min(e[1], pv), max(e[2], 0.0), max(e[3], pv)]
    if south:
        e = [min(e[0], 0.0), min(e[1], 0.0), max(e[2], 0.0), max(e[3], 0.0)]
    assert [f2i(v) for v in e] == roi, (e, roi, north, south)
    return dict(roi=roi, extrema=[float(v) for v in e], north=north, south=south, r_kinv=r_kinv)


# ---------------------------------------------------------------- the verdict
def exact_rule(kind, scale, planned, north=False, south=False):
    """The name of the exact rule the plan breaks, or None."""
    lim = f2i(np.float32(scale) * np.float32(PI_F))
    if abs(int(planned[0])) > lim or abs(int(planned[2])) > lim:
        return "u_beyond_pi"
    if kind == SPH and north and int(planned[3]) != f2i(np.float32(math.pi * float(np.float32(scale)))):
        return "north_pole"
    if kind == SPH and south and int(planned[1]) != 0:
        return "south_pole"
    return None


DOMAIN = {"d": (-2.0, 2.0), "w": (-1.0, 1.0), "q": (-math.inf, math.inf)}


def bound_verdict(kind, scale, k, planned_k, extremum):
    lo, hi = trunc_interval(int(planned_k))
    p_lo, p_hi, p_e = stand_in(kind, k, lo, scale), stand_in(kind, k, hi, scale), stand_in(kind, k, extremum, scale)
    t = 2.0 * ALLOWANCE * max(1.0, abs(p_lo), abs(p_hi))
    if not math.isfinite(p_e):
        return NO_CLAIM
    # an end of the interval at the end of the stand-in's range (the back seam, a pole) cannot be crossed: nothing to allow for there
    d_lo, d_hi = DOMAIN["d" if k in (0, 2) else "w" if kind == SPH else "q"]
    lo_open, hi_open = p_lo <= d_lo < p_hi, p_hi >= d_hi > p_lo
    if (not lo_open and p_e < p_lo - t) or (not hi_open and p_e > p_hi + t):
        return MUST_FLAG
    if (lo_open or p_e > p_lo + t) and (hi_open or p_e < p_hi - t):
        return MUST_PASS
    return NO_CLAIM


def verdict(kind, scale, planned, extrema, north=False, south=False):
    """-> (MUST_PASS | NO_CLAIM | MUST_FLAG, [per bound or the exact rule's name])"""
    rule = exact_rule(kind, scale, planned, north, south)
    if rule is not None:
        return MUST_FLAG, [rule]
    per = []
    for k in range(4):
        if kind == SPH and ((north and k == 3) or (south and k == 1)):
            per.append(MUST_PASS)          # the pole's own value (exact_rule): nothing the border could change
            continue
        per.append(bound_verdict(kind, scale, k, planned[k], extrema[k]))
    if MUST_FLAG in per:
        return MUST_FLAG, per
    return (MUST_PASS if all(p == MUST_PASS for p in per) else NO_CLAIM), per


SHIFTS = [(k, s) for k in range(4) for s in (-1, 1)]


def shifted(roi, k, s):
    r = [int(v) for v in roi]
    r[k] += s
    return r
