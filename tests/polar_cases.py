"""The fixed inputs of the proj_math.hpp self-tests (csrc/proj_math.hpp: sinf, cosf, atan2f, atanf, acosf), shared by tests/test_polar_model.py
(host compilation against tests/helpers/polar_np.py) and tests/test_gpu_polar_math.py (device compilation against the host): per function
every special value, the break points of its polynomials with their float32 neighbours, and a seeded random sweep."""
import numpy as np

F = np.float32
SIN, COS, ATAN2, ATAN, ACOS = range(5)
NAMES = {SIN: "sinf", COS: "cosf", ATAN2: "atan2f", ATAN: "atanf", ACOS: "acosf"}
N = 100000
_SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 1e-30, 3e38, -3e38, 1.17549435e-38]


def _around(vals):
    """every value with its two float32 neighbours, and the negatives"""
    v = np.asarray(vals, F)
    v = np.concatenate([v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))])
    return np.concatenate([v, -v])


def sweep(fn):
    """(in, in2): float32 arrays; in2 is None except for atan2f."""
    rng = np.random.default_rng(20261020 + fn)
    if fn in (SIN, COS):
        quarter = _around((np.arange(0, 65) * (np.pi / 4)).astype(F))                       # the reduction's break points
        far = _around([2.0 ** 20, 2.0 ** 28, 2.0 ** 20 * np.pi, 1e6, 1e7])                     # the last one served and the first one refused
        x = np.concatenate([np.asarray(_SPECIAL, F), quarter, far, rng.uniform(-2 * np.pi, 2 * np.pi, N).astype(F),
                            rng.uniform(-2.0 ** 20, 2.0 ** 20, N).astype(F), (rng.choice([-1, 1], N) * np.exp(rng.uniform(-40, 20, N))).astype(F)])
        return x, None
    if fn == ATAN:
        x = np.concatenate([np.asarray(_SPECIAL, F), _around([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66]), rng.uniform(-3, 3, N).astype(F),
                            (rng.choice([-1, 1], N) * np.exp(rng.uniform(-60, 60, N))).astype(F)])
        return x, None
    if fn == ACOS:
        x = np.concatenate([np.asarray(_SPECIAL, F), _around([0.5, 1.0, 0.0, 2.0]), rng.uniform(-1, 1, N).astype(F),
                            (F(1) - np.exp(rng.uniform(-17, 0, N)).astype(F)) * rng.choice([-1, 1], N).astype(F)])
        return x.astype(F), None
    sp = np.asarray(_SPECIAL, F)
    ys, xs = [a.ravel() for a in np.meshgrid(sp, sp)]                                        # every pair of special values
    xb = np.exp(rng.uniform(-5, 5, 64)).astype(F)
    bk = _around([0.4375, 0.6875, 1.1875, 2.4375])
    yb, xb2 = [a.ravel() for a in np.meshgrid(bk, xb)]
    y = np.concatenate([ys, yb * xb2, yb * -xb2, (rng.choice([-1, 1], N) * np.exp(rng.uniform(-30, 30, N))).astype(F), rng.uniform(-100, 100, N).astype(F)])
    x = np.concatenate([xs, xb2, -xb2, (rng.choice([-1, 1], N) * np.exp(rng.uniform(-30, 30, N))).astype(F), rng.uniform(-100, 100, N).astype(F)])
    return y.astype(F), x.astype(F)


def accuracy_sweep(fn):
    """The sweep of the ulp table: sinf / cosf on [-2 pi, 2 pi], the other functions on their natural domains."""
    rng = np.random.default_rng(777 + fn)
    n = 400000
    if fn in (SIN, COS):
        return rng.uniform(-2 * np.pi, 2 * np.pi, n).astype(F), None
    if fn == ATAN:
        return np.concatenate([rng.uniform(-4, 4, n // 2), rng.choice([-1, 1], n // 2) * np.exp(rng.uniform(-40, 40, n // 2))]).astype(F), None
    if fn == ACOS:
        return rng.uniform(-1, 1, n).astype(F), None
    return (rng.choice([-1, 1], n) * np.exp(rng.uniform(-20, 20, n))).astype(F), (rng.choice([-1, 1], n) * np.exp(rng.uniform(-20, 20, n))).astype(F)


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def ulp_distance(a, ref):
    """max distance in float32 steps between a and the float64 reference rounded to float32 (NaN positions excluded)"""
    a, r = np.asarray(a, F), np.asarray(ref, np.float64).astype(F)
    ok = ~(np.isnan(a) | np.isnan(r))

    def order(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(order(a[ok]) - order(r[ok])).max())


# ---- rigs, windows and expected tiles of the GPU tests (tests/test_gpu_polar_*.py) -------------------------------------------------------------
KIND_NAMES = {3: "fisheye", 4: "stereographic"}
NEAREST, LINEAR, TIES_EVEN = 0, 1, 0x100
CONST, REPL, REFLECT, WRAP, REFLECT101 = 0, 1, 2, 3, 4
FULL_WARP_PIXELS = 300000          # a rig whose ROI is larger is "blown up": its ROI and windows of it are tested, never the full warp


def window_of(roi, far=False):
    """The rectangle (tl.x, tl.y, br.x, br.y) the warp tests of a rig use: its whole ROI, or for a blown-up rig a 128 x 96 window that holds the
    destination origin (r = 0: the pole) - with far=True one that ends at the ROI's far corner instead (large r)."""
    roi = tuple(int(v) for v in roi)
    if (roi[2] - roi[0] + 1) * (roi[3] - roi[1] + 1) <= FULL_WARP_PIXELS:
        return roi
    if far:
        return (roi[2] - 127, roi[3] - 95, roi[2], roi[3])
    return (-61, -50, 66, 45)


def image(rng, h, w, cn=3, dtype=np.uint8):
    a = rng.integers(0, 256, (h, w, cn) if cn > 1 else (h, w)).astype(np.uint8)
    return a if dtype == np.uint8 else a.astype(F) * F(1.37)


def gained(tile, gain):
    """GainCompensator::apply on a CV_8U tile: saturate_cast<uchar>(cvRound(byte * gain))"""
    return np.clip(np.rint(tile.astype(np.float64) * gain), 0, 255).astype(np.uint8)
