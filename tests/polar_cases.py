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


# ---- where the ROI scan's extrema sit (tests/test_polar_scan_census.py on the CPU, tests/test_gpu_polar_scan.py on the device) -------------------
# k_polar_roi_scan reduces SCAN_COLS columns x SCAN_ROWS rows a block: 4 waves of 64 columns through shuffles, the 4 waves through LDS, the
# blocks through four atomics.  On the named rigs above every extremum sits on the image border or at the pole, in column block 0 or 1.  The
# rigs here put the extrema where each step of that reduction has to carry them.  "far" is the camera that looks at the point both maps send
# furthest from the destination origin - the fisheye antipole (pitch -pi/2: r = pi * scale) and the stereographic pole (pitch +pi/2: r ->
# inf, the pixel on it 0 / 0) - so the four extrema are the four neighbours of the principal point (cx, cy), which K places at will.
SCAN_COLS, SCAN_ROWS, WAVE = 256, 16, 64
SCAN_CLASSES = ("col_block_0", "col_block_1", "col_block_2plus", "wave_0", "wave_1", "wave_2", "wave_3", "lane_32plus", "partial_last_col_block",
                "middle_full_row_band", "partial_last_row_band", "interior")
FAR = {3: "pitch-pi/2", 4: "pitch+pi/2"}
# name: (w, h, f, cx, cy, rotation name or "far", the classes the rig is here for - with both kinds, by the model alone)
SCAN_RIGS = {
    "800x40_block2_wave2": (800, 40, 60.0, 700.0, 20.0, "far", ("col_block_2plus", "wave_2", "lane_32plus", "middle_full_row_band", "interior")),
    "800x40_last_blocks": (800, 40, 60.0, 790.0, 36.0, "far", ("col_block_2plus", "wave_0", "partial_last_col_block", "partial_last_row_band", "interior")),
    "600x37_block1_wave0": (600, 37, 50.0, 300.0, 5.0, "far", ("col_block_1", "wave_0", "lane_32plus", "interior")),
    "600x37_block1_wave1": (600, 37, 50.0, 330.0, 20.0, "far", ("col_block_1", "wave_1", "middle_full_row_band", "interior")),
    "600x37_block1_wave3": (600, 37, 50.0, 470.0, 34.0, "far", ("col_block_1", "wave_3", "partial_last_row_band", "interior")),
    "257x17_last_column": (257, 17, 30.0, 256.0, 16.0, "far", ("col_block_1", "wave_0", "partial_last_col_block", "partial_last_row_band")),
    "256x16_one_block": (256, 16, 30.0, 128.0, 8.0, "identity", ("col_block_0",)),
    "800x40_border": (800, 40, 300.0, 400.0, 20.0, "yaw0.52", ("col_block_0", "col_block_2plus")),
    "1x1": (1, 1, 5.0, 0.5, 0.5, "identity", ("col_block_0",)),
    "1x40": (1, 40, 20.0, 0.5, 20.0, "yaw0.52", ("col_block_0", "partial_last_row_band")),
    "300x1": (300, 1, 100.0, 150.0, 0.5, "pitch+pi/3", ("col_block_0",)),
}


def scan_rig(name, kind):
    """(w, h, scale, K, R) of a scan rig for the kind"""
    from helpers import polar_np as P
    w, h, f, cx, cy, rname, _ = SCAN_RIGS[name]
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], F)
    return w, h, F(f), K, P.ROTATIONS[FAR[kind] if rname == "far" else rname].astype(F)


def scan_extrema(model, w, h):
    """The source pixel (x, y) that holds each of detectResultRoi's four extrema (min u, min v, max u, max v) in the model: the first one
    in row order where several hold the value; None where every pixel is NaN."""
    xs, ys = np.meshgrid(np.arange(w, dtype=np.int64).astype(F), np.arange(h, dtype=np.int64).astype(F))
    u, v = model.map_forward(xs, ys)
    out = []
    for a, is_min in ((u, True), (v, True), (u, False), (v, False)):
        b = np.where(np.isnan(a), np.inf if is_min else -np.inf, a.astype(np.float64))
        i = int(np.argmin(b) if is_min else np.argmax(b))
        out.append(None if np.isinf(b.flat[i]) and np.isnan(a.flat[i]) else (i % w, i // w))
    return out


def scan_classes(x, y, w, h):
    """The classes of SCAN_CLASSES that an extremum at source pixel (x, y) of a w x h source exercises in the scan's reduction."""
    cb, rb = x // SCAN_COLS, y // SCAN_ROWS
    last_cb, last_rb = (w - 1) // SCAN_COLS, (h - 1) // SCAN_ROWS
    got = {"col_block_0" if cb == 0 else "col_block_1" if cb == 1 else "col_block_2plus"}
    if cb >= 1:
        got.add("wave_%d" % (x % SCAN_COLS // WAVE))
    if x % WAVE >= 32:
        got.add("lane_32plus")
    if cb == last_cb and w % SCAN_COLS:
        got.add("partial_last_col_block")
    if 0 < rb < last_rb:
        got.add("middle_full_row_band")
    if rb == last_rb and h % SCAN_ROWS:
        got.add("partial_last_row_band")
    if 0 < x < w - 1 and 0 < y < h - 1:
        got.add("interior")
    return got


# A camera whose mapForward is NaN on every source pixel, which setCameraParams accepts (finite K and R): K^-1 = 1e-30 * I, so x_ * x_ + y_ * y_
# + z_ * z_ underflows to 0 and y_ / sqrtf(0) is +-inf or 0 / 0 - acosf gives NaN either way.
NAN_CAMERA = (np.diag([1e30, 1e30, 1e30]).astype(F), np.eye(3, dtype=F))
