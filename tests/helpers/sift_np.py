"""NumPy model of isx_sift_find: SIFT::detectAndCompute(image, noArray()) as OpenCV 4.x defines it (features2d/src/sift.dispatch.cpp and
sift.simd.hpp, float DoG, SIFT_FIXPT_SCALE 1; neither file is in the reference tree, so OpenCV parity is UNPINNED): the standard of record
(DESIGN.md §8 "Features finder, SIFT").  Integers in int64, floats one rounded float32 operation at a time in the order written here.

Decisions (the GPU is held to this file bit for bit):
  * exp and exp2 are expf / exp2f below (imagestitch_amd/csrc/sift_math.hpp operation for operation), angles are polar_np.atan2f in degrees
    wrapped to [0, 360) where OpenCV calls fastAtan2, sin and cos are polar_np.sincosf; sqrt and / are the IEEE float32 operations
  * the six blur kernels of (sigma 1.6, 3 layers) are committed float32 bit patterns (TAPS); gaussian_taps regenerates them
  * a blur sums t[h] a[0], then for j = 1 .. h ascending t[h + j] (a[+j] + a[-j]); rows first into float32, then columns;
    BORDER_REFLECT_101 reflected repeatedly
  * every histogram bin sums its contributions in sample order (i outer, j inner)
  * a candidate is an extremum that survives adjustLocalExtrema; candidates lie in scan order (octave, layer, r, c of the STARTING pixel);
    of more than MAX_CANDIDATES the first in scan order are kept (STATUS_CANDIDATES)
  * a candidate is removed when an earlier one in scan order ends on the same (octave, layer, r, c)
  * candidates are ranked by response, size, octave, pt.y, pt.x descending, then by scan index ascending; keypoints follow their
    candidate's rank, then the ascending bin; count = min(total, nfeatures if nfeatures > 0) (retainBest without its keep-the-ties rule)
  * the contrast pre-threshold floor(0.5 contrast_threshold / 3 * 255) is computed in double and compared as a float (no int overflow)
"""
import numpy as np

from . import polar_np, resize_np
from .surf_np import gray  # noqa: F401  (the same gray as isx_orb_find and isx_surf_find)

f32 = np.float32
f64 = np.float64

MAX_CANDIDATES, MAX_SIDE, MAX_PIXELS = 32768, 8192, 1 << 23         # ISX_SIFT_MAX_CANDIDATES, ISX_SIFT_MAX_SIDE, ISX_SIFT_MAX_PIXELS
STATUS_TRUNCATED, STATUS_CANDIDATES = 1, 2                         # ISX_SIFT_TRUNCATED, ISX_SIFT_CANDIDATES_DROPPED
LAYERS, SIGMA = 3, 1.6
BORDER, MAX_STEPS, ORI_BINS, MAX_PEAKS = 5, 5, 36, 18
ORI_RADIUS_MAX = 16                                                # cvRound(4.5f * 1.6f * 2^(3.5 / 3))
DEG_F = f32(180.0 / np.pi)
RAD_F = f32(np.pi / 180.0)
FLT_EPSILON = f32(np.finfo(f32).eps)

# ---- sift_math.hpp, operation for operation -------------------------------------------------------------------------------------------
RND = f64(6755399441055744.0)                 # 1.5 * 2^52
INV_LN2 = f64(1.44269504088896338700e+00)
LN2_HI = f64(6.93147180369123816490e-01)      # the first 32 bits of ln 2 (k * LN2_HI is exact)
LN2_LO = f64(1.90821492927058770002e-10)      # ln 2 - LN2_HI
LN2 = f64(6.93147180559945286227e-01)
EXP_C = [f64(1.0) / f64(v) for v in (2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0)]   # 1 / n!, n = 2 .. 11


def _exp_core(x):
    """exp of a float64 array with |x| < 700, in float64"""
    k = ((x * INV_LN2) + RND) - RND
    r = (x - (k * LN2_HI)) - (k * LN2_LO)
    p = EXP_C[9]
    for c in EXP_C[8::-1]:
        p = c + (r * p)
    p = f64(1.0) + (r * (f64(1.0) + (r * p)))
    scale = ((k.astype(np.int64) + 1023) << 52).view(f64)
    return p * scale


def _exp_any(x, lo, hi, pre):
    x = np.asarray(x, f32)
    shape = x.shape
    x = np.atleast_1d(x)
    nan, big, small = np.isnan(x), x > f32(hi), x < f32(lo)
    with np.errstate(all="ignore"):
        xd = np.where(nan | big | small, f32(0), x).astype(f64)
        v = _exp_core(xd * pre if pre is not None else xd).astype(f32)
    v = np.where(small, f32(0), np.where(big, f32(np.inf), v))
    return np.where(nan, f32(np.nan), v).astype(f32).reshape(shape)


def expf(x):
    """pm_expf: NaN -> NaN, x > 89 -> inf, x < -104 -> 0"""
    return _exp_any(x, -104.0, 89.0, None)


def exp2f(x):
    """pm_exp2f: the same core on (double)x * ln 2; NaN -> NaN, x > 129 -> inf, x < -151 -> 0"""
    return _exp_any(x, -151.0, 129.0, LN2)


MATH_FUNCS = {0: ("expf", expf), 1: ("exp2f", exp2f)}      # isx_selftest_sift_math's fn


def ulp_error(got, x, fn):
    """|got - correctly rounded fn(x)| in float32 ulps of the exact value (got, x float32 arrays; fn = np.exp or np.exp2 in float64)"""
    exact = fn(np.asarray(x, f32).astype(f64))
    ulp = np.spacing(np.abs(exact).astype(f32)).astype(f64)
    return np.abs(np.asarray(got, f32).astype(f64) - exact) / ulp


# ---- the blur kernels -----------------------------------------------------------------------------------------------------------------
def sigmas():
    """[sig_diff of the base image, sig[1] .. sig[5]] in float64 as SIFT computes them"""
    out = [float(np.sqrt(max(SIGMA * SIGMA - 1.0, 0.01)))]
    k = 2.0 ** (1.0 / LAYERS)
    for i in range(1, LAYERS + 3):
        prev = (k ** float(i - 1)) * SIGMA
        total = prev * k
        out.append(float(np.sqrt(total * total - prev * prev)))
    return out


def width_of(s):
    return int(np.rint(s * 8.0 + 1.0)) | 1


def gaussian_taps(n, sigma):
    """getGaussianKernel(n, sigma) as GaussianBlur asks for it: exp in double, normalised in double, rounded to float32 once"""
    x = np.arange(n, dtype=f64) - (n - 1) * 0.5
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    total = 0.0
    for v in t:
        total += float(v)
    return (t * (1.0 / total)).astype(f32)


def regenerate_taps():
    """the six kernels from the formulas: [base blur, layer 1 .. layer 5]"""
    return [gaussian_taps(width_of(s), s) for s in sigmas()]


WIDTHS = (11, 11, 13, 17, 21, 27)
_BITS = (
    (0x38ddd93e, 0x3af825aa, 0x3c9234f8, 0x3db581b7, 0x3e6d6298, 0x3ea389e7),
    (0x38a76fd6, 0x3ad0a03d, 0x3c85aeef, 0x3db03687, 0x3e6ee6fe, 0x3ea691b2),
    (0x390fc865, 0x3ab40040, 0x3c14382a, 0x3d208e6a, 0x3de4cae5, 0x3e567243, 0x3e84353b),
    (0x3838c8a9, 0x39a72d49, 0x3ae8546e, 0x3bf7fb5c, 0x3ccb4ae0, 0x3d7fffdd, 0x3df79882, 0x3e37ec06, 0x3e51dd7e),
    (0x3827705b, 0x394b1a53, 0x3a50a0e3, 0x3b357aea, 0x3c05af59, 0x3ca6c9a4, 0x3d303713, 0x3d9da8dc, 0x3deee7bc, 0x3e1948e0, 0x3e269236),
    (0x379b5026, 0x388fc81f, 0x396fbe10, 0x3a33ffe9, 0x3af369c2, 0x3b9437e2, 0x3c228e8c, 0x3ca08e1d, 0x3d0ecf5d, 0x3d64ca77, 0x3da50bb5, 0x3dd671db,
     0x3dfaec87, 0x3e0434fb),
)
# each kernel is symmetric: the committed half up to the centre, mirrored
TAPS = [np.array(b + b[-2::-1], np.uint32).view(f32) for b in _BITS]


class Params:
    def __init__(self, nfeatures=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
        assert n_octave_layers == LAYERS and sigma == SIGMA
        self.nfeatures, self.contrast_threshold, self.edge_threshold = int(nfeatures), float(contrast_threshold), float(edge_threshold)


def cv_round(v):
    return int(np.rint(v))


# ---- 1: the base image and the pyramid -------------------------------------------------------------------------------------------------
def reflect101(p, n):
    """BORDER_REFLECT_101 of an index array, reflected until inside; a side of 1 maps everything to 0"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * (n - 1) - p, p)
        if ((p >= 0) & (p < n)).all():
            return p


def blur_rows(img, taps):
    h, cols = len(taps) // 2, img.shape[1]
    P = img[:, reflect101(np.arange(-h, cols + h), cols)]
    acc = P[:, h:h + cols] * taps[h]
    for j in range(1, h + 1):
        acc = acc + taps[h + j] * (P[:, h + j:h + j + cols] + P[:, h - j:h - j + cols])
    return acc.astype(f32)


def blur(img, taps):
    """GaussianBlur(Size(), s, s) on CV_32F with the committed taps: rows into float32, then columns"""
    return np.ascontiguousarray(blur_rows(np.ascontiguousarray(blur_rows(img, taps).T), taps).T)


def octave_count(m):
    """cvRound(log(m) / log 2 - 2) + 1 decided in integers: the largest c with 2^(2 c + 1) <= m^2, or 0"""
    c = 0
    while (1 << (2 * (c + 1) + 1)) <= m * m:
        c += 1
    return c if (1 << (2 * c + 1)) <= m * m else 0


def octave_sizes(rows, cols):
    """(rows, cols) of every octave that is built, from the source size: the doubled image halved, while at least 11 either way"""
    r, c = 2 * rows, 2 * cols
    out = []
    for _ in range(octave_count(min(r, c))):
        if r < 2 * BORDER + 1 or c < 2 * BORDER + 1:
            break
        out.append((r, c))
        r, c = r // 2, c // 2
    return out


def base_image(g):
    up = resize_np.resize(g.astype(f32), (2 * g.shape[1], 2 * g.shape[0]), resize_np.LINEAR)
    return blur(up, TAPS[0])


def pyramid(g):
    """[(gauss 6 x rows x cols, dog 5 x rows x cols) for every octave]"""
    out = []
    sizes = octave_sizes(*g.shape)
    layer0 = base_image(g)
    for o in range(len(sizes)):
        G = [layer0]
        for i in range(1, LAYERS + 3):
            G.append(blur(G[-1], TAPS[i]))
        G = np.stack(G)
        assert G.shape[1:] == sizes[o]
        out.append((G, (G[1:] - G[:-1]).astype(f32)))
        layer0 = np.ascontiguousarray(G[LAYERS][0:2 * (sizes[o][0] // 2):2, 0:2 * (sizes[o][1] // 2):2])
    return out


# ---- 2: extrema and adjustLocalExtrema ----------------------------------------------------------------------------------------------------
def pre_threshold(params):
    return f32(np.floor(0.5 * params.contrast_threshold / LAYERS * 255.0))


def extrema(D, thr):
    """the starting pixels of one octave in scan order: (layer, r, c) int64 arrays"""
    n, rows, cols = D.shape
    if rows <= 2 * BORDER or cols <= 2 * BORDER:
        z = np.zeros(0, np.int64)
        return z, z, z
    out = []
    for l in range(1, LAYERS + 1):
        v = D[l, BORDER:rows - BORDER, BORDER:cols - BORDER]
        ge, le = np.ones(v.shape, bool), np.ones(v.shape, bool)
        for k in (l - 1, l, l + 1):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    w = D[k, BORDER + dr:rows - BORDER + dr, BORDER + dc:cols - BORDER + dc]
                    ge &= v >= w
                    le &= v <= w
        hit = (np.abs(v) > thr) & (((v > 0) & ge) | ((v < 0) & le))
        r, c = np.nonzero(hit)
        out.append((np.full(len(r), l, np.int64), r + BORDER, c + BORDER))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def solve3(A, b):
    """Matx_FastSolveOp<float, 3, 1> on arrays (A[i][j], b[i] float32 arrays): Cramer's rule; zeros where det(A) == 0 (Matx::solve)"""
    a = A
    with np.errstate(all="ignore"):
        d = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + \
            a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])
        ok = d != 0
        d = f32(1) / d
        x0 = d * (b[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2]) + a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]))
        x1 = d * (a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]))
        x2 = d * (a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0]) + b[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    z = f32(0)
    return np.where(ok, x0, z).astype(f32), np.where(ok, x1, z).astype(f32), np.where(ok, x2, z).astype(f32)


IMG_SCALE = f32(1.0) / f32(255)
DERIV_SCALE = IMG_SCALE * f32(0.5)
SECOND_SCALE = IMG_SCALE
CROSS_SCALE = IMG_SCALE * f32(0.25)
HUGE = f32(2147483647 // 3)


def _derivs(D, l, r, c):
    img = lambda dl, dr, dc: D[l + dl, r + dr, c + dc]      # noqa: E731
    dD = ((img(0, 0, 1) - img(0, 0, -1)) * DERIV_SCALE, (img(0, 1, 0) - img(0, -1, 0)) * DERIV_SCALE, (img(1, 0, 0) - img(-1, 0, 0)) * DERIV_SCALE)
    v2 = img(0, 0, 0) * f32(2)
    dxx = (img(0, 0, 1) + img(0, 0, -1) - v2) * SECOND_SCALE
    dyy = (img(0, 1, 0) + img(0, -1, 0) - v2) * SECOND_SCALE
    dss = (img(1, 0, 0) + img(-1, 0, 0) - v2) * SECOND_SCALE
    dxy = (img(0, 1, 1) - img(0, 1, -1) - img(0, -1, 1) + img(0, -1, -1)) * CROSS_SCALE
    dxs = (img(1, 0, 1) - img(1, 0, -1) - img(-1, 0, 1) + img(-1, 0, -1)) * CROSS_SCALE
    dys = (img(1, 1, 0) - img(1, -1, 0) - img(-1, 1, 0) + img(-1, -1, 0)) * CROSS_SCALE
    return dD, (dxx, dyy, dss, dxy, dxs, dys)


def adjust(D, l, r, c, params, counters):
    """adjustLocalExtrema on every starting pixel of one octave at once.  Returns the survivors in the given order: dict of arrays
    (start index, layer, r, c, xi, xr, xc, contr)"""
    rows, cols = D.shape[1:]
    n = len(l)
    l, r, c = l.copy(), r.copy(), c.copy()
    l0, r0, c0 = l.copy(), r.copy(), c.copy()
    alive, done = np.ones(n, bool), np.zeros(n, bool)
    xi, xr, xc = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    for _ in range(MAX_STEPS):
        act = np.nonzero(alive & ~done)[0]
        if not len(act):
            break
        dD, (dxx, dyy, dss, dxy, dxs, dys) = _derivs(D, l[act], r[act], c[act])
        X = solve3(((dxx, dxy, dxs), (dxy, dyy, dys), (dxs, dys, dss)), dD)
        a_xc, a_xr, a_xi = -X[0], -X[1], -X[2]
        xi[act], xr[act], xc[act] = a_xi, a_xr, a_xc
        with np.errstate(all="ignore"):
            conv = (np.abs(a_xi) < f32(0.5)) & (np.abs(a_xr) < f32(0.5)) & (np.abs(a_xc) < f32(0.5))
            huge = ~conv & ((np.abs(a_xi) > HUGE) | (np.abs(a_xr) > HUGE) | (np.abs(a_xc) > HUGE))
        done[act[conv]] = True
        alive[act[huge]] = False
        counters["rej_huge"] += int(huge.sum())
        mv = act[~conv & ~huge]
        m = ~conv & ~huge
        with np.errstate(all="ignore"):
            c[mv] += np.rint(a_xc[m]).astype(np.int64)
            r[mv] += np.rint(a_xr[m]).astype(np.int64)
            l[mv] += np.rint(a_xi[m]).astype(np.int64)
        out = (l[mv] < 1) | (l[mv] > LAYERS) | (c[mv] < BORDER) | (c[mv] >= cols - BORDER) | (r[mv] < BORDER) | (r[mv] >= rows - BORDER)
        alive[mv[out]] = False
        counters["rej_left"] += int(out.sum())
    late = alive & ~done
    counters["rej_steps"] += int(late.sum())
    alive &= done
    s = np.nonzero(alive)[0]
    counters["moved_layer"] += int((l[s] != l0[s]).sum())
    counters["moved_pixel"] += int(((r[s] != r0[s]) | (c[s] != c0[s])).sum())
    dD, (dxx, dyy, dss, dxy, dxs, dys) = _derivs(D, l[s], r[s], c[s])
    t = dD[0] * xc[s] + dD[1] * xr[s] + dD[2] * xi[s]
    contr = D[l[s], r[s], c[s]] * IMG_SCALE + t * f32(0.5)
    ct, et = f32(params.contrast_threshold), f32(params.edge_threshold)
    low = np.abs(contr) * f32(LAYERS) < ct
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    with np.errstate(all="ignore"):
        edge = ~low & ((det <= 0) | (tr * tr * et >= (et + f32(1)) * (et + f32(1)) * det))
    counters["rej_contrast"] += int(low.sum())
    counters["rej_edge"] += int(edge.sum())
    k = ~low & ~edge
    s = s[k]
    return dict(start=s, layer=l[s], r=r[s], c=c[s], xi=xi[s], xr=xr[s], xc=xc[s], contr=contr[k].astype(f32), moved_layer=l[s] != l0[s],
                moved_pixel=(r[s] != r0[s]) | (c[s] != c0[s]))


def new_counters():
    return dict(extrema=0, rej_huge=0, rej_left=0, rej_steps=0, rej_contrast=0, rej_edge=0, moved_layer=0, moved_pixel=0, duplicates=0, dropped=0)


def candidates(pyr, params, counters=None):
    """every candidate in scan order, duplicates removed: dict of arrays - octave, layer, r, c (final), x, y, size (before the halving),
    response - and the status"""
    counters = new_counters() if counters is None else counters
    thr = pre_threshold(params)
    cols = dict(octave=[], layer=[], r=[], c=[], x=[], y=[], size=[], response=[])
    for o, (G, D) in enumerate(pyr):
        l, r, c = extrema(D, thr)
        counters["extrema"] += len(l)
        a = adjust(D, l, r, c, params, counters)
        two_o = f32(1 << o)
        cols["octave"].append(np.full(len(a["layer"]), o, np.int64))
        cols["layer"].append(a["layer"]); cols["r"].append(a["r"]); cols["c"].append(a["c"])
        cols["x"].append(((a["c"].astype(f32) + a["xc"]) * two_o).astype(f32))
        cols["y"].append(((a["r"].astype(f32) + a["xr"]) * two_o).astype(f32))
        p = exp2f(((a["layer"].astype(f32) + a["xi"]) / f32(LAYERS)).astype(f32))
        cols["size"].append((f32(SIGMA) * p * two_o * f32(2)).astype(f32))
        cols["response"].append(np.abs(a["contr"]).astype(f32))
    C = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    for k in ("octave", "layer", "r", "c"):
        C[k] = C[k].astype(np.int64)
    for k in ("x", "y", "size", "response"):
        C[k] = C[k].astype(f32)
    status = 0
    n = len(C["octave"])
    if n > MAX_CANDIDATES:
        counters["dropped"] = n - MAX_CANDIDATES
        C = {k: v[:MAX_CANDIDATES] for k, v in C.items()}
        status = STATUS_CANDIDATES
    key = ((C["octave"] * 4 + C["layer"]) << 32) | (C["r"] << 16) | C["c"]
    _, first = np.unique(key, return_index=True)
    keep = np.zeros(len(key), bool)
    keep[first] = True
    counters["duplicates"] += int((~keep).sum())
    C = {k: v[keep] for k, v in C.items()}
    return C, status, counters


def order(C):
    """the permutation that sorts by response, size, octave, pt.y, pt.x descending, then by scan index ascending"""
    n = len(C["octave"])
    return np.lexsort((np.arange(n), -C["x"].astype(f64), -C["y"].astype(f64), -C["octave"], -C["size"].astype(f64), -C["response"].astype(f64)))


# ---- 3: orientation ----------------------------------------------------------------------------------------------------------------------
def atan2deg(y, x):
    a = (polar_np.atan2f(y, x) * DEG_F).astype(f32)
    a = np.where(a < 0, a + f32(360), a).astype(f32)
    return np.where(a >= 360, a - f32(360), a).astype(f32)


def sum_in_order(nbins, bins, vals):
    """out[b] = the float32 sum of vals[k] over the k with bins[k] == b, in the order of k"""
    out = np.zeros(nbins, f32)
    np.add.at(out, bins, vals.astype(f32))
    return out


def orientations(img, r, c, scl):
    """calcOrientationHist and the peaks at (c, r) of a Gaussian layer: the angles in bin order, float32"""
    rows, cols = img.shape
    radius = cv_round(f32(4.5) * scl)
    assert radius <= ORI_RADIUS_MAX
    sigma = f32(1.5) * scl
    expf_scale = f32(-1) / (f32(2) * sigma * sigma)
    i, j = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    i, j = i.ravel(), j.ravel()
    y, x = r + i, c + j
    ok = (y > 0) & (y < rows - 1) & (x > 0) & (x < cols - 1)
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    w = expf((i * i + j * j).astype(f32) * expf_scale)
    ori = atan2deg(dy, dx)
    mag = np.sqrt(dx * dx + dy * dy).astype(f32)
    b = np.rint(f32(ORI_BINS / 360.0) * ori).astype(np.int64)
    b = np.where(b >= ORI_BINS, b - ORI_BINS, b)
    b = np.where(b < 0, b + ORI_BINS, b)
    t = sum_in_order(ORI_BINS, b, w * mag)
    h = ((np.roll(t, 2) + np.roll(t, -2)) * f32(1.0 / 16) + (np.roll(t, 1) + np.roll(t, -1)) * f32(4.0 / 16) + t * f32(6.0 / 16)).astype(f32)
    thr = h.max() * f32(0.8)
    out = []
    for k in range(ORI_BINS):
        lf, rt = h[(k - 1) % ORI_BINS], h[(k + 1) % ORI_BINS]
        if h[k] > lf and h[k] > rt and h[k] >= thr:
            b_ = f32(k) + f32(0.5) * (lf - rt) / (lf - f32(2) * h[k] + rt)
            b_ = f32(ORI_BINS) + b_ if b_ < 0 else (b_ - f32(ORI_BINS) if b_ >= ORI_BINS else b_)
            ang = f32(360) - f32(10) * b_
            if abs(ang - f32(360)) < FLT_EPSILON:
                ang = f32(0)
            out.append(f32(ang))
    return out


# ---- 4: descriptor -----------------------------------------------------------------------------------------------------------------------
def descriptor(img, ptx, pty, angle, scl):
    """calcSIFTDescriptor at (ptx, pty) of a Gaussian layer, for the keypoint angle `angle`: 128 float32"""
    rows, cols = img.shape
    d, n = 4, 8
    ori = f32(360) - f32(angle)
    if abs(ori - f32(360)) < FLT_EPSILON:
        ori = f32(0)
    px, py = cv_round(f32(ptx)), cv_round(f32(pty))
    sn, cs = polar_np.sincosf(f32(ori * RAD_F))
    cos_t, sin_t = f32(cs), f32(sn)
    bins_per_rad = f32(n / 360.0)
    exp_scale = f32(-1) / f32(d * d * 0.5)
    hist_width = f32(3) * f32(scl)
    radius = cv_round(hist_width * f32(1.4142135623730951) * f32(d + 1) * f32(0.5))
    radius = min(radius, int(np.sqrt(float(cols) * cols + float(rows) * rows)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    i, j = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    i, j = i.ravel(), j.ravel()
    fi, fj = i.astype(f32), j.astype(f32)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin = r_rot + f32(d // 2) - f32(0.5)
    cbin = c_rot + f32(d // 2) - f32(0.5)
    r, c = py + i, px + j
    ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
    r, c, rbin, cbin, r_rot, c_rot = r[ok], c[ok], rbin[ok], cbin[ok], r_rot[ok], c_rot[ok]
    dx = img[r, c + 1] - img[r, c - 1]
    dy = img[r - 1, c] - img[r + 1, c]
    w = expf((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    obin = (atan2deg(dy, dx) - ori) * bins_per_rad
    mag = np.sqrt(dx * dx + dy * dy).astype(f32) * w
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + n, o0)
    o0 = np.where(o0 >= n, o0 - n, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    v111 = v_rc11 * obin
    v110 = v_rc11 - v111
    v101 = v_rc10 * obin
    v100 = v_rc10 - v101
    v011 = v_rc01 * obin
    v010 = v_rc01 - v011
    v001 = v_rc00 * obin
    v000 = v_rc00 - v001
    idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
    offs = np.array([0, 1, n + 2, n + 3, (d + 2) * (n + 2), (d + 2) * (n + 2) + 1, (d + 3) * (n + 2), (d + 3) * (n + 2) + 1])
    vals = np.stack([v000, v001, v010, v011, v100, v101, v110, v111], axis=1).astype(f32)
    hist = sum_in_order((d + 2) * (d + 2) * (n + 2), (idx[:, None] + offs[None, :]).ravel(), vals.ravel()).reshape(d + 2, d + 2, n + 2)
    hist[:, :, 0] += hist[:, :, n]
    hist[:, :, 1] += hist[:, :, n + 1]
    dst = hist[1:d + 1, 1:d + 1, :n].reshape(d * d * n).astype(f32)
    nrm2 = np.add.accumulate(np.concatenate(([f32(0)], dst * dst)), dtype=f32)[-1]
    thr = np.sqrt(nrm2) * f32(0.2)
    dst = np.minimum(dst, thr)
    nrm2 = np.add.accumulate(np.concatenate(([f32(0)], dst * dst)), dtype=f32)[-1]
    scale = f32(512) / max(np.sqrt(nrm2), FLT_EPSILON)
    return np.clip(np.rint(dst * scale), 0, 255).astype(f32)


# ---- the whole entry ---------------------------------------------------------------------------------------------------------------------
def find(image, params=None, cap=None, trace=None):
    """isx_sift_find: dict(count, status, keypoints n x 2, meta n x 5 (size, angle, response, octave, layer), descriptors n x 128).
    `trace`, a dict, receives the counters, the ranked candidates and the keypoints of every candidate."""
    params = params or Params()
    g = gray(image)
    pyr = pyramid(g)
    C, status, counters = candidates(pyr, params)
    perm = order(C)
    limit = None if params.nfeatures <= 0 else params.nfeatures
    kp, meta, desc, per_cand = [], [], [], []
    total = 0
    for q in perm:
        o, l, r, c = (int(C[k][q]) for k in ("octave", "layer", "r", "c"))
        x, y, size, resp = C["x"][q], C["y"][q], C["size"][q], C["response"][q]
        two_o = f32(1 << o)
        scl = f32(size * f32(0.5) / two_o)
        angles = orientations(pyr[o][0][l], r, c, scl)
        per_cand.append(len(angles))
        for ang in angles:
            total += 1
            if limit is not None and total > limit:
                break
            if cap is not None and total > cap:
                break
            kp.append((x * f32(0.5), y * f32(0.5)))
            meta.append((size * f32(0.5), ang, resp, f32(o - 1), f32(l)))
            desc.append(descriptor(pyr[o][0][l], f32(x / two_o), f32(y / two_o), ang, scl))
        if (limit is not None and total >= limit) or (cap is not None and total > cap):
            break
    if limit is not None:
        total = min(total, limit)
    if cap is not None and total > cap:
        status |= STATUS_TRUNCATED
        total = cap
    n = len(kp)
    assert n == total
    if trace is not None:
        trace.update(counters=counters, candidates={k: v[perm] for k, v in C.items()}, peaks=per_cand, octaves=[p[0].shape[1:] for p in pyr])
    return dict(count=n, status=status, keypoints=np.array(kp, f32).reshape(n, 2), meta=np.array(meta, f32).reshape(n, 5),
                descriptors=np.array(desc, f32).reshape(n, 128))

