"""NumPy model of isx_surf_find: cv::detail::SurfFeaturesFinder as OpenCV 3.4.2 defines it (stitching/src/matchers.cpp on
xfeatures2d/src/surf.cpp; neither is in the reference tree, so OpenCV parity is UNPINNED): the standard of record (DESIGN.md §8 "Features
finder, SURF").  Integers in int64 / wrapping uint32, floats one rounded operation at a time in the order written here.

Decisions (the GPU is held to this file bit for bit):
  * the integral image is unsigned 32-bit with wrapping adds; a box difference is read as a signed 32-bit integer
  * the maxima are ordered by KeypointGreater (response, size, octave, pt.y, pt.x, all descending) and then by their scan index
    (octave, layer, i, j) ascending; of more than MAX_CANDIDATES maxima the first in scan order are ranked (STATUS_CANDIDATES)
  * angles are polar_np.atan2f in degrees wrapped to [0, 360), not fastAtan2; sin and cos are polar_np.sincosf
  * the rotated window is walked as OpenCV accumulates it: rows in float32, columns in double
  * the 21 x 21 patch is OpenCV's general resizeArea_ table for every window size (no integer-mean branch)
  * G13 and G20 are committed float32 bit patterns; gaussian_kernel regenerates them
"""
import numpy as np

from . import polar_np

f32 = np.float32
f64 = np.float64

MAX_CANDIDATES, MAX_SIDE, MAX_PIXELS = 32768, 16384, 1 << 24      # ISX_SURF_MAX_CANDIDATES, ISX_SURF_MAX_SIDE, ISX_SURF_MAX_PIXELS
STATUS_TRUNCATED, STATUS_CANDIDATES = 1, 2                         # ISX_SURF_TRUNCATED, ISX_SURF_CANDIDATES_DROPPED
HAAR_SIZE0, HAAR_SIZE_INC = 9, 6
ORI_RADIUS, ORI_WIN, ORI_STEP, PATCH_SZ = 6, 60, 5, 20
DX_BOXES = ((0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1))
DY_BOXES = ((2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1))
DXY_BOXES = ((1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1))
ORI_DX_BOXES = ((0, 0, 2, 4, -1), (2, 0, 4, 4, 1))
ORI_DY_BOXES = ((0, 0, 4, 2, 1), (0, 2, 4, 4, -1))

G13 = np.array([0x3c1413a5, 0x3cb27fc3, 0x3d375b73, 0x3da07fcc, 0x3def6fcb, 0x3e18311c, 0x3e24de12, 0x3e18311c, 0x3def6fcb, 0x3da07fcc, 0x3d375b73,
                0x3cb27fc3, 0x3c1413a5], np.uint32).view(f32)
G20 = np.array([0x3afbf6b2, 0x3b8ff21f, 0x3c160a7e, 0x3c8eac33, 0x3cf786bf, 0x3d43e181, 0x3d8d6929, 0x3dba42ec, 0x3ddfcfd7, 0x3df5564c, 0x3df5564c,
                0x3ddfcfd7, 0x3dba42ec, 0x3d8d6929, 0x3d43e181, 0x3cf786bf, 0x3c8eac33, 0x3c160a7e, 0x3b8ff21f, 0x3afbf6b2], np.uint32).view(f32)
# the 113 points of the disc i * i + j * j <= 36, row-major over i then j
ORI_POINTS = [(i, j) for i in range(-ORI_RADIUS, ORI_RADIUS + 1) for j in range(-ORI_RADIUS, ORI_RADIUS + 1) if i * i + j * j <= ORI_RADIUS * ORI_RADIUS]
RAD_F = f32(np.pi / 180.0)
DEG_F = f32(180.0 / np.pi)


def gaussian_kernel(n, sigma):
    """getGaussianKernel(n, sigma, CV_32F) for the sizes that take the formula: exp in double, rounded to float, normalised by the double
    sum of the rounded values"""
    cf = np.zeros(n, f32)
    total = 0.0
    scale2x = -0.5 / (sigma * sigma)
    for i in range(n):
        x = i - (n - 1) * 0.5
        cf[i] = f32(np.exp(scale2x * x * x))
        total += float(cf[i])
    inv = 1.0 / total
    return np.array([f32(float(v) * inv) for v in cf], f32)


class Params:
    def __init__(self, hess_thresh=300.0, num_octaves=3, num_layers=4):
        self.hess_thresh, self.num_octaves, self.num_layers = float(hess_thresh), int(num_octaves), int(num_layers)


def cv_round(v):
    return int(np.rint(v))


# ---- 1, 2: gray and the integral image ----------------------------------------------------------------------------------------------
def gray(image):
    img = np.asarray(image)
    if img.ndim == 2 or img.shape[2] == 1:
        return np.ascontiguousarray(img.reshape(img.shape[0], img.shape[1]).astype(np.uint8))
    c = img.astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def integral(g):
    """(rows + 1) x (cols + 1) uint32, wrapping"""
    s = np.zeros((g.shape[0] + 1, g.shape[1] + 1), np.uint64)
    s[1:, 1:] = np.cumsum(np.cumsum(g.astype(np.uint64), axis=0), axis=1)
    return (s & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- 3: fast Hessian -------------------------------------------------------------------------------------------------------------------
def layer_size(o, l):
    return (HAAR_SIZE0 + HAAR_SIZE_INC * l) << o


def resize_haar(boxes, old_size, new_size):
    """resizeHaarPattern: [(x1, y1, x2, y2, w float32)]"""
    ratio = f32(f32(new_size) / f32(old_size))
    out = []
    for x1, y1, x2, y2, w in boxes:
        a, b, c, d = (cv_round(f32(ratio * f32(v))) for v in (x1, y1, x2, y2))
        out.append((a, b, c, d, f32(f32(w) / f32(f32(c - a) * f32(d - b)))))
    return out


def haar_response(S, boxes, ys, xs):
    """calcHaarPattern at the origins ys x xs (index arrays): float32"""
    d = np.zeros((len(ys), len(xs)), f64)
    for x1, y1, x2, y2, w in boxes:
        p0, p1 = S[np.ix_(ys + y1, xs + x1)], S[np.ix_(ys + y2, xs + x1)]
        p2, p3 = S[np.ix_(ys + y1, xs + x2)], S[np.ix_(ys + y2, xs + x2)]
        diff = (p0 + p3 - p1 - p2).view(np.int32)
        d = d + (diff.astype(f32) * w).astype(f64)
    return d.astype(f32)


def haar_points(S, boxes, ys, xs):
    """calcHaarPattern at the origins (ys[k], xs[k]): float32"""
    d = np.zeros(len(ys), f64)
    for x1, y1, x2, y2, w in boxes:
        diff = (S[ys + y1, xs + x1] + S[ys + y2, xs + x2] - S[ys + y2, xs + x1] - S[ys + y1, xs + x2]).view(np.int32)
        d = d + (diff.astype(f32) * w).astype(f64)
    return d.astype(f32)


def det_trace(S, rows, cols, o, l):
    """the det and trace maps of layer l of octave o, or None where the filter does not fit"""
    size, step = layer_size(o, l), 1 << o
    if size > rows or size > cols:
        return None
    det = np.zeros((rows // step, cols // step), f32)
    trace = np.zeros_like(det)
    ni, nj = 1 + (rows - size) // step, 1 + (cols - size) // step
    margin = (size // 2) // step
    ys, xs = np.arange(ni) * step, np.arange(nj) * step
    dx = haar_response(S, resize_haar(DX_BOXES, 9, size), ys, xs)
    dy = haar_response(S, resize_haar(DY_BOXES, 9, size), ys, xs)
    dxy = haar_response(S, resize_haar(DXY_BOXES, 9, size), ys, xs)
    det[margin:margin + ni, margin:margin + nj] = dx * dy - f32(0.81) * dxy * dxy
    trace[margin:margin + ni, margin:margin + nj] = dx + dy
    return det, trace


# ---- 4: maxima -------------------------------------------------------------------------------------------------------------------------
def fast_solve3(A, b):
    """Matx_FastSolveOp<float, 3, 1>: Cramer's rule in float32, None when det(A) == 0"""
    a = [[f32(v) for v in r] for r in A]
    b = [f32(v) for v in b]
    d = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + \
        a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])
    if d == 0:
        return None
    d = f32(1) / d
    x0 = d * (b[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2]) + a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]))
    x1 = d * (a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]))
    x2 = d * (a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0]) + b[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    return x0, x1, x2


def interpolate(N0, N1, N2, step, ds, pt_x, pt_y, size):
    """interpolateKeypoint on the three 3 x 3 neighbourhoods (flat, row-major): (pt.x, pt.y, size) or None"""
    two, four = f32(2), f32(4)
    b = (-(N1[5] - N1[3]) / two, -(N1[7] - N1[1]) / two, -(N2[4] - N0[4]) / two)
    a01 = (N1[8] - N1[6] - N1[2] + N1[0]) / four
    a02 = (N2[5] - N2[3] - N0[5] + N0[3]) / four
    a12 = (N2[7] - N2[1] - N0[7] + N0[1]) / four
    A = ((N1[3] - two * N1[4] + N1[5], a01, a02), (a01, N1[1] - two * N1[4] + N1[7], a12), (a02, a12, N0[4] - two * N1[4] + N2[4]))
    with np.errstate(all="ignore"):
        x = fast_solve3(A, b)
    if x is None:
        return None
    ok = (x[0] != 0 or x[1] != 0 or x[2] != 0) and abs(x[0]) <= 1 and abs(x[1]) <= 1 and abs(x[2]) <= 1
    if not ok:
        return None
    return f32(pt_x + x[0] * f32(step)), f32(pt_y + x[1] * f32(step)), f32(np.rint(f32(size) + x[2] * f32(ds)))


def find_maxima(S, rows, cols, params):
    """every accepted candidate in scan order (octave, layer, i, j): rows of (pt.x, pt.y, size, response, octave, laplacian) float32"""
    thresh = f32(params.hess_thresh)
    out = []
    for o in range(params.num_octaves):
        step = 1 << o
        maps = [det_trace(S, rows, cols, o, l) for l in range(params.num_layers + 2)]
        for l in range(1, params.num_layers + 1):
            if maps[l - 1] is None or maps[l] is None or maps[l + 1] is None:
                continue
            size = layer_size(o, l)
            R, C = rows // step, cols // step
            m = (layer_size(o, l + 1) // 2) // step + 1
            if R - 2 * m <= 0 or C - 2 * m <= 0:
                continue
            D = [maps[l - 1][0], maps[l][0], maps[l + 1][0]]
            c = D[1][m:R - m, m:C - m]
            keep = c > thresh
            for k in range(3):
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        if k == 1 and di == 0 and dj == 0:
                            continue
                        keep &= c > D[k][m + di:R - m + di, m + dj:C - m + dj]
            for i, j in zip(*np.nonzero(keep)):
                i, j = int(i) + m, int(j) + m
                N = [D[k][i - 1:i + 2, j - 1:j + 2].reshape(9) for k in range(3)]
                half = (size // 2) // step
                sum_i, sum_j = step * (i - half), step * (j - half)
                cx, cy = f32(f32(sum_j) + f32(size - 1) * f32(0.5)), f32(f32(sum_i) + f32(size - 1) * f32(0.5))
                got = interpolate(N[0], N[1], N[2], step, size - layer_size(o, l - 1), cx, cy, size)
                if got is None:
                    continue
                tr = maps[l][1][i, j]
                lap = 1.0 if tr > 0 else (-1.0 if tr < 0 else 0.0)
                out.append((got[0], got[1], got[2], D[1][i, j], f32(o), f32(lap)))
    return np.array(out, f32).reshape(-1, 6)


# ---- 5: order --------------------------------------------------------------------------------------------------------------------------
def order(cands):
    """the permutation that sorts by response, size, octave, pt.y, pt.x descending, then by scan index ascending"""
    n = len(cands)
    return sorted(range(n), key=lambda i: (-cands[i, 3], -cands[i, 2], -cands[i, 4], -cands[i, 1], -cands[i, 0], i))


# ---- 6: orientation --------------------------------------------------------------------------------------------------------------------
def atan2deg(y, x):
    a = f32(polar_np.atan2f(f32(y), f32(x)) * DEG_F)
    if a < 0:
        a = f32(a + f32(360))
    if a >= 360:
        a = f32(a - f32(360))
    return a


def scale_of(size):
    return f32(f32(f32(size) * f32(1.2)) / f32(9.0))


def orientation(S, rows, cols, pt_x, pt_y, size):
    """the angle in degrees, or None where the keypoint is removed"""
    s = scale_of(size)
    g = 2 * cv_round(f32(f32(2) * s))
    if rows + 1 < g or cols + 1 < g:
        return None
    half = f32(f32(g - 1) / f32(2))
    dxb, dyb = resize_haar(ORI_DX_BOXES, 4, g), resize_haar(ORI_DY_BOXES, 4, g)
    pj, pi = np.array([q[1] for q in ORI_POINTS]), np.array([q[0] for q in ORI_POINTS])
    xs = np.rint((f32(pt_x) + pj.astype(f32) * s) - half).astype(np.int64)
    ys = np.rint((f32(pt_y) + pi.astype(f32) * s) - half).astype(np.int64)
    use = (ys >= 0) & (ys < rows + 1 - g) & (xs >= 0) & (xs < cols + 1 - g)
    if not use.any():
        return None
    xs, ys, w = xs[use], ys[use], (G13[pi + ORI_RADIUS] * G13[pj + ORI_RADIUS])[use]
    X, Y = haar_points(S, dxb, ys, xs) * w, haar_points(S, dyb, ys, xs) * w
    ang = polar_np.atan2f(Y, X) * DEG_F
    ang = np.where(ang < 0, ang + f32(360), ang)
    ang = np.where(ang >= 360, ang - f32(360), ang).astype(f32)
    ai = np.rint(np.array(ang, f32)).astype(np.int64)
    best, bx, by = f32(0), f32(0), f32(0)
    for a in range(0, 360, ORI_STEP):
        d = np.abs(ai - a)
        use = (d < ORI_WIN // 2) | (d > 360 - ORI_WIN // 2)
        sx = np.add.accumulate(np.concatenate(([f32(0)], np.where(use, X, f32(0)))), dtype=f32)[-1]
        sy = np.add.accumulate(np.concatenate(([f32(0)], np.where(use, Y, f32(0)))), dtype=f32)[-1]
        mod = f32(f32(sx * sx) + f32(sy * sy))
        if mod > best:
            best, bx, by = mod, sx, sy
    return atan2deg(-by, bx)


# ---- 7: descriptor ---------------------------------------------------------------------------------------------------------------------
def area_tab(ssize, dsize):
    """computeResizeAreaTab for one channel: per destination cell the list of (source index, float32 weight)"""
    scale = float(ssize) / dsize
    tab = []
    for d in range(dsize):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        row = []
        if sx1 - fsx1 > 1e-3:
            row.append((sx1 - 1, f32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            row.append((sx, f32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            row.append((sx2, f32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        tab.append(row)
    return tab


def window(g, pt_x, pt_y, size, angle):
    """the win x win rotated window, uint8"""
    rows, cols = g.shape
    s = scale_of(size)
    win = int(f32(f32(PATCH_SZ + 1) * s))
    sn, cs = polar_np.sincosf(f32(f32(angle) * RAD_F))
    sin_dir, cos_dir = f32(-f32(sn)), f32(cs)
    off = f32(-f32(win - 1) / f32(2))
    start_x = f32(f32(f32(pt_x) + f32(off * cos_dir)) + f32(off * sin_dir))
    start_y = f32(f32(f32(pt_y) - f32(off * sin_dir)) + f32(off * cos_dir))
    row_x = np.add.accumulate(np.concatenate(([start_x], np.full(win - 1, sin_dir, f32))), dtype=f32)
    row_y = np.add.accumulate(np.concatenate(([start_y], np.full(win - 1, cos_dir, f32))), dtype=f32)
    px = np.add.accumulate(np.concatenate((row_x.astype(f64)[:, None], np.full((win, win - 1), f64(cos_dir))), axis=1), axis=1)
    py = np.add.accumulate(np.concatenate((row_y.astype(f64)[:, None], np.full((win, win - 1), -f64(sin_dir))), axis=1), axis=1)
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    inside = (ix >= 0) & (ix < cols - 1) & (iy >= 0) & (iy < rows - 1)
    cx, cy = np.clip(ix, 0, max(cols - 2, 0)), np.clip(iy, 0, max(rows - 2, 0))
    a, b = (px - ix).astype(f32), (py - iy).astype(f32)
    one = f32(1)
    if rows >= 2 and cols >= 2:
        p00, p01, p10, p11 = (g[cy + v, cx + u].astype(f32) for v, u in ((0, 0), (0, 1), (1, 0), (1, 1)))
        lin = np.rint(p00 * (one - a) * (one - b) + p01 * a * (one - b) + p10 * (one - a) * b + p11 * a * b).astype(np.int64).astype(np.uint8)
    else:
        lin = np.zeros((win, win), np.uint8)
    nx = np.clip(np.rint(px).astype(np.int64), 0, cols - 1)
    ny = np.clip(np.rint(py).astype(np.int64), 0, rows - 1)
    return np.where(inside, lin, g[ny, nx])


def patch_of(W):
    """resize(win, PATCH, INTER_AREA) by the general table: 21 x 21 uint8"""
    win, n = W.shape[0], PATCH_SZ + 1
    tab = area_tab(win, n)
    Wf = W.astype(f32)
    buf = np.zeros((win, n), f32)
    for d, row in enumerate(tab):
        for k, (sx, alpha) in enumerate(row):
            buf[:, d] = Wf[:, sx] * alpha if k == 0 else buf[:, d] + Wf[:, sx] * alpha
    out = np.zeros((n, n), f32)
    for d, row in enumerate(tab):
        for k, (sy, beta) in enumerate(row):
            out[d] = buf[sy] * beta if k == 0 else out[d] + buf[sy] * beta
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def descriptor(g, pt_x, pt_y, size, angle):
    P = patch_of(window(g, pt_x, pt_y, size, angle)).astype(np.int64)
    DW = np.outer(G20, G20).astype(f32)                       # float32 products
    dx = (P[:-1, 1:] - P[:-1, :-1] + P[1:, 1:] - P[1:, :-1]).astype(f32) * DW
    dy = (P[1:, :-1] - P[:-1, :-1] + P[1:, 1:] - P[:-1, 1:]).astype(f32) * DW
    def cells(v):                                             # 4 x 4 cells of 5 x 5, each summed in y, x order
        return np.add.accumulate(v.reshape(4, 5, 4, 5).transpose(0, 2, 1, 3).reshape(4, 4, 25), axis=2, dtype=f32)[:, :, -1]
    vec = np.stack((cells(dx), cells(dy), cells(np.abs(dx)), cells(np.abs(dy))), axis=2).reshape(64).astype(f32)
    mag = 0.0
    for v in vec:
        mag += float(f32(v * v))
    scale = f32(1.0 / (np.sqrt(mag) + float(np.finfo(f32).eps)))
    return vec * scale


# ---- the whole entry -------------------------------------------------------------------------------------------------------------------
def detect(image, params=None):
    """steps 1 - 5: (gray, S, ranked candidates n x 6, status)"""
    params = params or Params()
    g = gray(image)
    rows, cols = g.shape
    S = integral(g)
    cands = find_maxima(S, rows, cols, params)
    status = 0
    if len(cands) > MAX_CANDIDATES:
        cands, status = cands[:MAX_CANDIDATES], STATUS_CANDIDATES
    return g, S, cands[order(cands)], status


def finish(g, S, cands, status, cap=None):
    """steps 6 - 8 on ranked candidates (rows of pt.x, pt.y, size, response, octave, laplacian)"""
    rows, cols = g.shape
    kp, meta, desc = [], [], []
    for c in cands:
        ang = orientation(S, rows, cols, c[0], c[1], c[2])
        if ang is None:
            continue
        if cap is not None and len(kp) >= cap:
            status |= STATUS_TRUNCATED
            break
        kp.append((c[0], c[1]))
        meta.append((c[2], ang, c[3], c[4], c[5]))
        desc.append(descriptor(g, c[0], c[1], c[2], ang))
    n = len(kp)
    return dict(count=n, status=status, keypoints=np.array(kp, f32).reshape(n, 2), meta=np.array(meta, f32).reshape(n, 5),
                descriptors=np.array(desc, f32).reshape(n, 64))


def find(image, params=None, cap=None):
    """isx_surf_find: dict(count, status, keypoints n x 2, meta n x 5 (size, angle, response, octave, laplacian), descriptors n x 64)"""
    g, S, cands, status = detect(image, params)
    return finish(g, S, cands, status, cap)
