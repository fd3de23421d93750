"""NumPy model of isx_orb_find: the reference's OrbFeaturesFinder (F = its 特征点检测 demo, find F:948-1017, detectAndCompute F:727-946,
computeKeyPoints F:56-191, HarrisResponses F:204-246, ICAngles F:250-283, computeOrbDescriptors F:287-353): the standard of record
(DESIGN.md §8 "Features finder").  Integers in int64, floats one rounded float32 operation at a time, in the order F writes them.

Decisions (the GPU is held to this file bit for bit; none of them is OpenCV's own text):
  * the pyramid is resize_np.resize(INTER_LINEAR) on uint8, level l from level l - 1 (F:834 asks for INTER_LINEAR_EXACT)
  * no border is built: every reader stays inside its layer (READER_REACH < EDGE)
  * FAST-9/16 with non-max suppression is restated from its definition; score = max(a, -b) - 1
  * the angle is polar_np.atan2f in degrees, wrapped to [0, 360), not fastAtan2; cos and sin are polar_np.sincosf
  * the 7 x 7, sigma 2 blur runs in exact integers on the Q8 taps BLUR_TAPS
  * the sampling pattern is an input; the default is makeRandomPattern(31) (F:709-718) on the restated cv::RNG
  * the output is in canonical order: cell (row-major), level, y, x
  * the candidate set of the first cut and the final set of every (cell, level) have room for CAND_TIE_ROOM / KEEP_TIE_ROOM ties; points
    strictly above the cut always fit, ties fill the room in canonical order, a set that dropped ties sets STATUS_TRUNCATED
"""
import math

import numpy as np

from . import homography_np, polar_np, resize_np

f32 = np.float32

EDGE, PATCH, HALF_PATCH, HARRIS_BLOCK = 31, 31, 15, 7
CAND_TIE_ROOM, KEEP_TIE_ROOM = 256, 32          # ISX_ORB_CAND_TIE_ROOM, ISX_ORB_KEEP_TIE_ROOM
MAX_LEVELS, MAX_CANDIDATES = 8, 4096            # ISX_ORB_MAX_LEVELS, ISX_ORB_MAX_CANDIDATES
MAX_LAYERS, MAX_SIDE = 1024, 16384              # ISX_ORB_MAX_LAYERS, ISX_ORB_MAX_SIDE
STATUS_TRUNCATED, STATUS_BAD_PATTERN = 1, 2     # ISX_ORB_TRUNCATED, ISX_ORB_BAD_PATTERN
BLUR_TAPS = (18, 34, 49, 54, 49, 34, 18)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
          (-1, 3))
# how far from a keypoint each reader goes: FAST's circle, Harris (block 7 and the 3 x 3 derivative), the moment patch, the rotated pattern
# (|x|, |y| <= 15: 15 (|cos| + |sin|) <= 21.3, rounded) plus the blur's 3
READER_REACH = {"fast": 3, "nms": 4, "harris": HARRIS_BLOCK // 2 + 1, "moments": HALF_PATCH, "pattern": 22, "pattern+blur": 22 + 3}


class Params:
    def __init__(self, grid=(3, 1), n_features=1500, scale_factor=1.3, nlevels=5, fast_threshold=20):
        self.grid = (int(grid[0]), int(grid[1]))            # (width, height) as cv::Size
        self.n_features = int(n_features)
        self.scale_factor = float(f32(scale_factor))        # `double scaleFactor = 1.3f` (F:45)
        self.nlevels = int(nlevels)
        self.fast_threshold = int(fast_threshold)

    @property
    def per_cell(self):
        area = self.grid[0] * self.grid[1]
        return self.n_features * (99 + area) // 100 // area                     # F:43


# ---- the restated cv::RNG and makeRandomPattern (F:709-718) -------------------------------------------------------------------------
def default_pattern():
    """512 x 2 int32 (x, y): rng.uniform(-15, 16) for x, then for y, on the RNG the homography model restates (unpinned like it)"""
    rng = homography_np.RNG(0x34985739)
    out = np.zeros((512, 2), np.int32)
    for i in range(512):
        out[i, 0] = rng.uniform(-(PATCH // 2), PATCH // 2 + 1)
        out[i, 1] = rng.uniform(-(PATCH // 2), PATCH // 2 + 1)
    return out


def pattern_ok(pattern):
    p = np.asarray(pattern)
    return p.shape == (512, 2) and bool((np.abs(p.astype(np.int64)) <= HALF_PATCH).all())


# ---- host-side tables -----------------------------------------------------------------------------------------------------------------
def cv_round(v):
    """cvRound of a float32 / double: half to even"""
    return int(np.rint(v))


def features_per_level(nfeatures, scale_factor, nlevels):
    """F:72-82"""
    factor = f32(1.0 / scale_factor)
    nd = f32(f32(f32(nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels)))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(cv_round(nd))
        total += out[-1]
        nd = f32(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


def level_scales(scale_factor, nlevels):
    """getScale (F:721-724): (float)pow(scaleFactor, level)"""
    return [f32(math.pow(scale_factor, float(l))) for l in range(nlevels)]


def layer_size(w, h, scale):
    """F:794: cvRound(cols / scale), an int over a float"""
    return cv_round(f32(f32(w) / scale)), cv_round(f32(f32(h) / scale))


def umax_table():
    """F:88-103"""
    hp = HALF_PATCH
    umax = [0] * (hp + 2)
    half_sqrt2 = f32(f32(f32(hp) * np.sqrt(f32(2))) / f32(2))
    vmax = int(math.floor(f32(half_sqrt2 + f32(1))))
    vmin = int(math.ceil(half_sqrt2))
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(float(hp) * hp - v * v))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:hp + 1]


def cells_of(w, h, grid):
    """F:981-987: (xl, yl, xr, yr) per cell, rows outside"""
    gw, gh = grid
    return [(c * w // gw, r * h // gh, (c + 1) * w // gw, (r + 1) * h // gh) for r in range(gh) for c in range(gw)]


def capacity(params):
    """isx_orb_capacity: the rows the outputs need"""
    n = features_per_level(params.per_cell, params.scale_factor, params.nlevels)
    return params.grid[0] * params.grid[1] * sum(v + KEEP_TIE_ROOM for v in n)


# ---- pixels ---------------------------------------------------------------------------------------------------------------------------
def gray_of(image):
    a = np.asarray(image)
    assert a.dtype == np.uint8
    if a.ndim == 2 or a.shape[2] == 1:
        return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1]))
    assert a.shape[2] in (3, 4)
    b, g, r = (a[:, :, i].astype(np.int64) for i in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def pyramid(cell, scales):
    """the layers of one cell; a layer without pixels ends the pyramid"""
    layers = [np.ascontiguousarray(cell)]
    for l in range(1, len(scales)):
        w, h = layer_size(cell.shape[1], cell.shape[0], scales[l])
        if w <= 0 or h <= 0 or layers[-1] is None:
            layers.append(None)
            continue
        layers.append(resize_np.resize(layers[-1], (w, h), resize_np.LINEAR))
    return layers


def fast_scores(img, threshold):
    """the score map: max(a, -b) - 1 where it is >= threshold, else 0; 0 within 3 px of the edge"""
    h, w = img.shape
    out = np.zeros((h, w), np.int64)
    if h < 7 or w < 7:
        return out
    I = img.astype(np.int64)
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in CIRCLE])
    a = np.full(c.shape, -1 << 20, np.int64)
    b = np.full(c.shape, 1 << 20, np.int64)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(9)]]
        a = np.maximum(a, arc.min(axis=0))
        b = np.minimum(b, arc.max(axis=0))
    score = np.maximum(a, -b) - 1
    out[3:h - 3, 3:w - 3] = np.where(score >= threshold, score, 0)
    return out


def nms_keep(scores):
    """scores where a corner is strictly greater than its 8 neighbours and inside runByImageBorder(31), else 0"""
    h, w = scores.shape
    out = np.zeros_like(scores)
    if h <= 2 * EDGE or w <= 2 * EDGE:
        return out
    c = scores[EDGE:h - EDGE, EDGE:w - EDGE]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > scores[EDGE + dy:h - EDGE + dy, EDGE + dx:w - EDGE + dx]
    out[EDGE:h - EDGE, EDGE:w - EDGE] = np.where(keep, c, 0)
    return out


def retain_best(values, n, cap):
    """KeyPointsFilter::retainBest(n) on values in canonical order, with the capacity rule: (indices kept, truncated)"""
    v = np.asarray(values)
    order = np.argsort(v, kind="stable")
    s = v[order]
    gt = len(v) - np.searchsorted(s, v, side="right")                 # values strictly greater
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    eq_before = rank - np.searchsorted(s, v, side="left")             # equal values earlier in canonical order
    wanted = gt < n
    keep = wanted & (gt + eq_before < cap)
    return np.nonzero(keep)[0], bool((wanted & ~keep).any())


def harris_responses(img, xs, ys):
    """F:216-244 at the points (xs, ys): int sums over the 7 x 7 block, then the float32 expression"""
    I = img.astype(np.int64)
    h, w = I.shape
    ix = np.zeros((h, w), np.int64)
    iy = np.zeros((h, w), np.int64)
    ix[1:-1, 1:-1] = (I[1:-1, 2:] - I[1:-1, :-2]) * 2 + (I[:-2, 2:] - I[:-2, :-2]) + (I[2:, 2:] - I[2:, :-2])
    iy[1:-1, 1:-1] = (I[2:, 1:-1] - I[:-2, 1:-1]) * 2 + (I[2:, :-2] - I[:-2, :-2]) + (I[2:, 2:] - I[:-2, 2:])
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    r = HARRIS_BLOCK // 2

    def block_sums(m):
        s = np.zeros((h + 1, w + 1), np.int64)
        s[1:, 1:] = m.cumsum(0).cumsum(1)
        return s[ys + r + 1, xs + r + 1] - s[ys - r, xs + r + 1] - s[ys + r + 1, xs - r] + s[ys - r, xs - r]
    return harris_from_sums(block_sums(ix * ix), block_sums(iy * iy), block_sums(ix * iy))


def harris_response(img, x, y):
    return harris_responses(img, [x], [y])[0]


def harris_scale():
    scale = f32(f32(1) / f32(f32((1 << 2) * HARRIS_BLOCK) * f32(255)))
    return f32(f32(f32(scale * scale) * scale) * scale)


def harris_from_sums(a, b, c):
    fa, fb, fc = np.asarray(a).astype(f32), np.asarray(b).astype(f32), np.asarray(c).astype(f32)
    s = (fa + fb).astype(f32)
    t = (((fa * fb).astype(f32) - (fc * fc).astype(f32)).astype(f32) - ((f32(0.04) * s).astype(f32) * s).astype(f32)).astype(f32)
    return (t * harris_scale()).astype(f32)


def moments(img, xs, ys, umax):
    """F:261-280: (m01, m10) at the points"""
    I = img.astype(np.int64)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    m01 = np.zeros(len(xs), np.int64)
    m10 = np.zeros(len(xs), np.int64)
    for u in range(-HALF_PATCH, HALF_PATCH + 1):
        m10 += u * I[ys, xs + u]
    for v in range(1, HALF_PATCH + 1):
        d = umax[v]
        vsum = np.zeros(len(xs), np.int64)
        for u in range(-d, d + 1):
            p, m = I[ys + v, xs + u], I[ys - v, xs + u]
            vsum += p - m
            m10 += u * (p + m)
        m01 += v * vsum
    return m01, m10


def ic_angle(img, x, y, umax):
    """F:250-283 with the restated atan2f, in degrees in [0, 360)"""
    m01, m10 = moments(img, [x], [y], umax)
    return angle_of(int(m01[0]), int(m10[0]))


RAD2DEG = f32(180.0 / math.pi)
DEG2RAD = f32(math.pi / 180.0)


def angle_of(m01, m10):
    a = f32(polar_np.atan2f(f32(m01), f32(m10)) * RAD2DEG)
    if a < 0:
        a = f32(a + f32(360))
    if a >= f32(360):
        a = f32(a - f32(360))
    return a


def blur(img):
    """(sum_y k_y sum_x k_x p + 2^15) >> 16 where the 7 x 7 window lies inside the layer; the rim is left as it is (nothing reads it)"""
    h, w = img.shape
    out = img.copy()
    if h < 7 or w < 7:
        return out
    I = img.astype(np.int64)
    hs = sum(k * I[:, i:w - 6 + i] for i, k in enumerate(BLUR_TAPS))
    vs = sum(k * hs[i:h - 6 + i] for i, k in enumerate(BLUR_TAPS))
    out[3:h - 3, 3:w - 3] = ((vs + (1 << 15)) >> 16).astype(np.uint8)
    return out


def describe(blurred, cx, cy, angle_deg, pattern):
    """F:300-352"""
    sn, cs = polar_np.sincosf(f32(f32(angle_deg) * DEG2RAD))
    a, b = f32(cs), f32(sn)
    px, py = pattern[:, 0].astype(f32), pattern[:, 1].astype(f32)
    x = ((px * a).astype(f32) - (py * b).astype(f32)).astype(f32)
    y = ((px * b).astype(f32) + (py * a).astype(f32)).astype(f32)
    ix, iy = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    v = blurred[cy + iy, cx + ix].astype(np.int64)
    bits = (v[0::2] < v[1::2]).astype(np.uint8)
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


# ---- the finder -----------------------------------------------------------------------------------------------------------------------
class Result:
    def __init__(self, keypoints, meta, descriptors, status):
        self.keypoints, self.meta, self.descriptors, self.status = keypoints, meta, descriptors, status
        self.count = len(keypoints)


def find(image, params=None, pattern=None, stages=None):
    """(keypoints n x 2 float32, meta n x 4 float32 = size, angle, response, octave, descriptors n x 32 uint8, status).  stages: a dict
    that receives the intermediate sets per (cell, level) when given."""
    p = params or Params()
    pattern = default_pattern() if pattern is None else np.asarray(pattern, np.int32)
    if not pattern_ok(pattern):
        return Result(np.zeros((0, 2), f32), np.zeros((0, 4), f32), np.zeros((0, 32), np.uint8), STATUS_BAD_PATTERN)
    gray = gray_of(image)
    H, W = gray.shape
    scales = level_scales(p.scale_factor, p.nlevels)
    n_l = features_per_level(p.per_cell, p.scale_factor, p.nlevels)
    umax = umax_table()
    kps, metas, descs, status = [], [], [], 0
    for ci, (xl, yl, xr, yr) in enumerate(cells_of(W, H, p.grid)):
        layers = pyramid(gray[yl:yr, xl:xr], scales)
        for l, img in enumerate(layers):
            if img is None:
                continue
            kept = nms_keep(fast_scores(img, p.fast_threshold))
            ys, xs = np.nonzero(kept)                               # row-major: canonical order
            first, trunc1 = retain_best(kept[ys, xs], 2 * n_l[l], 2 * n_l[l] + CAND_TIE_ROOM)
            ys, xs = ys[first], xs[first]
            resp = harris_responses(img, xs, ys) if len(xs) else np.zeros(0, f32)
            final, trunc2 = retain_best(resp, n_l[l], n_l[l] + KEEP_TIE_ROOM)
            if trunc1 or trunc2:
                status |= STATUS_TRUNCATED
            if stages is not None:
                stages[(ci, l)] = {"candidates": np.stack([xs, ys], 1), "responses": resp, "final": final, "truncated": (trunc1, trunc2)}
            if not len(final):
                continue
            blurred = blur(img)
            scale = scales[l]
            inv = f32(f32(1) / scale)
            m01, m10 = moments(img, xs[final], ys[final], umax)
            for k, i in enumerate(final):
                x, y = int(xs[i]), int(ys[i])
                ang = angle_of(int(m01[k]), int(m10[k]))
                ptx, pty = f32(f32(x) * scale), f32(f32(y) * scale)                    # F:189
                cx, cy = cv_round(f32(ptx * inv)), cv_round(f32(pty * inv))            # F:305-306
                descs.append(describe(blurred, cx, cy, ang, pattern))
                kps.append((f32(ptx + f32(xl)), f32(pty + f32(yl))))                   # F:1006-1007
                metas.append((f32(f32(PATCH) * scale), ang, resp[i], f32(l)))
    if not kps:
        return Result(np.zeros((0, 2), f32), np.zeros((0, 4), f32), np.zeros((0, 32), np.uint8), status)
    return Result(np.array(kps, f32), np.array(metas, f32), np.array(descs, np.uint8), status)
