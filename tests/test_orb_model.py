"""The features finder's NumPy model (tests/helpers/orb_np.py, the standard isx_orb_find is held to) on hand-built images: what FAST calls a
corner, non-max suppression, both cuts and their capacity rule, the host-side tables of F (the reference's 特征点检测 demo), the default
pattern, how far every reader goes, and the blur.  No GPU; the host entries of the library are compared where they exist."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
from helpers import orb_np as M  # noqa: E402

T = 20


def arc_image(n, delta, start=0):
    """flat 100 with `n` contiguous circle pixels around (20, 20) at 100 + delta"""
    img = np.full((41, 41), 100, np.uint8)
    for k in range(n):
        dx, dy = M.CIRCLE[(start + k) % 16]
        img[20 + dy, 20 + dx] = 100 + delta
    return img


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("start", [0, 5, 11])
def test_a_lone_arc_at_the_threshold(sign, start):
    """9 contiguous pixels brighter (darker) by d: score d - 1, a corner from d = threshold + 1 on; 8 are never one"""
    for d, want in ((T - 1, 0), (T, 0), (T + 1, T), (T + 2, T + 1), (90, 89)):
        assert M.fast_scores(arc_image(9, sign * d, start), T)[20, 20] == want, (sign, d)
    assert M.fast_scores(arc_image(8, sign * 90, start), T)[20, 20] == 0
    assert M.fast_scores(arc_image(16, sign * 90, start), T)[20, 20] == 89
    # the rim scores nothing
    rim = np.full((9, 9), 100, np.uint8)
    rim[0:3] = 250
    s = M.fast_scores(rim, T)
    assert not s[:3].any() and not s[-3:].any() and not s[:, :3].any() and not s[:, -3:].any()


def test_fast_against_its_definition():
    """the vectorised score map against the definition, pixel by pixel, on noise"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (24, 27), dtype=np.uint8)
    got = M.fast_scores(img, 5)
    for y in range(24):
        for x in range(27):
            want = 0
            if 3 <= y < 21 and 3 <= x < 24:
                d = [int(img[y + dy, x + dx]) - int(img[y, x]) for dx, dy in M.CIRCLE]
                a = max(min(d[(s + k) % 16] for k in range(9)) for s in range(16))
                b = min(max(d[(s + k) % 16] for k in range(9)) for s in range(16))
                sc = max(a, -b) - 1
                want = sc if sc >= 5 else 0
            assert got[y, x] == want, (x, y)


def test_nms_keeps_strict_maxima_inside_the_border():
    s = np.zeros((80, 90), np.int64)
    s[40, 40] = 50                                      # alone: kept
    s[40, 50] = s[40, 51] = 60                          # a plateau of two: neither
    s[44, 40], s[45, 41] = 70, 69                       # neighbours: the greater
    s[30, 40] = s[40, 30] = s[80 - 31, 40] = s[40, 90 - 31] = 90      # the border rule: 31 <= x < W - 31
    s[31, 45] = s[48, 58] = 91
    k = M.nms_keep(s)
    assert sorted(zip(*np.nonzero(k))) == [(31, 45), (40, 40), (44, 40), (48, 58)]
    assert not M.nms_keep(np.full((80, 90), 77, np.int64)).any()
    # the squares of orb_cases: at level 0 every corner of a square lies on a plateau
    img = cases.squares(224, 256)
    assert (M.fast_scores(img, T) > 0).any() and not M.nms_keep(M.fast_scores(img, T)).any()


def test_retain_best_and_the_capacity_rule():
    v = np.array([5, 9, 7, 7, 3, 7, 9, 1])
    keep = lambda n, cap: (list(M.retain_best(v, n, cap)[0]), M.retain_best(v, n, cap)[1])      # noqa: E731
    assert keep(8, 8) == ([0, 1, 2, 3, 4, 5, 6, 7], False) and keep(20, 20) == ([0, 1, 2, 3, 4, 5, 6, 7], False)      # count <= n: all
    assert keep(0, 4) == ([], False)                                                                                    # n = 0: none
    assert keep(2, 2) == ([1, 6], False)
    assert keep(3, 5) == ([1, 2, 3, 5, 6], False)       # the third largest is 7: its ties are kept
    assert keep(3, 4) == ([1, 2, 3, 6], True)           # ... while there is room, in canonical order
    assert keep(3, 3) == ([1, 2, 6], True)
    assert keep(1, 1) == ([1], True) and keep(1, 2) == ([1, 6], False)
    assert keep(6, 6) == ([0, 1, 2, 3, 5, 6], False)
    f = np.array([0.5, 0.25, 0.5, 0.5], np.float32)
    assert list(M.retain_best(f, 1, 2)[0]) == [0, 2] and M.retain_best(f, 1, 2)[1]


def test_ties_at_both_cuts_with_and_without_truncation():
    """identical dots: every FAST score and every Harris response ties"""
    st = {}
    r = M.find(cases.dots(224, 256, count=40), M.Params(grid=(1, 1), n_features=50), stages=st)       # n_0 = 16: 40 ties fit 288 and 48 rows
    assert st[(0, 0)]["truncated"] == (False, False) and len(st[(0, 0)]["candidates"]) == 40 and len(st[(0, 0)]["final"]) == 40 and r.status == 0
    assert len(set(st[(0, 0)]["responses"].tolist())) == 1
    st = {}
    r = M.find(cases.dots(224, 256, count=100), M.Params(grid=(1, 1), n_features=50), stages=st)      # 100 fit the first cut, 48 the final one
    assert st[(0, 0)]["truncated"] == (False, True) and len(st[(0, 0)]["candidates"]) == 100 and r.status == M.STATUS_TRUNCATED
    assert list(st[(0, 0)]["final"]) == list(range(48))                                               # the first in canonical order
    st = {}
    r = M.find(cases.dots(224, 256), M.Params(grid=(1, 1), n_features=100), stages=st)                # 480 dots: 2 * 32 + 256 candidates, 32 + 32 kept
    assert st[(0, 0)]["truncated"] == (True, True) and len(st[(0, 0)]["candidates"]) == 320 and len(st[(0, 0)]["final"]) == 64
    kp = r.keypoints[r.meta[:, 3] == 0]
    assert np.array_equal(kp, kp[np.lexsort((kp[:, 0], kp[:, 1]))])                                   # y, then x


def test_the_tables_of_f():
    p = M.Params()
    assert p.per_cell == 510 and p.scale_factor == float(np.float32(1.3)) and p.scale_factor != 1.3
    assert M.features_per_level(510, p.scale_factor, 5) == [161, 124, 95, 73, 57]
    assert M.features_per_level(3, p.scale_factor, 5)[-1] >= 0 and sum(M.features_per_level(510, p.scale_factor, 5)) == 510
    assert M.umax_table() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert [float(s) for s in M.level_scales(p.scale_factor, 3)] == [1.0, float(np.float32(1.3)), float(np.float32(np.float32(1.3).astype(np.float64) ** 2))]
    assert M.cells_of(1101, 1101, (3, 1)) == [(0, 0, 367, 1101), (367, 0, 734, 1101), (734, 0, 1101, 1101)]
    assert M.cells_of(256, 224, (3, 1))[1] == (85, 0, 170, 224)
    assert M.layer_size(367, 1101, M.level_scales(p.scale_factor, 5)[4]) == (128, 385)
    assert M.capacity(p) == 3 * (510 + 5 * M.KEEP_TIE_ROOM)
    assert M.cv_round(np.float32(2.5)) == 2 and M.cv_round(np.float32(3.5)) == 4 and M.cv_round(np.float32(-0.5)) == 0


def test_the_default_pattern():
    pat = M.default_pattern()
    assert pat.shape == (512, 2) and pat.dtype == np.int32 and pat.min() == -15 and pat.max() == 15 and M.pattern_ok(pat)
    assert pat[:4].tolist() == [[11, -10], [-14, 6], [8, -6], [7, 2]] and np.array_equal(pat, M.default_pattern())      # the seed, every time
    assert len({tuple(r) for r in pat.tolist()}) > 350
    bad = pat.copy()
    bad[17, 0] = -16
    assert not M.pattern_ok(bad) and M.find(cases.scene(80, 80, 1), M.Params(grid=(1, 1)), bad).status == M.STATUS_BAD_PATTERN
    from imagestitch_amd import features
    assert np.array_equal(features.default_pattern(), pat)


def test_the_host_entries_agree_with_the_model():
    from imagestitch_amd import _lib, features
    for grid, nf, sf, nl in (((3, 1), 1500, 1.3, 5), ((1, 1), 1500, 1.3, 5), ((2, 2), 777, 1.2, 8), ((3, 1), 100, 2.0, 3), ((1, 1), 0, 1.5, 1), ((4, 3), 5000, 1.1, 6)):
        q = features.default_params()
        q.grid_width, q.grid_height, q.n_features, q.scale_factor, q.nlevels = grid[0], grid[1], nf, sf, nl
        assert features.capacity(q) == M.capacity(M.Params(grid, nf, sf, nl)), (grid, nf, sf, nl)
    q = features.default_params()
    assert (q.grid_width, q.grid_height, q.n_features, q.nlevels, q.edge_threshold, q.patch_size, q.wta_k, q.first_level, q.score_type, q.fast_threshold) == \
        (3, 1, 1500, 5, 31, 31, 2, 0, 0, 20)
    for field, value, code in (("patch_size", 33, 6), ("wta_k", 3, 6), ("first_level", 1, 6), ("score_type", 1, 6), ("edge_threshold", 19, 6), ("nlevels", 9, 1),
                               ("nlevels", 0, 1), ("scale_factor", 1.0, 1), ("grid_width", 0, 1), ("fast_threshold", 0, 1), ("n_features", 20000, 6)):
        q = features.default_params()
        setattr(q, field, value)
        with pytest.raises(_lib.IsxError) as e:
            features.capacity(q)
        assert e.value.code == code, (field, e.value)
    assert {"isx_orb_find", "isx_orb_reserve", "isx_orb_release", "isx_orb_capacity", "isx_orb_default_params", "isx_orb_default_pattern"} <= set(_lib.declared_symbols())


def test_no_reader_leaves_its_layer():
    """every keypoint is >= 31 px inside its layer; FAST, Harris, the moment patch, the rotated pattern and the blur under it stay within 25,
    so the reference's copyMakeBorder (F:842-851) cannot be observed"""
    assert max(M.READER_REACH.values()) < M.EDGE
    assert M.READER_REACH["fast"] == max(max(abs(dx), abs(dy)) for dx, dy in M.CIRCLE)
    assert M.READER_REACH["harris"] == M.HARRIS_BLOCK // 2 + 1 and M.READER_REACH["moments"] == max(M.umax_table()) == M.HALF_PATCH
    corners = np.array([[15, 15], [15, -15], [-15, 15], [-15, -15], [15, 0], [0, 15]], np.float32)
    reach = 0
    for deg in np.arange(0, 360, 0.25, dtype=np.float32):
        sn, cs = M.polar_np.sincosf(np.float32(deg * M.DEG2RAD))
        x = (corners[:, 0] * cs).astype(np.float32) - (corners[:, 1] * sn).astype(np.float32)
        y = (corners[:, 0] * sn).astype(np.float32) + (corners[:, 1] * cs).astype(np.float32)
        reach = max(reach, int(np.abs(np.rint(x)).max()), int(np.abs(np.rint(y)).max()))
    assert reach <= M.READER_REACH["pattern"] and M.READER_REACH["pattern+blur"] == M.READER_REACH["pattern"] + len(M.BLUR_TAPS) // 2
    # the descriptor's centre is the keypoint again: cvRound(x * scale * (1.f / scale)) == x on every level
    for s in M.level_scales(M.Params().scale_factor, M.MAX_LEVELS):
        x = np.arange(0, 16384, dtype=np.float32)
        assert np.array_equal(np.rint(((x * s).astype(np.float32) * np.float32(np.float32(1) / s)).astype(np.float32)), x)
    # and the model reads nothing outside: a keypoint's outputs do not change when everything further than 25 px from it does
    img = cases.scene(100, 100, 2)
    st = {}
    r = M.find(img, M.Params(grid=(1, 1), nlevels=1), stages=st)
    assert r.count > 0
    x, y = (int(v) for v in r.keypoints[0])
    other = np.random.default_rng(1).integers(0, 256, img.shape, dtype=np.uint8)
    other[y - 25:y + 26, x - 25:x + 26] = img[y - 25:y + 26, x - 25:x + 26]
    pat, umax = M.default_pattern(), M.umax_table()
    for a in (img, other):
        ang = M.ic_angle(a, x, y, umax)
        assert ang == r.meta[0, 1] and M.harris_response(a, x, y) == r.meta[0, 2]
        assert np.array_equal(M.describe(M.blur(a), x, y, ang, pat), r.descriptors[0])


def test_the_blur():
    assert sum(M.BLUR_TAPS) == 256 and M.BLUR_TAPS == M.BLUR_TAPS[::-1]
    k = np.exp(-(np.arange(7) - 3.0) ** 2 / (2 * 2.0 ** 2))
    q = np.rint(k / k.sum() * 256).astype(int)
    q[3] -= q.sum() - 256                               # getGaussianKernel(7, 2) in Q8, the residual in the centre tap
    assert tuple(q) == M.BLUR_TAPS
    flat = np.full((20, 20), 137, np.uint8)
    assert np.array_equal(M.blur(flat), flat)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (15, 17), dtype=np.uint8)
    b = M.blur(img)
    acc = sum(M.BLUR_TAPS[i] * M.BLUR_TAPS[j] * int(img[4 + i, 6 + j]) for i in range(7) for j in range(7))
    assert b[7, 9] == (acc + (1 << 15)) >> 16
    assert np.array_equal(b[:3], img[:3]) and np.array_equal(b[:, -3:], img[:, -3:])


def test_harris_and_angle_against_their_loops():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (70, 70), dtype=np.uint8)
    x0, y0 = 33, 36
    I = img.astype(np.int64)
    a = b = c = 0
    for i in range(7):
        for j in range(7):
            y, x = y0 - 3 + i, x0 - 3 + j
            ix = (I[y, x + 1] - I[y, x - 1]) * 2 + (I[y - 1, x + 1] - I[y - 1, x - 1]) + (I[y + 1, x + 1] - I[y + 1, x - 1])
            iy = (I[y + 1, x] - I[y - 1, x]) * 2 + (I[y + 1, x - 1] - I[y - 1, x - 1]) + (I[y + 1, x + 1] - I[y - 1, x + 1])
            a, b, c = a + ix * ix, b + iy * iy, c + ix * iy
    assert M.harris_response(img, x0, y0) == M.harris_from_sums(a, b, c)
    f = np.float32
    k = f(f(1) / f(7140.0))
    want = f(f(f(f(f(a) * f(b)) - f(f(c) * f(c))) - f(f(f(0.04) * f(f(a) + f(b))) * f(f(a) + f(b)))) * f(f(f(k * k) * k) * k))
    assert M.harris_from_sums(a, b, c) == want
    # a vertical edge, brighter to the right: the centroid lies at +x, angle 0; brighter below: +y, 90 degrees
    edge = np.zeros((70, 70), np.uint8)
    edge[:, 36:] = 200
    assert M.ic_angle(edge, 35, 35, M.umax_table()) == 0 and M.ic_angle(edge.T.copy(), 35, 35, M.umax_table()) == 90
    assert M.ic_angle(edge[:, ::-1].copy(), 35, 35, M.umax_table()) == 180 and M.ic_angle(edge.T[::-1].copy(), 35, 35, M.umax_table()) == 270
    assert 0 <= float(M.angle_of(-1, 10 ** 9)) < 360 and math.isclose(float(M.angle_of(1, 1)), 45.0, rel_tol=1e-6)
