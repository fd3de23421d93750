"""An independent NumPy model of GainCompensator::feed (OpenCV 3.4.2, modules/stitching/src/exposure_compensate.cpp), the spec of
isx_gain_compensator_feed, with known-answer tests of the model itself, and the CPU-side checks of the new entry (exported, declared,
no CPU fallback).  tests/test_gpu_gain_feed.py compares the GPU entry with feed_model().

The model restates OpenCV's algorithm (its source is not in the reference tree; OpenCV is not installed here):
  for i <= j with overlapRoi(corners[i], corners[j], sizes[i], sizes[j], roi):
      intersect = (mask_i == 255) & (mask_j == 255);  N(i,j) = N(j,i) = max(1, countNonZero(intersect))
      I(i,j) = sum of sqrt((double)(r^2 + g^2 + b^2)) of image i over intersect / N(i,j);  I(j,i) the same of image j
  N and I start at 0 (Mat_::setTo(0)): a pair without overlap keeps N = 0, I = 0;   alpha = 0.01, beta = 100;   for i, for j:  b(i) += beta N;  A(i,i) += beta N;
      j != i:  A(i,i) += 2 alpha I(i,j) I(i,j) N(i,j);  A(i,j) -= 2 alpha I(i,j) I(j,i) N(i,j);   gains = solve(A, b, DECOMP_LU)
The sums here are math.fsum (correctly rounded), which is what the GPU entry's exact integer sums give; OpenCV's sequential
double sum differs from it by about n * eps relative."""
import ctypes as C
import math

import numpy as np
import pytest

ALPHA, BETA = 0.01, 100.0


def overlap_roi(tl1, tl2, sz1, sz2):
    """cv::detail::overlapRoi: (x, y, w, h) or None.  sz = (width, height)."""
    x_tl, y_tl = max(tl1[0], tl2[0]), max(tl1[1], tl2[1])
    x_br, y_br = min(tl1[0] + sz1[0], tl2[0] + sz2[0]), min(tl1[1] + sz1[1], tl2[1] + sz2[1])
    if x_tl < x_br and y_tl < y_br:
        return x_tl, y_tl, x_br - x_tl, y_br - y_tl
    return None


def terms(img):
    """sqrt((double)(r^2 + g^2 + b^2)) per pixel (IEEE sqrt: correctly rounded)."""
    s = (img.astype(np.int64) ** 2).sum(axis=2)
    return np.sqrt(s.astype(np.float64))


def feed_model(corners, images, masks):
    """Returns (N int64 n x n, I float64 n x n with a zero diagonal, Isum float64 n x n, A, b, gains)."""
    n = len(images)
    N = np.zeros((n, n), np.int64)
    I = np.zeros((n, n), np.float64)
    Isum = np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(i, n):
            hi, wi = images[i].shape[:2]
            hj, wj = images[j].shape[:2]
            roi = overlap_roi(corners[i], corners[j], (wi, hi), (wj, hj))
            if roi is None:
                continue
            x, y, w, h = roi
            def sub(a, k):
                ox, oy = x - corners[k][0], y - corners[k][1]
                return a[oy:oy + h, ox:ox + w]
            inter = (sub(masks[i], i) == 255) & (sub(masks[j], j) == 255)
            N[i, j] = N[j, i] = max(1, int(np.count_nonzero(inter)))
            if i == j:
                continue        # I(i,i) never enters A or b
            Isum[i, j] = math.fsum(terms(sub(images[i], i))[inter].tolist())
            Isum[j, i] = math.fsum(terms(sub(images[j], j))[inter].tolist())
            I[i, j] = Isum[i, j] / N[i, j]
            I[j, i] = Isum[j, i] / N[i, j]
    A = np.zeros((n, n), np.float64)
    b = np.zeros(n, np.float64)
    for i in range(n):
        for j in range(n):
            b[i] += BETA * N[i, j]
            A[i, i] += BETA * N[i, j]
            if j == i:
                continue
            A[i, i] += 2 * ALPHA * I[i, j] * I[i, j] * N[i, j]
            A[i, j] -= 2 * ALPHA * I[i, j] * I[j, i] * N[i, j]
    gains = np.linalg.solve(A, b)
    return N, I, Isum, A, b, gains


def _tile(h, w, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 3), dtype=np.uint8)


def _full(h, w):
    return np.full((h, w), 255, np.uint8)


# ---- known answers of the model --------------------------------------------------------------------------------------------------

def test_identical_images_give_unit_gains():
    """Tiles cut from one picture: every overlap sees the same pixels from both sides."""
    pano = _tile(60, 80, 1)
    corners = [(0, 0), (10, 3), (7, 25)]
    imgs = [pano[y:y + 30, x:x + 40] for x, y in corners]
    N, I, _, A, b, g = feed_model(corners, imgs, [_full(30, 40)] * 3)
    assert N[0, 1] == 30 * 27 and N[0, 0] == 1200
    assert I[0, 1] == I[1, 0] and I[0, 2] == I[2, 0]
    np.testing.assert_allclose(g, 1.0, rtol=1e-13)


def test_two_images_closed_form():
    a, c = _tile(20, 30, 2, 0, 128), _tile(20, 30, 3, 100, 256)
    corners = [(0, 0), (12, 4)]
    N, I, _, A, b, g = feed_model(corners, [a, c], [_full(20, 30)] * 2)
    n00, n11, n01 = 600, 600, 18 * 16
    assert (N[0, 0], N[1, 1], N[0, 1], N[1, 0]) == (n00, n11, n01, n01)
    i01 = math.fsum(terms(a[4:, 12:]).ravel().tolist()) / n01
    i10 = math.fsum(terms(c[:16, :18]).ravel().tolist()) / n01
    assert I[0, 1] == i01 and I[1, 0] == i10
    a00 = BETA * (n00 + n01) + 2 * ALPHA * i01 * i01 * n01
    a11 = BETA * (n01 + n11) + 2 * ALPHA * i10 * i10 * n01
    a01 = -2 * ALPHA * i01 * i10 * n01
    b0, b1 = BETA * (n00 + n01), BETA * (n01 + n11)
    det = a00 * a11 - a01 * a01
    want = [(b0 * a11 - a01 * b1) / det, (a00 * b1 - a01 * b0) / det]
    np.testing.assert_allclose(g, want, rtol=1e-13)
    assert g[0] > 1.0 > g[1]          # the darker tile is brightened, the brighter one darkened


def test_system_is_symmetric():
    rng = np.random.default_rng(4)
    imgs = [_tile(25, 35, 10 + k, 20 * k, 200 + 10 * k) for k in range(4)]
    masks = [(rng.random((25, 35)) < 0.8).astype(np.uint8) * 255 for _ in range(4)]
    corners = [(0, 0), (20, 2), (-10, 15), (30, -5)]
    N, I, _, A, b, g = feed_model(corners, imgs, masks)
    assert np.array_equal(N, N.T)
    # A(i,j) and A(j,i) are the same product taken in another order: equal up to its rounding
    np.testing.assert_allclose(A, A.T, rtol=4e-16, atol=0)
    assert np.all(A - np.diag(np.diag(A)) <= 0)
    assert np.all(np.linalg.eigvalsh(A) > 0)


def test_tiles_without_overlap_keep_gain_one():
    imgs = [_tile(10, 10, 5, 0, 60), _tile(10, 10, 6, 150, 256), _tile(10, 10, 7)]
    corners = [(0, 0), (5, 5), (100, 100)]
    N, I, _, A, b, g = feed_model(corners, imgs, [_full(10, 10)] * 3)
    assert N[0, 2] == N[2, 0] == N[1, 2] == N[2, 1] == 0 and I[0, 2] == I[2, 1] == 0.0
    assert N[2, 2] == 100 and b[2] == BETA * 100 and A[2, 2] == BETA * 100
    assert g[2] == 1.0
    assert g[0] != 1.0 and g[1] != 1.0


def three_tiles_one_pair_apart():
    """Three 10 x 10 tiles of one colour each in a row: 0 at x = 0, 1 at x = 5, 2 at x = 12 - tiles 0 and 2 do not overlap.
    Terms: tile 0 (3, 4, 0) -> 5, tile 1 (6, 8, 0) -> 10, tile 2 (0, 0, 20) -> 20; full masks."""
    colours = [(3, 4, 0), (6, 8, 0), (0, 0, 20)]
    imgs = [np.tile(np.array(c, np.uint8), (10, 10, 1)) for c in colours]
    return [(0, 0), (5, 0), (12, 0)], imgs, [_full(10, 10)] * 3


# Worked by hand.  Overlaps: 0-1 columns 5..9 (50 px), 1-2 columns 12..14 (30 px), 0-2 none.
#   N = [[100, 50, 0], [50, 100, 30], [0, 30, 100]];  I(0,1) = 5, I(1,0) = 10, I(1,2) = 10, I(2,1) = 20
#   b = 100 * row sums of N = [15000, 18000, 13000]
#   A(0,0) = 15000 + 2 * 0.01 * 5^2 * 50 = 15025;  A(0,1) = -2 * 0.01 * 5 * 10 * 50 = -50;  A(0,2) = 0
#   A(1,1) = 18000 + 0.02 * 100 * 50 + 0.02 * 100 * 30 = 18160;  A(1,0) = -50;  A(1,2) = -0.02 * 10 * 20 * 30 = -120
#   A(2,2) = 13000 + 0.02 * 400 * 30 = 13240;  A(2,1) = -120
# With N = 1 for the pair apart, b(0), b(2), A(0,0) and A(2,2) would each be 100 larger.
THREE_N = np.array([[100, 50, 0], [50, 100, 30], [0, 30, 100]], np.int64)
THREE_I = np.array([[0, 5, 0], [10, 0, 10], [0, 20, 0]], np.float64)
THREE_A = [[15025, -50, 0], [-50, 18160, -120], [0, -120, 13240]]
THREE_B = [15000, 18000, 13000]


def three_tiles_gains():
    """The exact solution of the hand-worked system (Cramer's rule in rationals)."""
    from fractions import Fraction as Fr

    def det(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    A = [[Fr(v) for v in r] for r in THREE_A]
    d = det(A)
    out = []
    for k in range(3):
        Ak = [[Fr(THREE_B[r]) if c == k else A[r][c] for c in range(3)] for r in range(3)]
        out.append(float(det(Ak) / d))
    return np.array(out)


def test_three_tiles_one_pair_apart_by_hand():
    corners, imgs, masks = three_tiles_one_pair_apart()
    N, I, _, A, b, g = feed_model(corners, imgs, masks)
    assert np.array_equal(N, THREE_N)
    assert np.array_equal(I, THREE_I)
    np.testing.assert_allclose(A, THREE_A, rtol=1e-15, atol=1e-12)
    assert np.array_equal(b, np.array(THREE_B, np.float64))
    want = three_tiles_gains()
    np.testing.assert_allclose(g, want, rtol=1e-13)
    assert g[0] > 1.0 and g[2] < 1.0


def test_mask_value_254_does_not_count():
    img = _tile(8, 8, 8)
    m0 = _full(8, 8)
    m1 = _full(8, 8)
    m1[:, :4] = 254
    N, I, _, _, _, _ = feed_model([(0, 0), (0, 0)], [img, img], [m0, m1])
    assert N[0, 1] == 32 and N[1, 1] == 32 and N[0, 0] == 64
    assert I[0, 1] == math.fsum(terms(img)[:, 4:].ravel().tolist()) / 32


def test_empty_intersect_gives_n_one_and_i_zero():
    img = _tile(8, 8, 9)
    m0 = np.zeros((8, 8), np.uint8)
    m0[:, :4] = 255
    m1 = np.zeros((8, 8), np.uint8)
    m1[:, 4:] = 255
    N, I, _, _, _, g = feed_model([(0, 0), (0, 0)], [img, img], [m0, m1])
    assert N[0, 1] == 1 and I[0, 1] == 0.0 and I[1, 0] == 0.0
    np.testing.assert_allclose(g, 1.0, rtol=1e-15)


# ---- the entry on the CPU side -----------------------------------------------------------------------------------------------------

def test_entry_is_exported_and_declared():
    from imagestitch_amd import _lib
    assert "isx_gain_compensator_feed" in _lib.declared_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "isx_gain_compensator_feed")
    import imagestitch_amd as I
    assert "GainCompensator" in I.__all__


def test_feed_without_gpu_fails_with_hip_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import imagestitch_amd as I
    comp = I.GainCompensator()
    with pytest.raises(I.IsxError) as e:
        comp.feed([(0, 0), (5, 0)], [_tile(6, 9, 1), _tile(6, 9, 2)], [_full(6, 9)] * 2)
    assert e.value.code == 4


def test_feed_argument_errors():
    """Argument checks come before any device call: they hold on a box without a GPU too."""
    import imagestitch_amd as I
    comp = I.GainCompensator()
    with pytest.raises(I.IsxError) as e:
        comp.feed([], [], [])
    assert e.value.code == 1
    with pytest.raises(I.IsxError) as e:
        comp.feed([(0, 0)], [np.zeros((6, 9), np.uint8)], [_full(6, 9)])
    assert e.value.code == 2
    with pytest.raises(I.IsxError) as e:
        comp.feed([(0, 0)], [_tile(6, 9, 1)], [np.zeros((6, 9), np.float32)])
    assert e.value.code == 2
    with pytest.raises(I.IsxError) as e:
        comp.feed([(0, 0)], [_tile(6, 9, 1)], [_full(6, 8)])
    assert e.value.code == 7
    with pytest.raises(I.IsxError):
        comp.gains()
