"""The NumPy model of the DP seam finder with both cost functions (tests/helpers/dpseam_grad_np.py, the specification of
isx_dp_seam_find_cost / isx_seam_estimate_cost / isx_seam_gradients; no GPU): its restated dynamic programme with COLOR against the C
oracle's estimateSeam point for point, its gradient maps on answers worked by hand, and the whole `find` with COLOR_GRAD on known
answers - on inputs where the two cost functions give different seams."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import dpseam_grad_np as M  # noqa: E402
from seam_cases import make_case, make_find_case  # noqa: E402

F = np.float32

# (n_images, u8, seed of make_find_case(1000 * n + seed, holes=True)) -> non-zero mask bytes the model leaves with COLOR and with COLOR_GRAD;
# tests/test_gpu_seam_grad.py reuses the table
FIND_CASES = {
    (2, False, 1): ([10002, 13845], [10164, 13683]),
    (2, False, 2): ([14168, 13217], [14480, 12905]),
    (2, False, 5): ([11003, 14438], [11642, 13799]),
    (2, True, 1): ([10002, 13845], [10168, 13679]),
    (2, True, 2): ([14168, 13217], [13886, 13499]),
    (2, True, 5): ([11003, 14438], [11492, 13949]),
    (3, False, 0): ([14543, 7182, 12390], [14340, 7951, 11824]),
    (3, False, 1): ([12907, 9794, 13764], [13080, 9447, 13938]),
    (3, False, 6): ([10902, 5755, 16337], [10894, 6046, 16054]),
    (3, True, 0): ([14543, 7182, 12390], [14338, 7953, 11824]),
    (3, True, 1): ([12907, 9794, 13764], [13094, 9433, 13938]),
    (3, True, 6): ([10902, 5755, 16337], [10891, 5974, 16129]),
}
# the reference's reconstructed inputs (tests/golden/ref_dpseam_artifact.npz): COLOR gives its committed mask_seam[*].bmp
REF_NONZERO_COLOR = [1021527, 1048272]
REF_NONZERO_COLOR_GRAD = [1021302, 1048497]


def seam_args(c):
    return (c["img1"], c["img2"], c["tl1"], c["tl2"], c["union_tl"], c["labels"], c["label"], c["roi"], c["p1"], c["p2"])


# ---- the restated dynamic programme, before the new cost is trusted ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("horizontal", [False, True])
def test_color_seam_equals_the_c_oracle(oracle, seed, u8, horizontal):
    """both directions, swapped tips (odd seeds), f32 and u8, with and without holes"""
    c = make_case(seed, u8=u8, horizontal=horizontal, swap=bool(seed & 1), holes=seed % 3 != 0)
    ref, rh = oracle.seam_estimate(*seam_args(c))
    got, gh = M.seam_estimate(*seam_args(c), M.COLOR)
    assert gh == rh and got.shape == ref.shape and np.array_equal(got, ref)
    assert len(ref) > 0


def test_color_seam_unreachable_tip_and_more_seeds(oracle):
    for seed in range(100, 108):
        c = make_case(seed, holes=False)
        ref, rh = oracle.seam_estimate(*seam_args(c))
        got, gh = M.seam_estimate(*seam_args(c), M.COLOR)
        assert gh == rh and len(ref) > 0 and np.array_equal(got, ref)
    c = make_case(5, holes=False)
    rx, ry, rw, rh = c["roi"]
    c["labels"][ry + rh // 2, :] = 9                      # a wall: p2 cannot be reached
    for cf in (M.COLOR, M.COLOR_GRAD):
        got, _ = M.seam_estimate(*seam_args(c), cf)
        assert got.shape == (0, 2)
    assert len(oracle.seam_estimate(*seam_args(c))[0]) == 0


def test_color_grad_moves_the_seam_of_the_estimate_cases():
    moved = 0
    for seed in range(6):
        c = make_case(seed, u8=bool(seed & 2), horizontal=bool(seed & 1))
        a, _ = M.seam_estimate(*seam_args(c), M.COLOR)
        b, _ = M.seam_estimate(*seam_args(c), M.COLOR_GRAD)
        assert len(a) == len(b) > 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[-1], b[-1])
        moved += not np.array_equal(a, b)
    assert moved == 6


# ---- gradients, worked by hand ---------------------------------------------------------------------------------------------------------
def grey_u8(g):
    """a CV_8UC3 image whose three channels all hold g: its gray is g itself (1868 + 9617 + 4899 = 16384 = 1 << 14)"""
    return np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=2)


def abs_grads(image):
    gx, gy = M.gradients(image)
    return np.abs(gx), np.abs(gy)


def test_constant_image_has_no_gradient():
    for img in (np.full((5, 7, 3), 93, np.uint8), np.full((5, 7, 3), 93.25, F), np.full((1, 1, 3), 200, np.uint8)):
        gx, gy = abs_grads(img)
        assert gx.shape == img.shape[:2] and gx.dtype == F and not gx.any() and not gy.any()


def test_ramp_in_x():
    """g = x: d = 2 inside, and the column pass weighs it (1 + 1) + (2 + 2) = 8 times a half: |gradx| = 8; REFLECT_101 makes the first
    and the last column see the same pixel on both sides: 0; nothing changes along y"""
    g = np.tile(np.arange(9), (6, 1))
    gx, gy = abs_grads(grey_u8(g))
    assert (gx[:, 1:-1] == 8).all() and not gx[:, 0].any() and not gx[:, -1].any() and not gy.any()
    gx, gy = abs_grads(grey_u8(g.T))                      # and g = y
    assert (gy[1:-1] == 8).all() and not gy[0].any() and not gy[-1].any() and not gx.any()


def test_one_pixel_dimensions():
    """1 x N: the rows above and below are row 0 itself, so the column pass gives 4 d = 8 inside; N x 1: s = 4 g, s(y + 1) - s(y - 1) = 8"""
    gx, gy = abs_grads(grey_u8(np.arange(7)[None, :] * 3))
    assert gx.tolist() == [[0, 24, 24, 24, 24, 24, 0]] and not gy.any()
    gx, gy = abs_grads(grey_u8(np.arange(7)[:, None] * 3))
    assert gy[:, 0].tolist() == [0, 24, 24, 24, 24, 24, 0] and not gx.any()
    gx, gy = abs_grads(grey_u8(np.array([[5, 9]])))       # 1 x 2: both columns are borders
    assert not gx.any() and not gy.any()


def test_byte_gray_of_a_few_triples():
    """(b * 1868 + g * 9617 + r * 4899 + 8192) >> 14: white 4186112 >> 14 = 255; blue 484532 >> 14 = 29; green 2460527 >> 14 = 150; red
    1257437 >> 14 = 76; (10, 20, 30) 366182 >> 14 = 22; (255, 255, 0) 2936867 >> 14 = 179"""
    bgr = np.array([[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30], [255, 255, 0], [0, 0, 0]]], np.uint8)
    assert M.gray(bgr).tolist() == [[255, 29, 150, 76, 22, 179, 0]]
    f = M.gray(bgr.astype(F))                             # the float form keeps its fraction: (255 * 0.114f + 255 * 0.587f) + 255 * 0.299f
    assert f.dtype == F and f[0, 0] == (F(255) * F(0.114) + F(255) * F(0.587)) + F(255) * F(0.299)
    assert abs(float(f[0, 4]) - (10 * 0.114 + 20 * 0.587 + 30 * 0.299)) < 1e-5


def test_the_association_order_is_the_specified_one():
    """Centre of a 3 x 3 gray with d(0, 1) = 2^24, d(1, 1) = 0.5, d(2, 1) = -2^24.  The specified order (d(y - 1) + d(y + 1)) + (d(y) + d(y))
    = 0 + 1 = 1; a running sum (d(y - 1) + 2 d(y)) + d(y + 1) rounds 2^24 + 1 to 2^24 (ties to even) and gives 0."""
    big = F(2.0 ** 24)
    g = np.array([[0, 7, big], [0, 7, 0.5], [big, 7, 0]], F)
    gradx, _ = M.sobel_xy(g)
    assert gradx[1, 1] == F(1.0)
    assert (big + (F(0.5) + F(0.5))) + -big == F(0.0)


def test_cost_cells_by_hand():
    """Two 3 x 4 byte tiles at the same corner, one component.  Tile 1: gray = 10 x (|gradx| = 80 inside, 0 in columns 0 and 3); tile 2: flat 0.
    costV(y, 2): the two SSDs are 3 * 10^2 and 3 * 20^2, costColor = (300 + 1200) / 2 = 750, costGrad = 80 + 80 + 0 + 0 + 1 = 161.
    costV(y, 1): SSDs 3 * 0 and 3 * 10^2 -> 150, costGrad = 80 + 0 + 1 = 81.  costH: both SSDs 3 * (10 x)^2, grady = 0 -> costGrad = 1."""
    img1 = grey_u8(np.tile(np.arange(4) * 10, (3, 1)))
    img2 = np.zeros((3, 4, 3), np.uint8)
    labels = np.full((3, 4), 1, np.int32)
    args = (img1, img2, (0, 0), (0, 0), (0, 0), labels, 1, (0, 0, 4, 3))
    cv, ch = M.compute_costs(*args, M.COLOR_GRAD)
    assert cv.shape == (3, 5) and ch.shape == (4, 4) and cv.dtype == F
    assert (cv[:, 0] == M.BAD_REGION_COST).all() and (cv[:, 4] == M.BAD_REGION_COST).all() and (ch[0] == M.BAD_REGION_COST).all() and (ch[3] == M.BAD_REGION_COST).all()
    assert (cv[:, 2] == F(750) / F(161)).all() and (cv[:, 1] == F(150) / F(81)).all()
    assert ch[1].tolist() == [0, 300, 1200, 2700]
    cv0, ch0 = M.compute_costs(*args, M.COLOR)
    assert (cv0[:, 2] == 750).all() and (cv0[:, 1] == 150).all() and np.array_equal(ch0, ch)


# ---- the whole find ------------------------------------------------------------------------------------------------------------------
def model_find(cost_func, images, corners, masks):
    out = [m.copy() for m in masks]
    M.DpSeamFinder(cost_func).find(images, corners, out)
    return out


@pytest.mark.parametrize("key", sorted(FIND_CASES))
def test_find_known_answers_and_the_two_cost_functions_differ(key):
    from oracle.dpseam_np import DpSeamFinder as OracleFinder
    n, u8, seed = key
    images, corners, masks = make_find_case(1000 * n + seed, n, u8, holes=True)
    color, grad = model_find(M.COLOR, images, corners, masks), model_find(M.COLOR_GRAD, images, corners, masks)
    ref = [m.copy() for m in masks]
    OracleFinder().find(images, corners, ref)                            # COLOR: the finder the C oracle's estimateSeam drives
    assert all(np.array_equal(a, b) for a, b in zip(color, ref))
    assert [int(np.count_nonzero(m)) for m in color] == FIND_CASES[key][0]
    assert [int(np.count_nonzero(m)) for m in grad] == FIND_CASES[key][1]
    assert any((a != b).any() for a, b in zip(color, grad))              # a suite on which both give the same seam shows nothing
    assert all(set(np.unique(m)) <= {0, 255} for m in grad)


def test_find_on_the_references_tiles():
    """tests/golden/ref_dpseam_artifact.npz: with COLOR the model gives the reference's committed mask_seam[*].bmp; COLOR_GRAD moves the seam."""
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    color = model_find(M.COLOR, c["images"], c["corners"], c["masks_in"])
    assert np.array_equal(color[0], c["masks_out"][0]) and np.array_equal(color[1], c["masks_out"][1])
    grad = model_find(M.COLOR_GRAD, c["images"], c["corners"], c["masks_in"])
    assert [int(np.count_nonzero(m)) for m in color] == REF_NONZERO_COLOR
    assert [int(np.count_nonzero(m)) for m in grad] == REF_NONZERO_COLOR_GRAD
    assert (color[0] != grad[0]).any() and (color[1] != grad[1]).any()
