"""The NumPy model of VoronoiSeamFinder (tests/helpers/voronoi_np.py, the specification of isx_voronoi_seam_find) on answers worked by hand,
its distance step against a brute-force city-block search, and the counts it gives on the reference's own tiles (no GPU)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import voronoi_np as V  # noqa: E402

# what the model gives on the reference's tiles and input masks (dpseam_case()); tests/test_gpu_voronoi_seam.py reuses them
REF_ROI = (256, -550, 287, 1097)
REF_SEAM_CELLS = 147736
REF_NONZERO_BEFORE = (1187558, 1194638)
REF_NONZERO_AFTER = (1022678, 1047121)


def ones(w, h):
    return np.full((h, w), 255, np.uint8)


def test_strip_pair_splits_in_the_middle_and_the_tie_goes_to_tile_2(oracle):
    """Two 1 x 6 strips at x = 0 and x = 3; the overlap is panorama columns 3, 4, 5.  Column 3 is 1 from tile 1's own cells (column 2) and 3
    from tile 2's (column 6): tile 2 loses it.  Column 4 is 2 from both: a tie, tile 1 loses it.  Column 5 is 3 and 1: tile 1 loses it."""
    m = [ones(6, 1), ones(6, 1)]
    V.find([(6, 1), (6, 1)], [(0, 0), (3, 0)], m)
    assert m[0].tolist() == [[255, 255, 255, 255, 0, 0]]
    assert m[1].tolist() == [[0, 255, 255, 255, 255, 255]]
    # one column wider (overlap columns 4, 5, 6 of two 1 x 7 strips at 0 and 4): 1|3, 2|2 (tie), 3|1 again
    m = [ones(7, 1), ones(7, 1)]
    V.find([(7, 1), (7, 1)], [(0, 0), (4, 0)], m)
    assert m[0].tolist() == [[255, 255, 255, 255, 255, 0, 0]] and m[1].tolist() == [[0, 255, 255, 255, 255, 255, 255]]


def test_tiles_meeting_corner_to_corner(oracle):
    """8 x 8 tiles at (0, 0) and (6, 6): the roi is the 2 x 2 block (6..7, 6..7) and the gap of 10 reaches past both tiles.  (6, 6) is 1
    from tile 1's own cells and 2 from tile 2's: tile 2 loses it.  (7, 7) is 2 and 1, and (7, 6), (6, 7) are 1 and 1 (ties): tile 1
    loses those three."""
    m = [ones(8, 8), ones(8, 8)]
    V.find([(8, 8), (8, 8)], [(0, 0), (6, 6)], m)
    want0, want1 = ones(8, 8), ones(8, 8)
    want0[6:8, 6:8] = [[255, 0], [0, 0]]
    want1[0, 0] = 0
    assert np.array_equal(m[0], want0) and np.array_equal(m[1], want1)


def test_identical_tiles_have_no_unique_cell(oracle):
    """Two 4 x 5 tiles at the same corner: neither has a cell of its own, both distances are the border-ring value, nothing is less:
    mask 1 is cleared over the roi (all of it), mask 2 is untouched."""
    m = [ones(5, 4), ones(5, 4)]
    V.find([(5, 4), (5, 4)], [(2, -3), (2, -3)], m)
    assert not m[0].any() and (m[1] == 255).all()


def test_one_tile_inside_the_other(oracle):
    """A 4 x 4 tile inside a 12 x 12 one: the small tile has no cell of its own, the large one has cells next to every roi cell:
    the small tile's mask is cleared, the large one's is untouched."""
    m = [ones(12, 12), ones(4, 4)]
    V.find([(12, 12), (4, 4)], [(0, 0), (4, 4)], m)
    assert (m[0] == 255).all() and not m[1].any()
    # the other way round in the list: tile 1 (the small one) loses the roi by the else branch
    m = [ones(4, 4), ones(12, 12)]
    V.find([(4, 4), (12, 12)], [(4, 4), (0, 0)], m)
    assert not m[0].any() and (m[1] == 255).all()


def test_a_later_pair_reads_what_an_earlier_pair_wrote(oracle):
    """Strips of one row: tile 0 = columns 0..5, tile 1 = 3..8, tile 2 = 4..10.
    (0, 1) as in the first test: tile 0 keeps 0..3, tile 1 loses column 3.
    (0, 2) over columns 4, 5: tile 0 is already 0 there, so both are tile 2's own cells (distance 0): tile 0 loses them again and tile 2
        stays whole.  (On the masks as given, column 4 would have been 1 from tile 0 and 2 from tile 2, and tile 2 would lose it.)
    (1, 2) over 4..8: all of it is shared and tile 1 has nothing else (column 3 is gone), tile 2 has 9, 10: tile 1 loses the roi."""
    sizes, corners = [(6, 1), (6, 1), (7, 1)], [(0, 0), (3, 0), (4, 0)]
    m = [ones(w, h) for w, h in sizes]
    V.find(sizes, corners, m)
    assert m[0].tolist() == [[255, 255, 255, 255, 0, 0]]
    assert not m[1].any()
    assert (m[2] == 255).all()
    # the same pair (0, 2) on fresh masks, for contrast
    f = [ones(6, 1), ones(7, 1)]
    V.find([sizes[0], sizes[2]], [corners[0], corners[2]], f)
    assert f[1].tolist() == [[0, 255, 255, 255, 255, 255, 255]] and f[0].tolist() == [[255, 255, 255, 255, 255, 0]]


def test_fewer_than_two_images_and_disjoint_tiles(oracle):
    assert V.find([], [], []) == []
    m = [ones(5, 4)]
    V.find([(5, 4)], [(0, 0)], m)
    assert (m[0] == 255).all()
    m = [ones(5, 4), ones(5, 4)]
    V.find([(5, 4), (5, 4)], [(0, 0), (5, 0)], m)          # they touch: overlapRoi is empty
    assert (m[0] == 255).all() and (m[1] == 255).all()


def test_distance_step_is_the_city_block_distance_to_the_nearest_unique_cell(oracle):
    rng = np.random.default_rng(7)
    for _ in range(12):
        h, w = int(rng.integers(3, 30)), int(rng.integers(3, 40))
        u = (rng.random((h, w)) < 0.08).astype(np.uint8) * 255
        u[int(rng.integers(0, h)), int(rng.integers(0, w))] = 255           # at least one unique cell
        ys, xs = np.nonzero(u)
        yy, xx = np.mgrid[0:h, 0:w]
        brute = (np.abs(yy[..., None] - ys) + np.abs(xx[..., None] - xs)).min(-1)
        assert np.array_equal(V.dist_to_unique(u), brute.astype(np.float32))
    # none at all: the border ring's INIT_DIST0 = INT_MAX >> 2 in 16.16 plus the distance to the ring
    d = V.dist_to_unique(np.zeros((5, 7), np.uint8))
    yy, xx = np.mgrid[0:5, 0:7]
    ring = 1 + np.minimum(np.minimum(yy, 4 - yy), np.minimum(xx, 6 - xx))
    want = ((np.int64(2 ** 31 - 1) >> 2) + 65536 * ring).astype(np.float32) * np.float32(1 / 65536)
    assert np.array_equal(d, want)


def test_float_comparison_past_8192_cells(oracle):
    """A 9000 x 3 tile inside a 9001 x 3 one at the same corner: tile 1 has no cell of its own (its distance is the ring value,
    INIT_DIST0 + 65536 * 11 on the roi's outer rows), tile 2 owns column 9000 only.  At panorama column 797 of those rows tile 2's
    distance is 8203 = 8192 + 11: the two 16.16 integers differ by one and the floats are equal, so seam is false there and tile 1 loses
    the cell - as it does left of it, where tile 2 is farther still; right of it tile 2 is nearer and also wins."""
    sizes, corners = [(9000, 3), (9001, 3)], [(0, 0), (0, 0)]
    m = [ones(*sizes[0]), ones(*sizes[1])]
    u1, u2 = V.unique_cells(V.submask(m[0], corners[0], (0, 0, 9000, 3)), V.submask(m[1], corners[1], (0, 0, 9000, 3)))
    d1, d2 = V.dist_to_unique(u1), V.dist_to_unique(u2)
    t1, t2 = (2 ** 31 - 1 >> 2) + 65536 * 11, 65536 * 8203
    assert t1 + 1 == t2 and np.float32(t1) == np.float32(t2)
    assert d1[10, 807] == d2[10, 807] == np.float32(t2) * np.float32(1 / 65536)
    V.find(sizes, corners, m)
    assert not m[0].any() and (m[1] == 255).all()


def test_reference_tiles(oracle):
    """The reference's warped tiles' masks as they went into its seam finder (tests/golden/ref_dpseam_artifact.npz)."""
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    masks = [np.array(m).copy() for m in c["masks_in"]]
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    assert [tuple(p) for p in c["corners"]] == [(-543, -550), (256, -555)]
    assert tuple(int((m != 0).sum()) for m in masks) == REF_NONZERO_BEFORE
    roi = V.overlap_roi(c["corners"][0], c["corners"][1], sizes[0], sizes[1])
    assert roi == REF_ROI
    work = [m.copy() for m in masks]
    seam = V.find_in_pair(work[0], work[1], c["corners"][0], c["corners"][1], roi)
    assert seam.shape == (1097, 287) and int(seam.sum()) == REF_SEAM_CELLS
    assert tuple(int((m != 0).sum()) for m in work) == REF_NONZERO_AFTER
    V.find(sizes, c["corners"], masks)
    assert all(np.array_equal(a, b) for a, b in zip(masks, work))


def test_no_cpu_fallback_without_gpu():
    """On a box without a GPU the finder fails with ISX_ERR_HIP and leaves the masks alone; argument errors come first."""
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import imagestitch_amd as I
    m = [ones(6, 1), ones(6, 1)]
    with pytest.raises(I.IsxError) as e:
        I.VoronoiSeamFinder().find([(6, 1), (6, 1)], [(0, 0), (3, 0)], m)
    assert e.value.code == 4 and (m[0] == 255).all() and (m[1] == 255).all()
    with pytest.raises(I.IsxError) as e:
        I.VoronoiSeamFinder().find([(6, 1), (7, 1)], [(0, 0), (3, 0)], m)
    assert e.value.code == 7
    assert I.VoronoiSeamFinder().find([(6, 1)], [(0, 0)], m[:1]) is not None     # fewer than 2 images: nothing to do, no device needed
