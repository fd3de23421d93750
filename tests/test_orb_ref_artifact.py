"""The pin of the features finder to the reference: F (its 特征点检测 demo) commits src1.bmp and 重构的特征点.bmp, which is src1.bmp with drawKeypoints of
F's restated finder on top - a radius-3 circle, the 16 pixels of FAST's own ring, around every keypoint.  tests/golden/ref_orb_artifact.npz
(tests/golden/make_golden_orb.py) holds the gray of src1.bmp and the mask of the pixels that differ.  The NumPy model at the F defaults
(tests/helpers/orb_np.py, which the GPU matches bit for bit: tests/test_gpu_orb.py) must have put its keypoints where the reference drew
them.  A wrong FAST, Harris or selection moves hundreds of keypoints; what is allowed to differ is what this project decided differently
(INTER_LINEAR for INTER_LINEAR_EXACT above level 0, DESIGN.md §8 "Features finder").  No GPU."""
import os

import numpy as np
import pytest

from helpers import orb_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the committed model's exact counts on the whole image (DESIGN.md §8 "Features finder" records them)
KEYPOINTS, LEVEL0, RING_16, RING_12_OR_MORE, RING_UNDER_10, DRAWN, DRAWN_FAR = 1530, 483, 1512, 1516, 13, 38911, 252


@pytest.fixture(scope="module")
def pinned():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_orb_artifact.npz"))
    shape = tuple(int(v) for v in z["shape"])
    drawn = np.unpackbits(z["drawn"])[:shape[0] * shape[1]].reshape(shape).astype(bool)
    whole = bool(z["whole"])
    p = M.Params() if whole else M.Params(grid=(1, 1), n_features=510)      # cell 0 alone is one cell of 510
    return z["gray"], drawn, whole, p, M.find(z["gray"], p)


def ring_counts(drawn, keypoints):
    c = np.rint(keypoints).astype(int)
    n = np.zeros(len(c), int)
    for dx, dy in M.CIRCLE:
        x, y = c[:, 0] + dx, c[:, 1] + dy
        ok = (x >= 0) & (y >= 0) & (x < drawn.shape[1]) & (y < drawn.shape[0])
        n += ok & drawn[np.clip(y, 0, drawn.shape[0] - 1), np.clip(x, 0, drawn.shape[1] - 1)]
    return n


def far_pixels(drawn, keypoints, radius=5):
    """drawn pixels farther than `radius` (Euclidean) from every rounded keypoint"""
    near = np.zeros(drawn.shape, bool)
    c = np.rint(keypoints).astype(int)
    offs = [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius]
    for dx, dy in offs:
        x, y = c[:, 0] + dx, c[:, 1] + dy
        ok = (x >= 0) & (y >= 0) & (x < drawn.shape[1]) & (y < drawn.shape[0])
        near[y[ok], x[ok]] = True
    return int((drawn & ~near).sum())


def test_the_model_finds_what_the_reference_drew(pinned):
    gray, drawn, whole, p, r = pinned
    cells = p.grid[0] * p.grid[1]
    assert r.status == 0 and r.count == 510 * cells
    # 510 per cell, in canonical order
    bounds = M.cells_of(gray.shape[1], gray.shape[0], p.grid)
    per_cell = [int(((r.keypoints[:, 0] >= xl) & (r.keypoints[:, 0] < xr)).sum()) for xl, yl, xr, yr in bounds]
    print("per cell", per_cell)
    ring = ring_counts(drawn, r.keypoints)
    level0 = r.meta[:, 3] == 0
    far = far_pixels(drawn, r.keypoints)
    print("keypoints", r.count, "level 0", int(level0.sum()), "ring == 16:", int((ring == 16).sum()), ">= 12:", int((ring >= 12).sum()), "< 10:", int((ring < 10).sum()),
          "drawn", int(drawn.sum()), "far", far)
    assert per_cell == [510] * cells
    assert (ring[level0] >= 12).all()                                     # every level-0 keypoint has its circle in the artefact
    assert (ring < 10).sum() <= 0.02 * r.count
    assert far <= 0.02 * drawn.sum()
    if whole:
        assert (r.count, int(level0.sum()), int((ring == 16).sum()), int((ring >= 12).sum()), int((ring < 10).sum()), int(drawn.sum()), far) == \
            (KEYPOINTS, LEVEL0, RING_16, RING_12_OR_MORE, RING_UNDER_10, DRAWN, DRAWN_FAR)


def test_the_fixture_is_what_its_maker_says(pinned):
    gray, drawn, whole, _, _ = pinned
    assert gray.dtype == np.uint8 and gray.shape == drawn.shape and gray.shape[0] == 1101 and gray.shape[1] == (1101 if whole else 367)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_orb_artifact.npz")) < (1 << 20)
    # circles only: no drawn pixel within 31 - 3 px of the image's edge rows (keypoints lie 31 px inside their layer)
    assert not drawn[:27].any() and not drawn[-27:].any()
