"""From pixels to a homography with nothing supplied from outside: two overlapping crops of one synthetic scene go through
OrbFeaturesFinder.find, BestOf2NearestMatcher (the exact 2-NN matcher and RANSAC homography), on device mats throughout, and H maps the
known shift.

The bound: the NumPy models alone (orb_np.find -> match_np.match_model -> homography_np.find_homography_np) on these two crops give
474 and 466 keypoints, 299 matches, 277 inliers and an H whose largest error at the four image corners is 0.70 px.  RANSAC draws from a
fixed seed, so the GPU chain - each stage bit-exact to its model - lands on the same H; the test asks for 2 x 0.70 = 1.4 px, the margin for
RANSAC's draw should a stage's order of matches ever change."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
from helpers import orb_np as M  # noqa: E402

pytestmark = pytest.mark.gpu
SHIFT, BOUND_PX = 60, 1.4


def test_find_match_homography_recover_the_shift(gpu):
    import torch
    scene = cases.scene(260, 400, 31)
    crops = [np.ascontiguousarray(scene[:, 0:300]), np.ascontiguousarray(scene[:, SHIFT:SHIFT + 300])]
    finder = gpu.OrbFeaturesFinder(grid=(1, 1), n_features=500)
    feats = finder.find([torch.from_numpy(c).cuda() for c in crops])
    want = [M.find(c, M.Params(grid=(1, 1), n_features=500)) for c in crops]
    assert [int(f.keypoints.shape[0]) for f in feats] == [w.count for w in want] == [474, 466]
    assert all(f.descriptors.is_cuda and f.keypoints.is_cuda for f in feats)
    matcher = gpu.BestOf2NearestMatcher(match_conf=0.3)
    info = matcher.match([f.descriptors for f in feats], [f.keypoints for f in feats], [f.img_size for f in feats])
    assert len(info) == 1 and info[0].H is not None
    print("matches", int(info[0].matches.shape[0]), "inliers", info[0].num_inliers, "confidence", info[0].confidence)
    H = info[0].H
    corners = np.array([[-150, -130, 1], [150, -130, 1], [150, 130, 1], [-150, 130, 1]], np.float64)      # pt - size / 2, as the matcher gathers points
    q = (H @ corners.T).T
    q = q[:, :2] / q[:, 2:]
    err = float(np.abs(q - (corners[:, :2] + [-SHIFT, 0])).max())
    print("largest corner error", err, "px")
    assert err <= BOUND_PX
    assert info[0].num_inliers >= 100 and info[0].confidence > 1.0
    gpu.OrbFeaturesFinder.release()
    matcher.release()
