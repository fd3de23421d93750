"""Float descriptors through the registration chain: two keypoint sets related by a known homography (tests/homography_cases.py) with a
shared random 64-vector per correspondence plus small noise and unrelated vectors for the outliers.  BestOf2NearestMatcher.match returns
H, the inlier mask, num_inliers and confidence bit-equal to what find_homography gives on the MODEL's points and counts, and
HomographyBasedEstimator runs on the result."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import homography_cases as hcases  # noqa: E402
from helpers import match_f32_np as MF  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def features(seed, n=90, inliers=60, cols=64):
    """(descriptors, keypoints, sizes): image 1 holds image 0's keypoints under H_TRUE for the inliers, uniform points for the rest, in a
    shuffled order."""
    pts = hcases.planted(seed, n, inliers, noise=0.3)
    rng = np.random.default_rng(seed)
    d0 = rng.standard_normal((n, cols)).astype(F32)
    d1 = (d0 + rng.normal(0.0, 0.02, (n, cols))).astype(F32)
    follows = np.hypot(*(hcases.project(pts[:, :2]) - pts[:, 2:]).T) < 5.0
    d1[~follows] = rng.standard_normal((int((~follows).sum()), cols)).astype(F32)
    perm = rng.permutation(n)
    centre = np.array([400, 300], F32)
    return [d0, np.ascontiguousarray(d1[perm])], [pts[:, :2] + centre, np.ascontiguousarray(pts[perm, 2:]) + centre], [(800, 600), (800, 600)], int(follows.sum())


def test_best_of_2_nearest_matcher_on_float_descriptors(gpu):
    import torch
    from imagestitch_amd import homography
    descs, kps, sizes, n_in = features(31)
    want = MF.match_model(descs, [(0, 1)], 0.3, kps, sizes)[0]
    c = want["count"]
    assert n_in >= 50 and c >= n_in
    # the existing find_homography on the model's points and counts
    H, stats, conf = np.zeros((3, 3)), np.zeros((1, 8), np.int32), np.zeros((1, 1))
    mask = np.zeros((c, 1), np.uint8)
    homography.find_homography([want["points"]], np.array([[c]], np.int32), H, [mask], stats, conf)
    assert stats[0, 0] & 1 and stats[0, 1] >= 50
    assert np.allclose(H, hcases.H_TRUE / hcases.H_TRUE[2, 2], rtol=1e-2, atol=0.5)
    bm = gpu.BestOf2NearestMatcher(0.3, 6, 6)
    for place in (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(), np.array):
        rec = bm.match([place(d) for d in descs], [place(k) for k in kps], sizes)[0]
        m = rec.matches.cpu().numpy() if hasattr(rec.matches, "cpu") else rec.matches
        assert np.array_equal(m, want["matches"]) and rec.float_distances
        assert np.array_equal(np.asarray(rec.H).view(np.uint64), H.view(np.uint64))
        got_mask = rec.inliers_mask.cpu().numpy() if hasattr(rec.inliers_mask, "cpu") else np.asarray(rec.inliers_mask)
        assert np.array_equal(got_mask.ravel(), mask.ravel())
        assert rec.num_inliers == stats[0, 1] and np.float64(rec.confidence).view(np.uint64) == conf.view(np.uint64)[0, 0]
        est = gpu.HomographyBasedEstimator()
        cams = est([(800, 600), (800, 600)], bm)
        assert len(cams) == 2 and all(np.isfinite(cam.focal) and cam.focal > 0 for cam in cams) and est.last_info == (1, 1)
    bm.release()
    est.release()
    homography.release()
