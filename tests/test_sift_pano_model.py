"""The planted rig of tests/pano_cases.py through the SIFT model chain (sift_cases.model_chain: sift_np.find -> match_f32_np -> homography_np ->
estimator_np -> bundle_np) at the classes' defaults (contrast_threshold 0.04, which the rendered rig is not too smooth for; match_conf 0.3): what the 128 floats are worth against the
ground truth.  The records below are the model chain's own figures on the CPU (python tests/test_sift_pano_model.py prints them); every bound
is pano_cases.BOUND_FACTOR (2) x the recorded one, the margin pano_cases.within takes for a change in match order moving RANSAC's draw.
tests/test_gpu_sift_chain.py holds the GPU classes to the same figures.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pano_cases as P  # noqa: E402
import sift_cases as cases  # noqa: E402

CONF_THRESH = 1.0               # the adjusters' conf_thresh

# rig3(): keypoints per view; per pair (0,1) (0,2) (1,2) matches, inliers and confidence
RECORDED = dict(keypoints=[442, 390, 414], pairs=[(0, 1), (0, 2), (1, 2)], matches=[173, 111, 148], inliers=[134, 86, 116], confidence=[2.24, 2.08, 2.21])
# pano_cases.measure of the estimator's and BundleAdjusterRay's cameras: focal error, rotation error in degrees, misregistration in px
MEASURED = {
    "est": dict(focal=7.74, rot=0.161, mean_cylindrical=0.153, max_cylindrical=0.285, mean_spherical=0.151, max_spherical=0.284, mean_plane=0.156,
                max_plane=0.363, mean_angle=0.148, max_angle=0.264),
    "ray": dict(focal=0.683, rot=0.0351, mean_cylindrical=0.0921, max_cylindrical=0.186, mean_spherical=0.0893, max_spherical=0.16, mean_plane=0.0942,
                max_plane=0.191, mean_angle=0.0883, max_angle=0.16),
}


def test_the_records_are_the_chains():
    c = cases.chain3()
    assert [f["count"] for f in c["feats"]] == RECORDED["keypoints"] and c["pairs"] == RECORDED["pairs"]
    assert [r["count"] for r in c["recs"]] == RECORDED["matches"] and c["stats"][:, 1].tolist() == RECORDED["inliers"]
    assert np.allclose(c["conf"][0], RECORDED["confidence"], atol=0.005)


def test_every_pair_is_confident():
    conf = cases.chain3()["conf"][0]
    print("confidence", conf)
    assert (conf > CONF_THRESH).all(), conf


def test_measures_within_twice_the_records():
    rig, c = P.rig3(), cases.chain3()
    for stage in ("est", "ray"):
        got = P.measure(c[stage][0], rig)
        print(stage, {k: float("%.3g" % v) for k, v in got.items()})
        assert P.within(got, MEASURED[stage]) == [], stage
    # the adjuster does not undo what the features gave it
    assert P.measure(c["ray"][0], rig)["max_angle"] < 1.0


def test_control_keypoints_not_centred():
    """The points reach the homography as pt, not pt - size / 2: the estimator's cameras leave the panorama by more than the floor."""
    rig = P.rig3()
    c = cases.model_chain(rig["views"], centred=False)
    worst = {kind: max(v[1] for v in P.misregistration(c["est"][0], rig, kind)) for kind in P.KINDS}
    print("not centred: estimator", worst)
    assert min(worst.values()) > P.CONTROL_FLOOR_PX and P.within(P.measure(c["est"][0], rig), MEASURED["est"]) != []


if __name__ == "__main__":
    c, rig = cases.chain3(), P.rig3()
    print([f["count"] for f in c["feats"]], c["pairs"], [r["count"] for r in c["recs"]], c["stats"][:, 1].tolist(), c["conf"][0])
    for stage in ("est", "ray"):
        print(stage, {k: float("%.3g" % v) for k, v in P.measure(c[stage][0], rig).items()})
