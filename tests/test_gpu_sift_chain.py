"""The planted rig of tests/pano_cases.py from pixels to cameras through the 128-float path - SiftFeaturesFinder -> BestOf2NearestMatcher (the L2
entry) -> HomographyBasedEstimator -> BundleAdjusterRay - on device mats: every hand-off against the CPU model chain of
tests/sift_cases.py (np.array_equal on bits for the finder, the matcher, the homography and the estimator; the adjuster by its own suite's
comparison), the ground-truth measures within the bounds tests/test_sift_pano_model.py records, and examples/stitch_pair.py --register
--small --features sift in a fresh process."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pano_cases as P  # noqa: E402
import sift_cases as cases  # noqa: E402
from test_gpu_bundle import check as check_ray  # noqa: E402
from test_gpu_estimator import check as check_estimator  # noqa: E402
from test_sift_pano_model import CONF_THRESH, MEASURED, RECORDED  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_registration_through_the_classes(gpu):
    import torch
    rig, want = P.rig3(), cases.chain3()
    imgs = [torch.from_numpy(v).cuda() for v in rig["views"]]
    feats = gpu.SiftFeaturesFinder().find(imgs)
    sizes = [f.img_size for f in feats]
    matcher = gpu.BestOf2NearestMatcher(cases.MATCH_CONF)
    info = matcher.match([f.descriptors for f in feats], [f.keypoints for f in feats], sizes)      # a list of SiftFeaturesFinder features, unchanged
    est = gpu.HomographyBasedEstimator()
    est(sizes, matcher)
    ba = gpu.BundleAdjusterRay()
    ba(sizes, [f.keypoints for f in feats], matcher, est)
    lo = matcher.last_outputs
    for a in [f.keypoints for f in feats] + [f.descriptors for f in feats] + [lo["counts"], lo["H"], lo["stats"], lo["conf"]] + list(lo["matches"]) + list(est.last_outputs) \
            + list(ba.last_outputs):
        assert a.is_cuda, "a hand-off mat is not on the device"
    # the finder
    assert [int(f.keypoints.shape[0]) for f in feats] == RECORDED["keypoints"]
    for i, (f, w) in enumerate(zip(feats, want["feats"])):
        assert f.status == w["status"] and f.descriptors.dtype == torch.float32 and tuple(f.descriptors.shape) == (w["count"], 128) and f.meta.shape[1] == 5
        assert np.array_equal(_np(f.keypoints), w["keypoints"]) and np.array_equal(_np(f.meta), w["meta"]) and np.array_equal(_np(f.descriptors), w["descriptors"]), i
    # the matcher and the homography
    assert lo["pairs"] == want["pairs"] and np.array_equal(_np(lo["counts"])[0, :len(want["pairs"])], want["counts"][0])
    H, stats, conf = _np(lo["H"]), _np(lo["stats"]), _np(lo["conf"])
    for k, (rec, hom, inf) in enumerate(zip(want["recs"], want["hom"], info)):
        assert inf.float_distances and np.array_equal(_np(inf.matches), rec["matches"]), ("matches", k)
        assert np.array_equal(_np(inf.src_points), rec["points"][:, 0:2]) and np.array_equal(_np(inf.dst_points), rec["points"][:, 2:4]), ("points", k)
        assert np.array_equal(stats[k], hom["stats"]) and np.array_equal(_u64(H[3 * k:3 * k + 3]), _u64(hom["H"])) and np.array_equal(_u64(conf[0, k]), _u64(hom["conf"])), k
        assert inf.num_inliers == RECORDED["inliers"][k] and inf.confidence > CONF_THRESH
    # the estimator and the adjuster
    got_est, got_ray = tuple(_np(a) for a in est.last_outputs), tuple(_np(a) for a in ba.last_outputs)
    check_estimator(got_est, want["est"], "estimator")
    check_ray(got_ray, want["ray"], "ray")
    for stage, cams in (("est", got_est[0]), ("ray", got_ray[0])):
        m = P.measure(cams, rig)
        print(stage, {k: round(v, 4) for k, v in m.items()})
        assert P.within(m, MEASURED[stage]) == [], stage
    matcher.release()
    est.release()
    ba.release()
    gpu.SiftFeaturesFinder.release()


def test_the_example_registers_with_sift_in_a_fresh_process(gpu, tmp_path):
    """examples/stitch_pair.py --register --small --features sift in a child process: exit status 0, and the keypoints, matches and inliers of
    its output line are those of the CPU model chain on the same two crops: 212 and 209, 154 and 154"""
    script = os.path.join(ROOT, "examples", "stitch_pair.py")
    run = subprocess.run([sys.executable, script, "--register", "--small", "--features", "sift", "--out", str(tmp_path / "pano.bmp")], capture_output=True, text=True,
                         timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("registered:")]
    assert len(line) == 1
    spec = importlib.util.spec_from_file_location("stitch_pair_example", script)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    c = cases.model_chain(ex.register_views(True), contrast_threshold=ex.BUILT_IN_CONTRAST_THRESHOLD)      # (the built-in scene is smooth: 0.02, not 0.04)
    said = "registered: keypoints %s, %d matches, %d inliers" % ([f["count"] for f in c["feats"]], c["recs"][0]["count"], int(c["stats"][0, 1]))
    assert line[0].startswith(said), (line[0], said)
    assert [f["count"] for f in c["feats"]] == [212, 209] and int(c["stats"][0, 1]) == 154 and os.path.getsize(str(tmp_path / "pano.bmp")) > 480 * 270 * 3


def test_blobs_on_the_gpu_within_the_ground_truth_bounds(gpu):
    """the ground truth of tests/test_sift_model.py asked of the GPU class: one blob, every keypoint at its centre and of a size near 2 s_b,
    within BOUND_FACTOR x the model's recorded errors"""
    import torch
    from test_sift_model import RECORDED_BLOBS
    keys = sorted(cases.BLOBS)
    feats = gpu.SiftFeaturesFinder().find([torch.from_numpy(np.array(cases.image("blob-%d-%d" % k))).cuda() for k in keys])
    for k, f in zip(keys, feats):
        kp, meta, s_b = _np(f.keypoints), _np(f.meta), cases.BLOBS[k]
        assert len(kp) >= 1 and (meta[:, 3] == k[0]).all() and (meta[:, 4] == k[1]).all(), k
        centre, size = float(np.hypot(*(kp - 47.75).T).max()), float(np.abs(meta[:, 0] - 2 * s_b).max() / (2 * s_b))
        print(k, "centre error %.3f px, size error %.3f" % (centre, size))
        assert centre <= P.BOUND_FACTOR * RECORDED_BLOBS[k][0] and size <= P.BOUND_FACTOR * RECORDED_BLOBS[k][1], (k, centre, size)
