"""isx_estimate_cameras (imagestitch_amd/cameras.py) on the GPU against the NumPy model of tests/helpers/estimator_np.py: cameras and kr32
through their uint64 / uint32 views, tree and rig_stats with np.array_equal.  The named cases of tests/estimator_cases.py (the demo's 2
images; a chain; complete graphs of 5, 7, 9, 17 and 64 images - either side of a wave, past the 256-thread block, both LDS sorts at full
size; equal weights; two components; the fallback focal; given focals; a singular H), three rigs in one launch, host / device / strided
mats, and the chain matcher -> homography -> estimator on CUDA tensors."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimator_cases as cases  # noqa: E402
import fuzz_estimator as fz  # noqa: E402
from helpers import estimator_np as em  # noqa: E402

pytestmark = pytest.mark.gpu
NAMED = cases.named()
NAMES = ("cameras", "kr32", "tree", "rig_stats")


@functools.lru_cache(maxsize=None)
def model(name):
    c = NAMED[name]
    return em.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"], c["focals_in"])


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind == "f":
        u = np.uint64 if got.dtype == np.float64 else np.uint32
        return np.array_equal(got.view(u), want.view(u))
    return np.array_equal(got, want)


def check(got, want, what, nan_by_position=False):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        ok = fz.same(g, w) if nan_by_position else bits_equal(g, w)
        assert ok, (what, name, np.argwhere(g != w)[:5].tolist(), g, w)


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(gpu, name):
    """Every named case on device mats; the singular H compares NaNs by position and everything else by bits."""
    got, info = fz.run_library(NAMED[name], "device")
    check(got, model(name), name, nan_by_position=name == "singular_H")
    assert info == (1, 1)


def test_three_rigs_in_one_launch_equal_the_three_alone(gpu):
    rigs = [NAMED["demo_2_images_1_pair"], NAMED["complete_5"], NAMED["complete_9"]]
    got, info = fz.run_library(cases.join(rigs), "device")
    assert info == (3, 1)
    at = 0
    for k, r in enumerate(rigs):
        alone, info1 = fz.run_library(r, "device")
        assert info1 == (1, 1)
        m = len(r["sizes"])
        for name, g, a in zip(NAMES[:3], got, alone):
            assert bits_equal(g[at:at + m], a), (k, name)
        assert np.array_equal(got[3][k:k + 1], alone[3]), k
        at += m


@pytest.mark.parametrize("name", ["complete_9", "focals_given", "two_components_5_3"])
def test_host_device_and_strided_mats_give_the_same_bits(gpu, name):
    """Host mats, device mats and mats with a step above a row's bytes (H: 40 bytes a row, not 24)."""
    want = model(name)
    for layout in fz.LAYOUTS:
        got, info = fz.run_library(NAMED[name], layout)
        check(got, want, (name, layout))
        assert info == (1, 1)


def test_the_class_on_host_arrays_and_the_warper_inputs(gpu):
    """HomographyBasedEstimator on the tuple of mats; K32 / R32 are what RotationWarper takes (float32, 3 x 3)."""
    import imagestitch_amd as I
    c = NAMED["complete_5"]
    est = I.HomographyBasedEstimator()
    cams = est(c["sizes"], (c["pairs"], c["H"].reshape(-1, 3), c["stats"], np.zeros((1, len(c["pairs"])))))
    want = model("complete_5")
    assert len(cams) == 5 and np.array_equal(est.last_rig_stats, want[3]) and np.array_equal(cams.rig_stats, want[3]) and est.last_info == (1, 1)
    for i, cam in enumerate(cams):
        assert bits_equal(np.array([cam.focal, cam.aspect, cam.ppx, cam.ppy]), want[0][i, 0:4]) and bits_equal(cam.R.ravel(), want[0][i, 4:13])
        assert cam.K32.dtype == np.float32 and cam.K32.shape == (3, 3) and bits_equal(cam.K32.ravel(), want[1][i, 0:9])
        assert bits_equal(cam.R32.ravel(), want[1][i, 9:18]) and bits_equal(cam.K().astype(np.float32), cam.K32)
        assert (cam.parent, cam.depth) == tuple(want[2][i])
    warper = I.CylindricalWarper().create(float(cams[0].focal))
    roi = warper.warpRoi((c["sizes"][0][0], c["sizes"][0][1]), cams[0].K32, cams[0].R32)
    assert len(roi) == 4 and roi[2] > 0 and roi[3] > 0
    est.release()


def test_the_chain_matcher_homography_estimator_on_cuda_tensors(gpu):
    """The synthetic features of tests/test_gpu_homography.py through BestOf2NearestMatcher, then HomographyBasedEstimator on the device
    mats the matcher left: equal to the model run on the read-back H and stats."""
    import torch
    import imagestitch_amd as I
    from test_gpu_homography import _synthetic_features
    descs, kps, sizes = _synthetic_features(5, [90, 70, 110], 40)
    m = I.BestOf2NearestMatcher()
    infos = m.match([torch.from_numpy(d).cuda() for d in descs], [torch.from_numpy(k).cuda() for k in kps], sizes)
    lo = m.last_outputs
    assert lo["pairs"] == [(i.src_img_idx, i.dst_img_idx) for i in infos] and lo["H"].is_cuda and lo["stats"].is_cuda
    est = I.HomographyBasedEstimator()
    cams = est(sizes, m)
    H, stats = lo["H"].cpu().numpy(), lo["stats"].cpu().numpy()
    assert any(s[0] & 1 for s in stats)
    want = em.estimate(sizes, lo["pairs"], H, stats)
    assert est.last_outputs[0].is_cuda and est.last_info == (1, 1)
    got = tuple(a.cpu().numpy() for a in est.last_outputs)
    check(got, want, "chain")
    assert bits_equal(np.array([c.focal for c in cams]), want[0][:, 0])
    m.release()
    est.release()
