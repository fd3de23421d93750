"""isx_bundle_adjust_ray (imagestitch_amd/adjuster.py) on the GPU against the model of tests/helpers/bundle_np.py: cameras and rig_err
through their uint64 views, kr32 through uint32, rig_stats with np.array_equal.  The named cases of tests/bundle_cases.py (2 images with 8
inliers; max_iter 1, 2, 3; a pair at conf == conf_thresh; edges one fewer, exactly and one more inlier than the tile of the accumulation with
zeros interleaved in the masks; a camera and a rig without an edge; the estimator's assert bit; a NaN focal; a count above its mat's rows;
indices outside the keypoints; a singular R; pairs in another order; a chain of 64 images - 256 parameters, the block's size; 276 edges - more tiles than the block has threads; two runs to
their natural end; the rigs that go round of bundle_cases.WIDE - rings of 8, 6 and 16 cameras, an arc, an exact half turn, a mirrored R - which
take the branches of csrc/bundle_math.hpp that no narrow rig does), three rigs in one launch - narrow ones, and a ring, a narrow rig and the half turn -, host / device / strided mats, and the chain matcher -> homography -> estimator -> adjuster on CUDA
tensors."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_cases as cases  # noqa: E402
import fuzz_bundle as fz  # noqa: E402
from helpers import bundle_np as bm  # noqa: E402

pytestmark = pytest.mark.gpu
NAMED = cases.named()
NAMES = fz.NAMES
PASS_THROUGH = {"rig_without_edge": bm.ST_NO_EDGES, "estimator_assert_bit": bm.ST_EST_ASSERT, "nan_focal_in": bm.ST_NAN}


@functools.lru_cache(maxsize=None)
def model(name):
    return fz.run_model(NAMED[name])


def check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert fz.same(g, w), (what, name, np.argwhere(g != w)[:5].tolist(), g, w)


def check_wide(name, c, got):
    """What a rig that goes round shows beyond its bits: it does not pass through, every edge has its 12 inliers, the focals moved."""
    st, centre = int(got[2][0, bm.RIG_STATUS]), int(c["est_rig_stats"][0, 2])
    assert st & (bm.ST_NAN | bm.ST_NO_EDGES | bm.ST_EST_ASSERT | bm.ST_SINGULAR_R) == 0
    assert got[2][0, bm.RIG_EDGES] == len(c["pairs"]) and got[2][0, bm.RIG_MATCHES] == 12 * len(c["pairs"])
    assert not (got[0][:, 0] == c["cameras_in"][:, 0]).any()
    if name.startswith("ring_8x45"):
        assert (0, 7) in c["pairs"] and len(c["pairs"]) == 8 and got[2][0, bm.RIG_ITERS] == c["max_iter"] and got[3][0, 1] < got[3][0, 0] / 1000.0
        far = got[0][(centre + 4) % 8, 4:13].reshape(3, 3)     # half a turn from the centre: 1 + 2 cos(theta) is near -1
        assert np.trace(far) < -0.9 and np.abs(got[0][centre, 4:13] - np.eye(3).ravel()).max() <= 1e-6
    if name == "ring_8x45_center_4":
        assert centre == 4
    if name == "ring_8x45_exact_half_turn":
        assert np.array_equal(np.diag(c["cameras_in"][4, 4:13].reshape(3, 3)), [-1.0, 1.0, -1.0]) and np.array_equal(c["cameras_in"][0, 4:13], np.eye(3).ravel())
    if name == "ring_6x60_center_0":
        assert (0, 5) in c["pairs"] and got[2][0, bm.RIG_ITERS] == 4 and got[3][0, 1] < got[3][0, 0] / 1000.0
    if name == "arc_5x50_natural_end":
        assert (0, 4) not in c["pairs"] and 1 < got[2][0, bm.RIG_ITERS] < 1000 and got[3][0, 1] < got[3][0, 0] / 100.0
    if name == "reflection_R_in":
        assert np.linalg.det(c["cameras_in"][1, 4:13].reshape(3, 3)) < -0.9
    if name == "ring_16x22p5_two_steps":
        assert 4 * len(c["sizes"]) == 64 and len(c["pairs"]) == 32 and got[2][0, bm.RIG_ITERS] == 2


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(gpu, name):
    """Every named case on device mats, by bits (NaNs, which only the NaN focal carries, by position)."""
    c = NAMED[name]
    got, info = fz.run_library(c, "device")
    want = model(name)
    check(got, want, name)
    assert info == (1, 1)
    if name in PASS_THROUGH:                                   # cameras_out equals cameras_in
        assert got[2][0, bm.RIG_STATUS] & PASS_THROUGH[name] and fz.same(got[0], c["cameras_in"])
    else:
        assert not np.isnan(got[0]).any() and got[2][0, bm.RIG_ITERS] >= 1
    if name.startswith("max_iter_"):
        assert got[2][0, bm.RIG_ITERS] == c["max_iter"]
    if name.startswith("natural_end"):
        assert got[2][0, bm.RIG_ITERS] < 1000 and got[3][0, 1] < got[3][0, 0] / 100.0
    if name == "conf_equal_thresh_is_excluded":
        assert got[2][0, bm.RIG_EDGES] == 2
    if name == "tiles_5":
        assert sorted(int(m.sum()) for m in c["masks"]) == sorted([cases.TILE - 1, cases.TILE, cases.TILE + 1, 2 * cases.TILE + 1, 5, 2 * cases.TILE])
        assert all(0 in m and m.shape[0] > int(m.sum()) for m in c["masks"][:4])
    if name == "camera_without_edge":
        assert got[2][0, bm.RIG_STATUS] == bm.ST_DROPPED and got[0][3, 0] == c["cameras_in"][3, 0]
    if name == "count_above_rows":
        assert got[2][0, bm.RIG_EDGES] == 3 and got[2][0, bm.RIG_MATCHES] == int(c["masks"][0].sum() + c["masks"][1].sum())
    if name in cases.WIDE:
        check_wide(name, c, got)


def test_a_ring_a_narrow_rig_and_the_exact_half_turn_in_one_launch(gpu):
    """Three blocks of one launch, of which two take branches of bundle_math.hpp that the narrow one between them never does: each rig
    equals its run alone and the model."""
    rigs = [NAMED["ring_8x45_center_4"], NAMED["max_iter_3"], NAMED["ring_8x45_exact_half_turn"]]
    assert all(r["max_iter"] == 3 and r["conf_thresh"] == 1.0 for r in rigs)
    joined = cases.join(rigs)
    got, info = fz.run_library(joined, "device")
    assert info == (3, 1)
    at = 0
    for k, r in enumerate(rigs):
        alone, info1 = fz.run_library(r, "device")
        assert info1 == (1, 1)
        m = len(r["sizes"])
        assert fz.same(got[0][at:at + m], alone[0]) and fz.same(got[1][at:at + m], alone[1]), k
        assert np.array_equal(got[2][k:k + 1], alone[2]) and fz.same(got[3][k:k + 1], alone[3]), k
        at += m
    check(got, fz.run_model(joined), "ring, narrow, half turn")


def test_three_rigs_in_one_launch_equal_the_three_alone(gpu):
    rigs = [NAMED["max_iter_3"], NAMED["two_images_8_inliers"], NAMED["camera_without_edge"]]
    rigs = [dict(r, max_iter=3) for r in rigs]
    got, info = fz.run_library(cases.join(rigs), "device")
    assert info == (3, 1)
    at = 0
    for k, r in enumerate(rigs):
        alone, info1 = fz.run_library(r, "device")
        assert info1 == (1, 1)
        m = len(r["sizes"])
        assert fz.same(got[0][at:at + m], alone[0]) and fz.same(got[1][at:at + m], alone[1]), k
        assert np.array_equal(got[2][k:k + 1], alone[2]) and fz.same(got[3][k:k + 1], alone[3]), k
        at += m
    check(got, fz.run_model(cases.join(rigs)), "three rigs")


@pytest.mark.parametrize("name", ["tiles_5", "camera_without_edge", "pairs_in_another_order"])
def test_host_device_and_strided_mats_give_the_same_bits(gpu, name):
    """Host mats, device mats and mats with a step above a row's bytes (matches: 20 bytes a row, not 12; masks: 3, not 1)."""
    want = model(name)
    for layout in fz.LAYOUTS:
        got, info = fz.run_library(NAMED[name], layout)
        check(got, want, (name, layout))
        assert info == (1, 1)


def test_the_chain_matcher_homography_estimator_adjuster_on_cuda_tensors(gpu):
    """The synthetic features of tests/test_gpu_homography.py through BestOf2NearestMatcher, HomographyBasedEstimator and BundleAdjusterRay,
    each on the device mats the one before left, with no synchronisation between the four stages' launches: equal to the model fed the
    read-back mats."""
    import torch
    import imagestitch_amd as I
    from imagestitch_amd import adjuster as adj
    from imagestitch_amd import cameras as cam
    from imagestitch_amd import homography as hg
    from imagestitch_amd import matcher as mt
    from test_gpu_homography import _synthetic_features
    descs, kps, sizes = _synthetic_features(5, [90, 70, 110], 40)
    n = len(descs)
    d_dev, k_dev = [torch.from_numpy(d).cuda() for d in descs], [torch.from_numpy(k).cuda() for k in kps]
    rows = [d.shape[0] for d in descs]
    pairs = I.FeaturesMatcher.near_pairs(rows)
    cap = [rows[i] + rows[j] for i, j in pairs]
    dev = dict(device="cuda")
    ms = [torch.empty((c, 3), dtype=torch.int32, **dev) for c in cap]
    ps = [torch.empty((c, 4), dtype=torch.float32, **dev) for c in cap]
    mk = [torch.zeros((c, 1), dtype=torch.uint8, **dev) for c in cap]
    counts = torch.empty((1, len(pairs)), dtype=torch.int32, **dev)
    H, stats, conf = (torch.empty((3 * len(pairs), 3), dtype=torch.float64, **dev), torch.empty((len(pairs), 8), dtype=torch.int32, **dev),
                      torch.empty((1, len(pairs)), dtype=torch.float64, **dev))
    cams, kr, tree, ers = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
                           torch.empty((n, 2), dtype=torch.int32, **dev), torch.empty((1, 8), dtype=torch.int32, **dev))
    outs = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
            torch.empty((1, 8), dtype=torch.int32, **dev), torch.empty((1, 2), dtype=torch.float64, **dev))
    torch.cuda.synchronize()
    mt.match_features(d_dev, pairs, 0.3, ms, counts, k_dev, sizes, ps)                     # four launches in stream order, nothing in between
    hg.find_homography(ps, counts, H, mk, stats, conf)
    cam.estimate_cameras(sizes, pairs, H, stats, conf, cams, kr, tree, ers)
    info = adj.bundle_adjust_ray(sizes, k_dev, pairs, ms, mk, counts, stats, conf, ers, cams, *outs, conf_thresh=1.0, max_iter=20)
    torch.cuda.synchronize()
    assert info == (1, 1)
    host = [a.cpu().numpy() for a in (counts, conf, ers, cams)]
    assert (host[1] > 1.0).sum() >= 2
    want = bm.adjust(sizes, kps, pairs, [m.cpu().numpy() for m in ms], [m.cpu().numpy() for m in mk], *host, None, 1.0, 20)
    got = tuple(a.cpu().numpy() for a in outs)
    check(got, want, "chain")
    assert got[2][0, bm.RIG_STATUS] & ~bm.ST_DROPPED == 0 and got[2][0, bm.RIG_ITERS] >= 1 and got[3][0, 1] < got[3][0, 0]
    # the classes: the adjuster reads the matcher's and the estimator's last_outputs where they lie
    m = I.BestOf2NearestMatcher()
    m.match(d_dev, k_dev, sizes)
    est = I.HomographyBasedEstimator()
    est(sizes, m)
    ba = I.BundleAdjusterRay(max_iter=20)
    ba.setConfThresh(1.0)
    refined = ba(sizes, k_dev, m, est)
    assert all(a.is_cuda for a in ba.last_outputs) and ba.last_info == (1, 1)
    check(tuple(a.cpu().numpy() for a in ba.last_outputs), want, "classes")
    assert len(refined) == n and np.array_equal(refined.rig_stats, want[2]) and np.array_equal(ba.last_rig_err, want[3])
    for i, c in enumerate(refined):
        assert c.focal == want[0][i, 0] and np.array_equal(c.R32, want[1][i, 9:18].reshape(3, 3)) and c.R32.dtype == np.float32
    m.release()
    est.release()
    ba.release()
