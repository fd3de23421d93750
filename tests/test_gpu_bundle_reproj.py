"""isx_bundle_adjust_reproj (imagestitch_amd/adjuster.py) on the GPU against the model of tests/helpers/bundle_reproj_np.py: cameras and
rig_err through their uint64 views, kr32 through uint32, rig_stats with np.array_equal.  The named cases of tests/bundle_reproj_cases.py -
those of the Ray adjuster that exercise the shared control flow (max_iter 1, 2, 3; a pair at conf == conf_thresh; a camera and a rig without
an edge; the estimator's assert bit; a NaN focal; a count above its mat's rows; indices outside the keypoints; a singular R; pairs in another
order; two runs to their natural end) and the shapes where the new constants can go wrong: 2 images with 8 inliers (14 unknowns, 16 rows),
edges around the tile of the accumulation, a chain of 37 images (259 unknowns: past 256 rows and four waves), 528 tiles (more than the block
has threads), a chain of 64 images (448 unknowns, against outputs of the model recorded in tests/golden), refine_flags 0, 1 and 31, a z of
0, the rigs that go round of bundle_cases.WIDE (112 unknowns for 16 cameras) - then three rigs in one launch (narrow ones; a ring, a narrow
rig and an exact half turn), host / device / strided mats, the chain matcher -> homography -> estimator -> BundleAdjusterReproj ->
waveCorrect on CUDA tensors, and the ring of 8 from the estimator through the adjuster to both kinds of wave correction."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_reproj_cases as cases  # noqa: E402
import fuzz_bundle_reproj as fz  # noqa: E402
from helpers import bundle_reproj_np as rp  # noqa: E402

pytestmark = pytest.mark.gpu
NAMED = cases.named()
NAMES = fz.NAMES
PASS_THROUGH = {"rig_without_edge": rp.ST_NO_EDGES, "estimator_assert_bit": rp.ST_EST_ASSERT, "nan_focal_in": rp.ST_NAN}
GOLDEN = os.path.join(ROOT, "tests", "golden", "bundle_reproj_chain64.npz")


@functools.lru_cache(maxsize=None)
def model(name):
    return fz.run_model(NAMED[name])


def check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert fz.same(g, w), (what, name, np.argwhere(g != w)[:5].tolist(), g, w)


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(gpu, name):
    """Every named case on device mats, by bits (NaNs by position)."""
    c = NAMED[name]
    got, info = fz.run_library(c, "device")
    want = model(name)
    check(got, want, name)
    assert info == (1, 1)
    st = int(got[2][0, rp.RIG_STATUS])
    if name in PASS_THROUGH:                                   # cameras_out equals cameras_in
        assert st & PASS_THROUGH[name] and fz.same(got[0], c["cameras_in"])
    elif name != "z_zero":
        assert not np.isnan(got[0]).any() and got[2][0, rp.RIG_ITERS] >= 1
    if name.startswith("max_iter_"):
        assert got[2][0, rp.RIG_ITERS] == c["max_iter"]
    if name.startswith("natural_end"):
        assert got[2][0, rp.RIG_ITERS] < 1000 and got[3][0, 1] < got[3][0, 0] / 100.0
    if name == "conf_equal_thresh_is_excluded":
        assert got[2][0, rp.RIG_EDGES] == 2
    if name == "two_images_8_inliers":
        assert got[2][0, rp.RIG_MATCHES] == 8
    if name == "tiles_5":
        assert sorted(int(m.sum()) for m in c["masks"]) == sorted([cases.TILE - 1, cases.TILE, cases.TILE + 1, 2 * cases.TILE + 1, 5, 2 * cases.TILE])
    if name == "camera_without_edge":
        assert st & rp.ST_DROPPED and fz.same(got[0][3, 0:4], c["cameras_in"][3, 0:4])
    if name == "count_above_rows":
        assert got[2][0, rp.RIG_EDGES] == 3 and got[2][0, rp.RIG_MATCHES] == int(c["masks"][0].sum() + c["masks"][1].sum())
    if name == "chain_37":
        assert len(c["sizes"]) * rp.PC == 259
    if name == "tiles_past_a_block":
        assert got[2][0, rp.RIG_MATCHES] == 528 and got[2][0, rp.RIG_EDGES] == 528
    if name == "refine_flags_0":                               # nothing but the rotations moves
        assert st & rp.ST_DROPPED and fz.same(got[0][:, 0:4], c["cameras_in"][:, 0:4]) and got[3][0, 1] < got[3][0, 0]
    if name == "refine_flags_1":                               # the focal moves, ppx, ppy and aspect stay
        assert st & rp.ST_DROPPED and fz.same(got[0][:, 1:4], c["cameras_in"][:, 1:4]) and not (got[0][:, 0] == c["cameras_in"][:, 0]).any()
    if name == "refine_flags_31":
        assert not (got[0][:, 0:4] == c["cameras_in"][:, 0:4]).any()
    if name == "z_zero":                                       # NaN residuals: every pivot drops, the step is 0, the error norms are NaN
        assert np.isnan(got[3]).all() and st & rp.ST_DROPPED and got[0][0, 0] == 0.0
    if name in cases.WIDE:
        check_wide(name, c, got)


def check_wide(name, c, got):
    """What a rig that goes round shows beyond its bits: it does not pass through, every edge has its 12 inliers, all four intrinsics moved."""
    st, centre = int(got[2][0, rp.RIG_STATUS]), int(c["est_rig_stats"][0, 2])
    assert st & (rp.ST_NAN | rp.ST_NO_EDGES | rp.ST_EST_ASSERT | rp.ST_SINGULAR_R) == 0
    assert got[2][0, rp.RIG_EDGES] == len(c["pairs"]) and got[2][0, rp.RIG_MATCHES] == 12 * len(c["pairs"])
    assert not (got[0][:, 0:4] == c["cameras_in"][:, 0:4]).any() and got[3][0, 1] < got[3][0, 0]
    if name.startswith("ring_8x45"):
        assert (0, 7) in c["pairs"] and len(c["pairs"]) == 8 and got[2][0, rp.RIG_ITERS] == c["max_iter"] and got[3][0, 1] < got[3][0, 0] / 1000.0
        far = got[0][(centre + 4) % 8, 4:13].reshape(3, 3)     # half a turn from the centre: 1 + 2 cos(theta) is near -1
        assert np.trace(far) < -0.9 and np.abs(got[0][centre, 4:13] - np.eye(3).ravel()).max() <= 1e-6
    if name == "ring_8x45_center_4":
        assert centre == 4
    if name == "ring_8x45_exact_half_turn":
        assert np.array_equal(np.diag(c["cameras_in"][4, 4:13].reshape(3, 3)), [-1.0, 1.0, -1.0]) and np.array_equal(c["cameras_in"][0, 4:13], np.eye(3).ravel())
    if name == "ring_6x60_center_0":
        assert (0, 5) in c["pairs"] and got[2][0, rp.RIG_ITERS] == 4
    if name == "arc_5x50_natural_end":
        assert (0, 4) not in c["pairs"] and 6 < got[2][0, rp.RIG_ITERS] < 1000 and got[3][0, 1] < got[3][0, 0] / 100.0
    if name == "reflection_R_in":
        assert np.linalg.det(c["cameras_in"][1, 4:13].reshape(3, 3)) < -0.9
    if name == "ring_16x22p5_two_steps":
        assert rp.PC * len(c["sizes"]) == 112 and len(c["pairs"]) == 32 and got[2][0, rp.RIG_ITERS] == 2


def test_a_ring_a_narrow_rig_and_the_exact_half_turn_in_one_launch(gpu):
    """Three blocks of one launch, of which two take branches of bundle_math.hpp that the narrow one between them never does: each rig
    equals its run alone and the model."""
    rigs = [NAMED["ring_8x45_center_4"], NAMED["max_iter_3"], NAMED["ring_8x45_exact_half_turn"]]
    assert all(r["max_iter"] == 3 and r["conf_thresh"] == 1.0 and r["refine_flags"] == 31 for r in rigs)
    joined = dict(cases.join(rigs), refine_flags=31)
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


def test_chain_64_against_the_recorded_model(gpu):
    """448 unknowns, a row of the Cholesky per thread of seven waves, against the model's outputs recorded once by
    tests/golden/make_golden_bundle_reproj.py (the largest system the entry takes is not solved in Python in every run of the suite)."""
    g = np.load(GOLDEN)
    c = cases.chain_64()
    assert len(c["sizes"]) * rp.PC == 448 and c["max_iter"] == int(g["max_iter"]) == 1
    assert fz.same(c["cameras_in"], g["cameras_in"]) and all(fz.same(a, g["keypoints_%d" % i]) for i, a in enumerate(c["keypoints"][:3]))
    got, info = fz.run_library(c, "device")
    check(got, tuple(g[k] for k in NAMES), "chain_64")
    assert info == (1, 1) and got[2][0, rp.RIG_ITERS] == 1 and not np.isnan(got[0]).any()


def test_three_rigs_in_one_launch_equal_the_three_alone(gpu):
    rigs = [NAMED["max_iter_3"], NAMED["two_images_8_inliers"], NAMED["camera_without_edge"]]
    rigs = [dict(r, max_iter=3) for r in rigs]
    joined = dict(cases.join(rigs), refine_flags=31)
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
    check(got, fz.run_model(joined), "three rigs")


@pytest.mark.parametrize("name", ["tiles_5", "camera_without_edge", "pairs_in_another_order"])
def test_host_device_and_strided_mats_give_the_same_bits(gpu, name):
    want = model(name)
    for layout in fz.LAYOUTS:
        got, info = fz.run_library(NAMED[name], layout)
        check(got, want, (name, layout))
        assert info == (1, 1)


def ring_chain_inputs():
    """The ring of 8 cameras 45 degrees apart as the homography stage would leave it: (case, H of its pairs stacked 3 k x 3) with H the
    planted K R_j^T R_i K^-1 / h22 of estimator_cases.homography."""
    import estimator_cases as EC
    c = NAMED["ring_8x45_center_0"]
    focal, Rs = c["planted"][:2]
    return c, np.concatenate([EC.homography(Rs[i], Rs[j], focal) for i, j in c["pairs"]])


def test_the_ring_from_the_estimator_to_both_wave_corrections_on_cuda_tensors(gpu):
    """HomographyBasedEstimator on the planted homographies of the ring, BundleAdjusterReproj on its cameras - which reach half a turn from
    the centre - and waveCorrect of both kinds on the adjuster's, every mat on the device, four launches in stream order with no
    synchronisation: each equal to its model fed the read-back mats."""
    import torch
    from helpers import estimator_np as EM
    from imagestitch_amd import adjuster as adj
    from imagestitch_amd import cameras as cam
    from test_gpu_estimator import check as check_estimator
    c, H = ring_chain_inputs()
    n, pairs, dev = len(c["sizes"]), c["pairs"], dict(device="cuda")
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    kps, ms, mk = [put(k) for k in c["keypoints"]], [put(m) for m in c["matches"]], [put(m) for m in c["masks"]]
    counts, stats, conf, Hd = put(c["counts"]), put(c["stats"]), put(c["conf"]), put(H)
    est = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
           torch.empty((n, 2), dtype=torch.int32, **dev), torch.empty((1, 8), dtype=torch.int32, **dev))
    outs = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
            torch.empty((1, 8), dtype=torch.int32, **dev), torch.empty((1, 2), dtype=torch.float64, **dev))
    waves = [(torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev), torch.empty((1, 2), dtype=torch.int32, **dev))
             for _ in range(2)]
    torch.cuda.synchronize()
    cam.estimate_cameras(c["sizes"], pairs, Hd, stats, conf, *est)                          # four launches in stream order, nothing in between
    info = adj.bundle_adjust_reproj(c["sizes"], kps, pairs, ms, mk, counts, stats, conf, est[3], est[0], *outs, conf_thresh=1.0, max_iter=3)
    winfo = [adj.wave_correct(outs[0], *w, kind=kind) for w, kind in zip(waves, (adj.WAVE_CORRECT_HORIZ, adj.WAVE_CORRECT_VERT))]
    torch.cuda.synchronize()
    assert info == (1, 1) and winfo == [(1, 1), (1, 1)]
    got_est = tuple(a.cpu().numpy() for a in est)
    check_estimator(got_est, EM.estimate(c["sizes"], pairs, H, c["stats"]), "ring: estimator")
    turns = [np.trace(R.reshape(3, 3)) / np.cbrt(np.linalg.det(R.reshape(3, 3))) for R in got_est[0][:, 4:13]]      # 1 + 2 cos(theta): R comes scaled
    assert min(turns) < -0.9 and got_est[3][0, 0] & (EM.EST_ASSERT | EM.EST_UNREACHED) == 0             # a camera half a turn from the centre
    want = rp.adjust(c["sizes"], c["keypoints"], pairs, c["matches"], c["masks"], c["counts"], c["conf"], got_est[3], got_est[0], None, 1.0, 3)
    got = tuple(a.cpu().numpy() for a in outs)
    check(got, want, "ring: adjuster")
    assert got[2][0, rp.RIG_STATUS] & ~rp.ST_DROPPED == 0 and got[2][0, rp.RIG_ITERS] == 3 and got[3][0, 1] < got[3][0, 0]
    for w, kind in zip(waves, (rp.WAVE_HORIZ, rp.WAVE_VERT)):
        wwant = rp.wave_correct(got[0], None, kind)
        for g, m in zip((a.cpu().numpy() for a in w), wwant):
            assert g.dtype == m.dtype and fz.same(g, m), kind
        assert wwant[2][0].tolist() == [0, n]
    assert not fz.same(waves[0][0].cpu().numpy(), waves[1][0].cpu().numpy())


def test_the_chain_to_the_wave_correction_on_cuda_tensors(gpu):
    """The synthetic features of tests/test_gpu_homography.py through BestOf2NearestMatcher, HomographyBasedEstimator, BundleAdjusterReproj and
    waveCorrect, each on the device mats the one before left, no host mat and no synchronisation between the five launches: equal to the
    models fed the read-back mats."""
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
    wouts = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev), torch.empty((1, 2), dtype=torch.int32, **dev))
    torch.cuda.synchronize()
    mt.match_features(d_dev, pairs, 0.3, ms, counts, k_dev, sizes, ps)                     # five launches in stream order, nothing in between
    hg.find_homography(ps, counts, H, mk, stats, conf)
    cam.estimate_cameras(sizes, pairs, H, stats, conf, cams, kr, tree, ers)
    info = adj.bundle_adjust_reproj(sizes, k_dev, pairs, ms, mk, counts, stats, conf, ers, cams, *outs, conf_thresh=1.0, max_iter=20)
    winfo = adj.wave_correct(outs[0], *wouts, kind=adj.WAVE_CORRECT_HORIZ)
    torch.cuda.synchronize()
    assert info == (1, 1) and winfo == (1, 1)
    host = [a.cpu().numpy() for a in (counts, conf, ers, cams)]
    assert (host[1] > 1.0).sum() >= 2
    want = rp.adjust(sizes, kps, pairs, [m.cpu().numpy() for m in ms], [m.cpu().numpy() for m in mk], *host, None, 1.0, 20)
    got = tuple(a.cpu().numpy() for a in outs)
    check(got, want, "chain")
    assert got[2][0, rp.RIG_STATUS] & ~rp.ST_DROPPED == 0 and got[2][0, rp.RIG_ITERS] >= 1 and got[3][0, 1] < got[3][0, 0]
    wwant = rp.wave_correct(want[0], None, rp.WAVE_HORIZ)
    for g, w in zip((a.cpu().numpy() for a in wouts), wwant):
        assert g.dtype == w.dtype and fz.same(g, w)
    assert wwant[2][0].tolist() == [0, n]
    # the classes: the adjuster reads the matcher's and the estimator's last_outputs where they lie, waveCorrect the adjuster's
    m = I.BestOf2NearestMatcher()
    m.match(d_dev, k_dev, sizes)
    est = I.HomographyBasedEstimator()
    est(sizes, m)
    ba = I.BundleAdjusterReproj(max_iter=20)
    ba.setConfThresh(1.0)
    ba.setRefinementMask(np.array([[1, 1, 1], [0, 1, 1], [0, 0, 0]], np.uint8))
    assert ba.refine_flags == 31
    refined = ba(sizes, k_dev, m, est)
    assert all(a.is_cuda for a in ba.last_outputs) and ba.last_info == (1, 1)
    check(tuple(a.cpu().numpy() for a in ba.last_outputs), want, "classes")
    assert len(refined) == n and np.array_equal(refined.rig_stats, want[2]) and np.array_equal(ba.last_rig_err, want[3])
    waved = I.waveCorrect(ba, "horiz")
    assert all(a.is_cuda for a in waved.last_outputs) and waved.last_info == (1, 1) and np.array_equal(waved.rig_stats, wwant[2])
    for i, c in enumerate(waved):
        assert c.focal == want[0][i, 0] and c.ppx == want[0][i, 2] and np.array_equal(c.R32, wwant[1][i, 9:18].reshape(3, 3)) and c.R32.dtype == np.float32
        assert np.array_equal(np.asarray(c.R).ravel(), wwant[0][i, 4:13])
    again = I.waveCorrect(refined, I.WAVE_CORRECT_HORIZ)                 # a CameraList: host mats
    assert all(np.array_equal(a.R32, b.R32) for a, b in zip(again, waved))
    m.release()
    est.release()
    ba.release()
