"""From pixels to panorama on the GPU against the planted rig of tests/pano_cases.py: views of one texture rendered through known rotations
by plain float64 NumPy, so the ground truth comes from no model of ours (tests/test_pano_model.py holds the NumPy models to it on the CPU).

Registration through the classes - OrbFeaturesFinder(grid=(1, 1), n_features=500).find -> BestOf2NearestMatcher(0.3).match ->
HomographyBasedEstimator -> BundleAdjusterRay / BundleAdjusterReproj -> waveCorrect(adjuster, "horiz") - on device tensors and on NumPy
arrays: at every hand-off the mats the next class reads (last_outputs) equal pano_cases.model_chain's intermediates, each by its own stage's
comparison (np.array_equal on bits for the finder, the matcher, the homography and the estimator; fuzz_*.same for the adjusters and the
wave correction), and the GPU's cameras meet the bounds of the CPU test (2 x pano_cases.MEASURED, measured on the models; the GPU is
bit-equal to them and gets no margin).  Once more with every class on one non-default stream behind a large kernel on the default one, and
rig3_plus_2() in one call with mask= and rigs=[3, 2] against the two rigs run apart.

Composition from the registered cameras - warper at the median focal, warp_with_mask(view, K32, R32) with the wave-corrected cameras,
GainCompensator feed and apply, DpSeamFinder on copies of the masks, feed_dilated(20, 20), FeatherBlender(0.1) / MultiBandBlender(4,
PREC_I16) - for the three projections: every step equals the oracle's on the same inputs (the three-tile tests/test_gpu_end_to_end.py),
warpPoint equals pano_cases.project to 1e-3 px, and the overlap agreement and the error against the texture rendered into the panorama's
frame stay within 1.5 x pano_cases.COMPOSED (measured on the CPU oracle, never on the GPU output).

The example: examples/stitch_pair.py --register --small in a fresh process.

What the file measured on an MI355X is in the commit that added it; every test runs well under 5 s."""
import functools
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
import fuzz_bundle  # noqa: E402
import fuzz_bundle_reproj  # noqa: E402
from fuzz_estimator import same  # noqa: E402
from helpers import bundle_np, estimator_np  # noqa: E402
from test_gpu_bundle import check as check_ray  # noqa: E402
from test_gpu_bundle_reproj import check as check_reproj  # noqa: E402
from test_gpu_estimator import check as check_estimator  # noqa: E402
from test_gpu_wave_correct import check as check_wave  # noqa: E402

pytestmark = pytest.mark.gpu
assert fuzz_bundle.NAMES and fuzz_bundle_reproj.NAMES


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def register(gpu, views, adjuster, where="device", stream=None, mask=None, rigs=None):
    """The classes in order, each reading the one before where its mats lie.  Returns a dict: feats, info, matcher, est_list, adj_list, waved
    and the read-back mats of every last_outputs.  views: NumPy arrays; where: "device" (CUDA tensors) or "host"."""
    import torch
    kw = {} if stream is None else dict(stream=stream)
    if where == "device":
        if stream is None:
            imgs = [torch.from_numpy(v).cuda() for v in views]
        else:
            with torch.cuda.stream(stream):                       # placed on the stream that reads them
                imgs = [torch.from_numpy(v).cuda() for v in views]
    else:
        imgs = list(views)
    finder = gpu.OrbFeaturesFinder(grid=P.ORB_KW["grid"], n_features=P.ORB_KW["n_features"], **kw)
    feats = finder.find(imgs)
    sizes = [f.img_size for f in feats]
    matcher = gpu.BestOf2NearestMatcher(P.MATCH_CONF, **kw)
    info = matcher.match([f.descriptors for f in feats], [f.keypoints for f in feats], sizes, mask=mask)
    est = gpu.HomographyBasedEstimator(**kw)
    est_list = est(sizes, matcher, rigs=rigs)
    ba = (gpu.BundleAdjusterRay if adjuster == "ray" else gpu.BundleAdjusterReproj)(**kw)
    adj_list = ba([f.img_size for f in feats], [f.keypoints for f in feats], matcher, est, rigs=rigs)
    waved = gpu.waveCorrect(ba, "horiz", rigs=rigs, **kw)
    if stream is not None:
        stream.synchronize()
    on_device = where == "device"
    lo = matcher.last_outputs
    for a in [f.keypoints for f in feats] + [f.descriptors for f in feats] + [lo["counts"], lo["H"], lo["stats"], lo["conf"]] + list(lo["matches"]) \
            + list(lo["masks"]) + list(est.last_outputs) + list(ba.last_outputs) + list(waved.last_outputs):
        assert bool(getattr(a, "is_cuda", False)) == on_device, "a hand-off mat is not where the inputs were"
    out = dict(feats=feats, sizes=sizes, info=info, est_list=est_list, adj_list=adj_list, waved=waved, pairs=lo["pairs"],
               counts=_np(lo["counts"]), matches=[_np(m) for m in lo["matches"]], H=_np(lo["H"]), stats=_np(lo["stats"]), conf=_np(lo["conf"]),
               masks=[_np(m) for m in lo["masks"]], est=tuple(_np(a) for a in est.last_outputs), adj=tuple(_np(a) for a in ba.last_outputs),
               wave=tuple(_np(a) for a in waved.last_outputs), same_keypoints=all(a is b.keypoints for a, b in zip(lo["keypoints"], feats)),
               infos=(matcher.last_info, matcher.last_homography_info, est.last_info, ba.last_info, waved.last_info))
    matcher.release()
    est.release()
    ba.release()
    gpu.OrbFeaturesFinder.release()
    return out


def check_hand_offs(got, want, adjuster, what):
    """Every mat a class hands to the next against the model chain `want`, each by its own stage's comparison."""
    for i, (f, w) in enumerate(zip(got["feats"], want["feats"])):                                   # tests/test_gpu_orb.py: check
        n = int(f.keypoints.shape[0])
        assert n == w.count and f.status == w.status, (what, "orb", i, n, w.count)
        assert np.array_equal(_np(f.keypoints), w.keypoints) and np.array_equal(_np(f.descriptors), w.descriptors), (what, "orb", i)
        assert np.array_equal(_np(f.meta).view(np.uint32), w.meta.view(np.uint32).reshape(n, 4)), (what, "orb meta", i)
    assert got["same_keypoints"] and got["sizes"] == want["sizes"]
    assert got["pairs"] == want["pairs"] and np.array_equal(got["counts"][0, :len(want["pairs"])], want["counts"][0]), (what, "pairs, counts")
    for k, (rec, hom, inf) in enumerate(zip(want["recs"], want["hom"], got["info"])):               # tests/test_gpu_match.py, test_gpu_homography.py
        c = rec["count"]
        assert np.array_equal(got["matches"][k][:c], rec["matches"]), (what, "matches", k)
        assert np.array_equal(_np(inf.matches), rec["matches"]), (what, "matches of the MatchesInfo", k)
        assert np.array_equal(_np(inf.src_points), rec["points"][:, 0:2]) and np.array_equal(_np(inf.dst_points), rec["points"][:, 2:4]), (what, "points", k)
        assert np.array_equal(got["stats"][k], hom["stats"]), (what, "stats", k, got["stats"][k], hom["stats"])
        assert np.array_equal(_u64(got["H"][3 * k:3 * k + 3]), _u64(hom["H"])), (what, "H", k)
        assert np.array_equal(_u64(got["conf"][0, k]), _u64(hom["conf"])), (what, "conf", k)
        assert hom["mask"] is not None and np.array_equal(got["masks"][k][:c, 0], hom["mask"]), (what, "inlier mask", k)
        assert inf.num_inliers == int(hom["stats"][1]) and inf.confidence == hom["conf"] and np.array_equal(_u64(inf.H), _u64(hom["H"]))
        assert (inf.src_img_idx, inf.dst_img_idx) == want["pairs"][k]
    check_estimator(got["est"], want["est"], (what, "estimator"))
    (check_ray if adjuster == "ray" else check_reproj)(got["adj"], want[adjuster], (what, adjuster))
    check_wave(got["wave"], want["wave_" + adjuster], (what, "wave"))
    for lst, (cams, kr32) in ((got["est_list"], want["est"][:2]), (got["adj_list"], want[adjuster][:2]), (got["waved"], want["wave_" + adjuster][:2])):
        for i, c in enumerate(lst):                                                                  # what a warper is handed
            assert c.K32.dtype == np.float32 and c.R32.dtype == np.float32
            assert same(c.K32.ravel(), kr32[i, 0:9]) and same(c.R32.ravel(), kr32[i, 9:18]) and c.focal == cams[i, 0] and c.ppx == cams[i, 2]


def check_ground_truth(got, rig, adjuster, measured, first=0, last=None):
    """The GPU's cameras of every stage against the planted rig: the CPU test's bounds."""
    for stage, cams in (("est", got["est"][0]), (adjuster, got["adj"][0]), ("wave_" + adjuster, got["wave"][0])):
        m = P.measure(cams, rig, first, last)
        print(stage, {k: round(v, 4) for k, v in m.items()})
        assert P.within(m, measured[stage]) == [], stage


def check_clean(got, rigs):
    assert (got["conf"] > 1.0).all()
    est = got["est"][3]
    assert (est[:, estimator_np.RIG_STATUS] & (estimator_np.EST_ASSERT | estimator_np.EST_UNREACHED) == 0).all() and est[:, estimator_np.RIG_REACHED].tolist() == rigs
    assert (got["adj"][2][:, bundle_np.RIG_STATUS] == 0).all() and got["wave"][2].tolist() == [[0, n] for n in rigs]
    assert [i[0] for i in got["infos"][2:]] == [len(rigs)] * 3


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("adjuster", ["ray", "reproj"])
def test_registration_through_the_classes(gpu, adjuster, where):
    rig, want = P.rig3(), P.chain3()
    got = register(gpu, rig["views"], adjuster, where)
    assert [int(f.keypoints.shape[0]) for f in got["feats"]] == P.RECORDED["keypoints"][:3]
    assert got["counts"][0].tolist() == P.RECORDED["matches"][:3] and got["stats"][:, 1].tolist() == P.RECORDED["inliers"][:3]
    check_hand_offs(got, want, adjuster, (adjuster, where))
    check_clean(got, [3])
    check_ground_truth(got, rig, adjuster, P.MEASURED["rig3"])


@pytest.mark.parametrize("adjuster", ["ray", "reproj"])
def test_registration_on_a_stream_behind_a_large_kernel_on_the_default_stream(gpu, adjuster):
    """Every class on one non-default stream, the views placed on it, a large unrelated product queued on the default stream first: the
    results are the model's.  This pins results only: were a class to run part of its work on the default stream, or to read a mat before
    the class before had written it, it would race, and a race need not fail."""
    import torch
    rig, want = P.rig3(), P.chain3()
    s = torch.cuda.Stream()
    a = torch.ones((8192, 8192), device="cuda")
    torch.cuda.synchronize()
    for _ in range(10):
        b = a @ a                                                  # the default stream is busy while the chain runs on s
    got = register(gpu, rig["views"], adjuster, "device", stream=s)
    s.synchronize()
    check_hand_offs(got, want, adjuster, (adjuster, "stream"))
    check_ground_truth(got, rig, adjuster, P.MEASURED["rig3"])
    torch.cuda.synchronize()
    assert float(b[0, 0]) == 8192.0 and float(b[-1, -1]) == 8192.0


@pytest.mark.parametrize("adjuster", ["ray", "reproj"])
def test_two_rigs_in_one_call_equal_the_two_rigs_apart(gpu, adjuster):
    """rig3_plus_2(): five views (three of 3 channels, two of 1) in one call of every class with the matcher's mask and rigs=[3, 2]."""
    rig5, want = P.rig3_plus_2(), P.chain3_plus_2()
    got = register(gpu, rig5["views"], adjuster, "device", mask=rig5["mask"], rigs=rig5["rigs"])
    assert got["pairs"] == [(0, 1), (0, 2), (1, 2), (3, 4)]
    assert [int(f.keypoints.shape[0]) for f in got["feats"]] == P.RECORDED["keypoints"] and got["counts"][0].tolist() == P.RECORDED["matches"]
    assert got["stats"][:, 1].tolist() == P.RECORDED["inliers"] and got["conf"][0].tolist() == P.RECORDED["conf"]
    check_hand_offs(got, want, adjuster, (adjuster, "3 + 2"))
    check_clean(got, [3, 2])
    check_ground_truth(got, rig5, adjuster, P.MEASURED["rig3"], 0, 3)
    check_ground_truth(got, rig5, adjuster, P.MEASURED["rig2"], 3, 5)
    at_pair = 0
    for r, n in enumerate(rig5["rigs"]):
        a, b = P.part(rig5, r)
        alone = register(gpu, rig5["views"][a:b], adjuster, "device")
        npairs = len(alone["pairs"])
        for key in ("est", "adj", "wave"):
            for k, (g, w) in enumerate(zip(got[key], alone[key])):
                rows = slice(a, b) if g.shape[0] == 5 else slice(r, r + 1)
                assert g[rows].shape == w.shape and same(g[rows], w), (adjuster, r, key, k)
        assert same(got["H"][3 * at_pair:3 * (at_pair + npairs)], alone["H"]) and np.array_equal(got["stats"][at_pair:at_pair + npairs], alone["stats"])
        assert same(got["conf"][:, at_pair:at_pair + npairs], alone["conf"]) and np.array_equal(got["counts"][:, at_pair:at_pair + npairs], alone["counts"])
        at_pair += npairs


# ---- composition ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def registered(adjuster):
    """The wave-corrected cameras the GPU classes give for rig3() (one registration a process and adjuster, shared, never written to)."""
    import imagestitch_amd as gpu
    return register(gpu, P.rig3()["views"], adjuster, "device")


def _creator(gpu, kind):
    return {"cylindrical": gpu.CylindricalWarper, "spherical": gpu.SphericalWarper, "plane": gpu.PlaneWarper}[kind]


@pytest.mark.parametrize("adjuster", ["ray", "reproj"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_warp_point_is_the_projection_the_measures_use(gpu, kind, adjuster):
    """warper.warpPoint(p, K32, R32) against pano_cases.project, written out in float64, to 1e-3 px on the 12 px grid of every view: the
    formulas that measured the models are the warper's."""
    got = registered(adjuster)
    scale = float(np.median([c.focal for c in got["waved"]]))
    warper = _creator(gpu, kind)().create(scale)
    yy, xx = np.mgrid[0:P.VIEW_H:P.GRID_STEP, 0:P.VIEW_W:P.GRID_STEP]
    pts = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    worst = 0.0
    for c in got["waved"]:
        want = P.project(kind, scale, c.K32.astype(np.float64), c.R32.astype(np.float64), pts)
        have = np.array([warper.warpPoint(p, c.K32, c.R32) for p in pts], np.float64)
        worst = max(worst, float(np.abs(have - want).max()))
    print(kind, adjuster, "warpPoint against the float64 projection: largest difference", worst, "px over", 3 * len(pts), "points")
    assert worst <= 1e-3


@pytest.mark.parametrize("case", P.COMPOSE_CASES + (P.REPROJ_CASE,), ids="-".join)
def test_composition_from_the_registered_cameras(gpu, oracle, case):
    kind, blend, adjuster = case
    rig, got, rec = P.rig3(), registered(adjuster), P.COMPOSED[case]
    waved = got["waved"]
    scale = float(np.median([c.focal for c in waved]))                                   # W:207-216: the warper's scale is the median focal
    assert scale == float(np.median(P.chain3()["wave_" + adjuster][0][:, 0]))
    kr32 = np.stack([np.concatenate([c.K32.ravel(), c.R32.ravel()]) for c in waved])
    warper = _creator(gpu, kind)().create(scale)
    corners, warped, masks = [], [], []
    for v, c in zip(rig["views"], waved):
        tl, wi, wm = warper.warp_with_mask(v, c.K32, c.R32)                              # W:229 + W:232
        corners.append(tuple(tl)); warped.append(wi); masks.append(wm)
    comp = gpu.GainCompensator().feed(corners, warped, masks)                            # W:238-240
    gains = comp.gains()
    want = P.compose_oracle(oracle, rig["views"], kr32, scale, kind, blend, gains=gains)
    assert corners == want["corners"]
    assert all(np.array_equal(a, b) for a, b in zip(warped, want["warped"])) and all(np.array_equal(a, b) for a, b in zip(masks, want["masks"]))
    N, I, _, _, _, g = want["feed_model"]                                                # tests/test_gpu_gain_feed.py: _check
    assert np.array_equal(comp.N, N) and np.array_equal(comp.I.view(np.uint64), I.view(np.uint64))
    np.testing.assert_allclose(gains, g, rtol=1e-12, atol=0)
    for i in range(3):
        comp.apply(i, corners[i], warped[i], masks[i])                                   # W:241-244
        assert np.array_equal(warped[i], want["applied"][i]), i
    seam = [m.copy() for m in masks]                                                     # W:247-249
    gpu.DpSeamFinder().find([a.astype(np.float32) for a in warped], corners, seam)       # W:259-262
    assert all(np.array_equal(a, b) for a, b in zip(seam, want["seam"])) and any((a != b).any() for a, b in zip(seam, masks))
    sizes = [(a.shape[1], a.shape[0]) for a in warped]
    gb = gpu.FeatherBlender(False, 0.1) if blend == "feather" else gpu.MultiBandBlender(False, 4, gpu.PREC_I16)      # W:278-280 / W:271-273
    gb.prepare(corners, sizes)
    for i in range(3):
        assert np.array_equal(gpu.dilate_and(seam[i], 20, 20, other=masks[i]), want["fed"][i])
        gb.feed_dilated(warped[i].astype(np.int16), seam[i], masks[i], 20, 20, corners[i])                           # W:294-302 in one call
    res, rmask = gb.blend()                                                              # W:313
    assert np.array_equal(rmask, want["result_mask"]) and np.array_equal(res, want["result"])
    # the figures: bounds from the CPU oracle's run on the model chain's cameras (pano_cases.COMPOSED), never from this output
    overlap = P.overlap_agreement(corners, warped, masks)
    tl = (min(c[0] for c in corners), min(c[1] for c in corners))
    centre = int(got["est"][3][0, estimator_np.RIG_CENTER0])
    gt, share = P.ground_truth_error(res, rmask, tl, kind, scale, P.alignment(rig, got["wave"][0], centre), rig["texture"])
    print(case, "overlap agreement", overlap, "ground-truth error", gt, "share kept", share)
    assert len(overlap) == 3 and max(v[3] for v in overlap) <= P.COMPOSE_FACTOR * rec["overlap"]
    assert gt <= P.COMPOSE_FACTOR * rec["gt"] and share >= P.MIN_SHARE
    if case in P.COMPOSE_CASES:
        assert gt < 2.0 * rec["gt_planted"] + rec["overlap"]


# ---- the example ------------------------------------------------------------------------------------------------------------------------------
def test_the_example_registers_and_stitches_in_a_fresh_process(gpu, tmp_path, capsys):
    """examples/stitch_pair.py --register --small --out pano.bmp in a child process, as a user starts it: exit status 0, at least 100
    inliers on its output line, and the image it wrote equals the one the same calls write in this process.  (Its two crops differ by a
    translation, which carries no focal: the estimator's is around 7e9, the cylinder flat at that scale, the panorama the scene.)"""
    script = os.path.join(ROOT, "examples", "stitch_pair.py")
    child = str(tmp_path / "pano.bmp")
    run = subprocess.run([sys.executable, script, "--register", "--small", "--out", child], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("registered:")]
    assert len(line) == 1
    inliers = int(line[0].split(" inliers")[0].split()[-1])
    assert inliers >= 100
    spec = importlib.util.spec_from_file_location("stitch_pair_example", script)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    mine = str(tmp_path / "pano_in_process.bmp")
    capsys.readouterr()
    argv = sys.argv
    try:
        sys.argv = [script, "--register", "--small", "--out", mine]
        ex.main()
    finally:
        sys.argv = argv
    said = capsys.readouterr().out
    print(said)
    assert line[0] in said.splitlines()
    a, b = gpu.imread(child), gpu.imread(mine)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[1] > 480 and np.array_equal(a, b)
    with open(child, "rb") as f, open(mine, "rb") as g:
        assert f.read() == g.read()
    gpu.OrbFeaturesFinder.release()
