"""The host plumbing of the per-thread stages (imagestitch_amd/csrc/scratch.hpp and the stages that use it), pinned in three parts.

1. Decisions against a recorded fixture (tests/golden/stage_scratch.json, recorded from the commit before scratch.hpp existed; the
   estimator's entries - estimator-dev, -host, -mixed and -errors - from the commit before StagedMat existed, the last one that spelt every
   staged mat out by hand).  For a fixed set of calls of isx_match_features, isx_find_homography, isx_estimate_cameras (the host / device
   cases of its own suite and three rigs in one call; every mat on the device, on the host, and alternating), the graph-cut and Voronoi
   seam finders, the gain feed, isx_seam_estimate_cost, isx_blend_pair_linear and the first BlocksGainCompensator apply, the fixture holds
   per step the launches per launch name, their summed algorithmic bytes (isx_profile_*) and the `info` outputs.  Launches must match
   exactly, bytes to a relative 1e-9 (see tests/test_gpu_warp_plan.py).  Every output is also compared with the model or oracle its own suite uses.  The graph cut's sweeps
   (SWEEPS below) are the exception: how many rounds push-relabel needs depends on the order in which the nodes of one launch see each
   other's pushes - two calls leave different residuals (tests/test_gpu_graphcut_grad.py) - so the host decides their number from
   counters it reads back, not from its arguments.  They are recorded with a count of -1 and the bytes of one launch, as is any other
   launch name whose count differed between the recorder's two passes (none did).  The graph cut's build, check, certificate and
   write-back launches are pinned exactly, like everything else.
   isx_seam_estimate_cost: the LDS route of its DP only - the global route needs more than 15 360 cells per step, which
   tests/test_gpu_seam.py::test_seam_step_longer_than_lds reaches with a 16 500-pixel tile.

2. The cross-stream fence and the pinned upload buffer in use: two different problems at once on two streams with no host synchronisation
   in between, a call with device mats followed at once by one with host mats (which refills the pinned buffer the first call's upload
   reads), and big / small / release() sequences - for the matcher, the homography, the matcher-then-homography chain, the estimator,
   and the three entries that carve one BaScratch: BundleAdjusterRay, BundleAdjusterReproj, the wave correction and the three in
   cv::Stitcher's order, each on the cameras of the one before; those three also back to back on three streams, and from two threads,
   which have a scratch each.  These pin RESULTS only: a missing fence or a pinned buffer rewritten too early is a race, and a race need not fail on any given run.

3. The full message of every refused call that test_errors_leave_the_outputs_untouched of the matcher's and the homography's suites
   lists, and of every one that _refusals() of tests/test_gpu_estimator_guard.py lists plus its capturing stream, against the fixture.

    python tests/test_gpu_stage_scratch.py --record      # rewrites the fixture from the library as built (on a GPU)
"""
import ctypes as C
import functools
import gc
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tools")):      # (run as a script too: --record)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bundle_cases as BC  # noqa: E402
import bundle_reproj_cases as BRC  # noqa: E402
import estimator_cases as EC  # noqa: E402
import homography_cases as HC  # noqa: E402
import match_cases as MC  # noqa: E402
from helpers import blocks_gain_np as BGM  # noqa: E402
from helpers import bundle_np as BM  # noqa: E402
from helpers import bundle_reproj_np as BRP  # noqa: E402
from helpers import dpseam_grad_np as DPG  # noqa: E402
from helpers import estimator_np as EM  # noqa: E402
from helpers import graphcut_grad_np as GG  # noqa: E402
from helpers import graphcut_np as G  # noqa: E402
from helpers import homography_np as HM  # noqa: E402
from helpers import match_np as MM  # noqa: E402
from helpers import voronoi_np as V  # noqa: E402
from seam_cases import make_case  # noqa: E402
from test_gpu_warp_plan import BYTES_RTOL, _Rec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_scratch.json")
S_I, S_F, S_B = -7777, -7777.25, 0xA5      # what the outputs hold before a call
SWEEPS = ("graphcut_bfs", "graphcut_bfs_init", "graphcut_count", "graphcut_push", "graphcut_relabel")
NAMED = HC.named()
ENAMED = EC.named()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _sync():
    import torch
    torch.cuda.synchronize()


def _placer(where):
    """put(array, k): a device tensor or a host copy - all of one kind, or alternating with k ("mixed")"""
    def put(a, k=0):
        dev = where == "dev" or (where == "mixed" and k % 2 == 0)
        return _dev(a) if dev else np.array(a)
    return put


# ---- the matcher: a call that does not synchronise, and its outputs read afterwards -------------------------------------------------------
def mt_prepare(descs, pairs, conf=0.3, kps=None, sizes=None, where="dev", knn=True):
    put = _placer(where)
    cap = [descs[i].shape[0] + descs[j].shape[0] for i, j in pairs]
    b = dict(pairs=list(pairs), conf=conf, sizes=sizes)
    b["m"] = [put(np.full((n, 3), S_I, np.int32), k) for k, n in enumerate(cap)]
    b["p"] = [put(np.full((n, 4), S_I, np.float32), k + 1) for k, n in enumerate(cap)] if kps is not None else None
    b["k"] = [put(np.full((descs[p[d]].shape[0], 4), S_I, np.int32), k + d) for k, p in enumerate(pairs) for d in range(2)] if knn else None
    b["c"] = put(np.full((1, max(len(pairs), 1)), S_I, np.int32), 1)
    b["d"] = [put(d, k) for k, d in enumerate(descs)]
    b["kp"] = None if kps is None else [put(kp, k + 1) for k, kp in enumerate(kps)]
    return b


def mt_run(b, stream=None):
    from imagestitch_amd import matcher
    b["info"] = matcher.match_features(b["d"], b["pairs"], b["conf"], b["m"], b["c"], b["kp"], b["sizes"], b["p"], b["k"], 0, stream)
    return b


def mt_call(descs, pairs, conf=0.3, kps=None, sizes=None, where="dev", knn=True, stream=None):
    b = mt_prepare(descs, pairs, conf, kps, sizes, where, knn)
    _sync()                                                       # the inputs are in place, whatever stream wrote them
    return mt_run(b, stream)


def mt_read(b):
    return [dict(count=int(_np(b["c"])[0, k]), matches=_np(b["m"][k]), points=_np(b["p"][k]) if b["p"] else None,
                 knn=(_np(b["k"][2 * k]), _np(b["k"][2 * k + 1])) if b["k"] else None) for k in range(len(b["pairs"]))]


def mt_check(b, want, what):
    from test_gpu_match import check_against_model
    check_against_model(mt_read(b), want, what)


def mt_problems():
    """big (more than two query blocks, more than one train chunk), small, and an image without rows"""
    from imagestitch_amd import matcher
    a, b, _ = MC.planted_pair(4, 2 * matcher.QUERY_BLOCK + 7, matcher.TRAIN_CHUNK + 9)
    c, d, _ = MC.planted_pair(5, 31, 29)
    descs = [a, b, c, d, np.zeros((0, 32), np.uint8)]
    kps, sizes = MC.keypoints_for(4, [x.shape[0] for x in descs])
    return descs, kps, sizes


MT_PAIRS = [(0, 1), (2, 3), (2, 4)]      # (2, 4): a pair with an empty image


def _match(gpu, oracle, where):
    rec = _Rec()
    descs, kps, sizes = mt_problems()
    for name, with_kp, knn in (("keypoints-points-knn", True, True), ("descriptors-knn", False, True), ("keypoints-points", True, False)):
        want = MM.match_model(descs, MT_PAIRS, 0.3, kps if with_kp else None, sizes if with_kp else None)
        b = rec.step(name, lambda: mt_call(descs, MT_PAIRS, 0.3, kps if with_kp else None, sizes if with_kp else None, where, knn))
        _sync()
        rec.note("info", list(b["info"]))
        mt_check(b, want, (where, name))
    b = rec.step("zero-pairs", lambda: mt_call(descs, [], 0.3, kps, sizes, where, False))
    rec.note("info", list(b["info"]))
    assert (_np(b["c"]) == S_I).all()
    return rec.done()


# ---- the homography ------------------------------------------------------------------------------------------------------------------------
def hg_prepare(point_sets, counts_where="dev", points_where="dev", masks_where="dev", outs_where="dev", points=None, counts=None):
    """points / counts: mats to use as they are (the matcher's outputs); otherwise made from point_sets"""
    n = len(point_sets)
    b = dict(n=n)
    b["p"] = points if points is not None else [_placer(points_where)(p) for p in point_sets]
    b["m"] = [_placer(masks_where)(np.full((int(p.shape[0]), 1), S_B, np.uint8)) for p in b["p"]]
    b["c"] = counts if counts is not None else _placer(counts_where)(np.array([[p.shape[0] for p in point_sets]], np.int32).reshape(1, n))
    put = _placer(outs_where)
    b["H"], b["st"], b["cf"] = put(np.full((3 * n, 3), S_F, np.float64)), put(np.full((n, 8), S_I, np.int32)), put(np.full((1, n), S_F, np.float64))
    return b


def hg_run(b, stream=None):
    from imagestitch_amd import homography as hg
    b["info"] = hg.find_homography(b["p"], b["c"], b["H"], b["m"], b["st"], b["cf"], device=0, stream=stream)
    return b


def hg_call(point_sets, counts_where="dev", points_where="dev", masks_where="dev", outs_where="dev", stream=None):
    b = hg_prepare(point_sets, counts_where, points_where, masks_where, outs_where)
    _sync()
    return hg_run(b, stream)


def hg_check(b, wants, what):
    from test_gpu_homography import check
    for k, want in enumerate(wants):
        m = _np(b["m"][k])
        check(dict(H=_np(b["H"])[3 * k:3 * k + 3], mask=m[:, 0], mask_rest=m[:, 1:], stats=_np(b["st"])[k], conf=float(_np(b["cf"])[0, k])), want, (what, k))


HG_SETS = ["n6_exact", "n64_half_noisy", "n5_below_thresh1"]      # n5: fewer than num_matches_thresh1 matches


def _hg_models(names):
    out = []
    for name in names:
        pts, kw = NAMED[name]
        assert kw == {}, name
        w = HM.find_homography_np(pts)
        assert w["margin"] >= 1e-9, name
        out.append(w)
    return out


def _homography(gpu, oracle):
    rec = _Rec()
    sets, wants = [NAMED[k][0] for k in HG_SETS], _hg_models(HG_SETS)
    for name, cw, pw, mw, ow in (("all-device", "dev", "dev", "dev", "dev"), ("all-host", "host", "host", "host", "host"),
                                 ("host-counts", "host", "dev", "dev", "dev"), ("host-masks", "dev", "dev", "host", "dev"),
                                 ("host-points-and-outputs", "dev", "host", "dev", "host")):
        b = rec.step(name, lambda: hg_call(sets, cw, pw, mw, ow))
        _sync()
        rec.note("info", list(b["info"]))
        hg_check(b, wants, name)
    return rec.done()


# ---- the estimator -------------------------------------------------------------------------------------------------------------------------
ES_SETS = ["complete_9", "focals_given", "two_components_5_3"]      # the cases of the stage's host / device / strided test; focals_given stages focals_in
ES_RIGS = ["demo_2_images_1_pair", "complete_5", "complete_9"]      # three rigs in one call


@functools.lru_cache(maxsize=None)
def es_problem(name):
    """(case, model) of a named case of tests/estimator_cases.py, or of ES_RIGS joined ("three-rigs")"""
    c = EC.join([ENAMED[k] for k in ES_RIGS]) if name == "three-rigs" else ENAMED[name]
    return c, EM.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"], c["focals_in"])


def es_prepare(prob, where):
    c = prob[0]
    put = _placer(where)
    n, npairs = len(c["sizes"]), len(c["pairs"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    b = dict(case=c)
    b["H"], b["st"] = put(np.asarray(c["H"], np.float64).reshape(3 * npairs, 3), 0), put(c["stats"], 1)
    b["cf"] = put(np.zeros((1, npairs)), 2)
    b["fin"] = None if c["focals_in"] is None else put(c["focals_in"], 3)
    b["outs"] = [put(np.full((n, 16), S_F, np.float64), 4), put(np.full((n, 18), S_F, np.float32), 5), put(np.full((n, 2), S_I, np.int32), 6),
                 put(np.full((nrigs, 8), S_I, np.int32), 7)]
    return b


def es_run(b, stream=None):
    from imagestitch_amd import cameras as cam
    c = b["case"]
    b["info"] = cam.estimate_cameras(c["sizes"], c["pairs"], b["H"], b["st"], b["cf"], *b["outs"], rig_first=c["rig_first"], focals_in=b["fin"], stream=stream)
    return b


def es_call(prob, where):
    b = es_prepare(prob, where)
    _sync()
    return es_run(b)


def es_check(b, prob, what):
    from test_gpu_estimator import check
    check(tuple(_np(a) for a in b["outs"]), prob[1], what)


def _estimator(gpu, oracle, where):
    rec = _Rec()
    for name in ES_SETS + ["three-rigs"]:
        prob = es_problem(name)
        b = rec.step(name, lambda: es_call(prob, where))
        _sync()
        rec.note("info", list(b["info"]))
        es_check(b, prob, (where, name))
    return rec.done()


# ---- the graph cut -------------------------------------------------------------------------------------------------------------------------
def _graphcut(gpu, oracle):
    from test_gpu_graphcut_seam import layout
    from test_graphcut_grad_model import layout as grad_layout
    rec = _Rec()
    for name, cost, wide, lay, f32 in (("u8-color", GG.COST_COLOR, False, layout(2, 1), False), ("f32-color", GG.COST_COLOR, False, layout(2, 1), True),
                                      ("f32-color-grad-64", GG.COST_COLOR_GRAD, True, grad_layout(2, 1), True)):
        corners, imgs, masks = lay
        src = [a.astype(np.float32) for a in imgs] if f32 else imgs
        m1, m2 = masks[0].copy(), masks[1].copy()
        sizes = [(a.shape[1], a.shape[0]) for a in imgs]
        roi = G.overlap_roi(corners[0], corners[1], sizes[0], sizes[1])
        assert roi is not None
        g = GG.pair_graph(src[0], src[1], m1, m2, corners[0], corners[1], roi, cost)
        w1, w2 = m1.copy(), m2.copy()
        r = rec.step(name, lambda: gpu.GraphCutSeamFinder(cost_type=cost).find_pair(src[0], src[1], corners[0], corners[1], m1, m2, certificate=True, wide=wide))
        assert r["residuals"].dtype == (np.int64 if wide else np.int32)
        G.check_certificate(g, r["flow"], r["residuals"], r["labels"])
        G.write_back(r["labels"], w1, w2, corners[0], corners[1], roi)
        assert np.array_equal(m1, w1) and np.array_equal(m2, w2)
        rec.note("grid_and_flow", [r["rows"], r["cols"], int(r["flow"])])
    return rec.done()


# ---- Voronoi -------------------------------------------------------------------------------------------------------------------------------
def _voronoi(gpu, oracle):
    from test_gpu_voronoi_seam import _sizes, layout
    rec = _Rec()
    corners, masks = layout(3, 2)
    want = [m.copy() for m in masks]
    V.find(_sizes(want), corners, want)
    gpu.VoronoiSeamFinder.release()
    for name in ("device", "host", "device-after-reserve"):
        got = [m.copy() for m in masks] if name == "host" else [_dev(m) for m in masks]
        if name == "device-after-reserve":
            gpu.VoronoiSeamFinder().reserve(200, 160)
        rec.step(name, lambda: gpu.VoronoiSeamFinder().find(_sizes(masks), corners, got))
        _sync()
        assert all(np.array_equal(_np(a), w) for a, w in zip(got, want)), name
    gpu.VoronoiSeamFinder.release()
    return rec.done()


# ---- the gain feed -------------------------------------------------------------------------------------------------------------------------
def _gain_feed(gpu, oracle):
    from test_gain_model import THREE_I, THREE_N, three_tiles_gains, three_tiles_one_pair_apart
    rec = _Rec()
    corners, imgs, masks = three_tiles_one_pair_apart()
    for name in ("host", "device"):
        im, mk = (imgs, masks) if name == "host" else ([_dev(a) for a in imgs], [_dev(m) for m in masks])
        comp = rec.step(name, lambda: gpu.GainCompensator().feed(corners, im, mk))
        assert np.array_equal(comp.N, THREE_N) and np.array_equal(comp.I, THREE_I)
        np.testing.assert_allclose(comp.gains(), three_tiles_gains(), rtol=1e-13, atol=0)
    return rec.done()


# ---- isx_seam_estimate_cost ----------------------------------------------------------------------------------------------------------------
def _seam_estimate(gpu, oracle):
    rec = _Rec()
    for name, kw in (("f32-vertical", dict(seed=1)), ("u8-horizontal", dict(seed=2, u8=True, horizontal=True))):
        c = make_case(**kw)
        args = (c["img1"], c["img2"], c["tl1"], c["tl2"], c["union_tl"], c["labels"], c["label"], c["roi"], c["p1"], c["p2"])
        ref, rh = oracle.seam_estimate(*args)
        got, gh = rec.step(name + "-color", lambda: gpu.seam_estimate(*args, cost_func=gpu.DP_COLOR))
        assert gh == rh and len(ref) > 0 and np.array_equal(got, ref), name
        ref, rh = DPG.seam_estimate(*args, DPG.COLOR_GRAD)
        got, gh = rec.step(name + "-color-grad", lambda: gpu.seam_estimate(*args, cost_func=gpu.DP_COLOR_GRAD))
        assert gh == rh and len(ref) > 0 and np.array_equal(got, ref), name
    return rec.done()


# ---- isx_blend_pair_linear -----------------------------------------------------------------------------------------------------------------
LINEAR = {"two-tiles": (40, 64, 43, 60, (10, 20), (37, 23)), "one-row": (1, 64, 1, 60, (3, 5), (30, 5))}      # h1, w1, h2, w2, tl1, tl2


def linear_case(name):
    h1, w1, h2, w2, tl1, tl2 = LINEAR[name]
    rng = np.random.default_rng(17 + h1)
    img1, img2 = rng.random((h1, w1, 3)).astype(np.float32) * 255, rng.random((h2, w2, 3)).astype(np.float32) * 255
    if h1 > 1:      # black corners: all four overlap classes occur
        img1[:6, -9:] = 3.0
        img2[-7:, :8] = 2.0
    return img1, img2, tl1, tl2


def _blend_pair_linear(gpu, oracle):
    from imagestitch_amd import _lib
    rec = _Rec()
    for name in sorted(LINEAR):
        img1, img2, tl1, tl2 = linear_case(name)
        rc, opano, oseam = oracle.blend_pair_linear(img1, img2, tl1, tl2)
        assert rc == 0, name
        for where in ("host", "device"):
            a, b = (img1, img2) if where == "host" else (_dev(img1), _dev(img2))
            pano = np.empty_like(opano) if where == "host" else _dev(np.zeros_like(opano))
            seam = np.zeros(opano.shape[0], np.int32)
            m1, m2, mp = _lib.as_mat(a), _lib.as_mat(b), _lib.as_mat(pano)
            rec.step("%s-%s" % (name, where), lambda: _lib.check(_lib.load().isx_blend_pair_linear(
                C.byref(m1), C.byref(m2), tl1[0], tl1[1], tl2[0], tl2[1], C.byref(mp), seam.ctypes.data_as(_lib._IP), 0, None)))
            assert np.array_equal(seam, oseam) and np.array_equal(_np(pano), opano, equal_nan=True), (name, where)
    return rec.done()


# ---- BlocksGainCompensator: the first apply builds the tables ------------------------------------------------------------------------------
def _blocks_gain_apply(gpu, oracle):
    rec = _Rec()
    w, h, blw, blh = 67, 45, 32, 32
    rng = np.random.default_rng(7)
    imgs = [rng.integers(60, 120, (h, w, 3), dtype=np.uint8), rng.integers(150, 256, (h, w, 3), dtype=np.uint8)]
    masks = [np.full((h, w), 255, np.uint8)] * 2
    comp = rec.step("feed", lambda: gpu.BlocksGainCompensator(blw, blh).feed([(0, 0), (w // 3, h // 4)], imgs, masks))
    maps = comp.gain_maps()
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for name, index in (("first-apply", 0), ("second-apply", 1), ("first-again", 0)):
        t = _dev(img)
        rec.step(name, lambda: comp.apply(index, (0, 0), t, None))
        assert np.array_equal(_np(t), BGM.apply_model(img, maps[index])), name
    return rec.done()


# ---- part 3: the messages ------------------------------------------------------------------------------------------------------------------
def _refused(rec, gpu, name, fn):
    with pytest.raises(gpu.IsxError) as e:
        fn()
    rec.note("errors", [name, int(e.value.code), str(e.value.msg)])


def _match_errors(gpu, oracle):
    """the refused calls of tests/test_gpu_match.py::test_errors_leave_the_outputs_untouched, in its order"""
    from imagestitch_amd import _lib, matcher
    rec = _Rec()
    a, b, _ = MC.planted_pair(1, 24, 30)
    kps, sizes = MC.keypoints_for(1, [24, 30])
    d, k = [_dev(a), _dev(b)], [_dev(kps[0]), _dev(kps[1])]
    m, p, c = _dev(np.full((54, 3), S_I, np.int32)), _dev(np.full((54, 4), S_I, np.float32)), _dev(np.full((1, 1), S_I, np.int32))
    kn = [_dev(np.full((24, 4), S_I, np.int32)), _dev(np.full((30, 4), S_I, np.int32))]
    z = lambda shape, dt: _dev(np.zeros(shape, dt))      # noqa: E731

    def call(descs=d, pairs=((0, 1),), conf=0.3, ms=None, cnt=None, kp=k, sz=sizes, ps=None, ks=None):
        return lambda: matcher.match_features(descs, list(pairs), conf, [m] if ms is None else ms, c if cnt is None else cnt, kp, sz,
                                              [p] if ps is None else ps, kn if ks is None else ks)
    cases = [("pair-1-0", call(pairs=((1, 0),))), ("pair-0-0", call(pairs=((0, 0),))), ("pair-0-2", call(pairs=((0, 2),))), ("pair--1-1", call(pairs=((-1, 1),)))]
    cases += [("conf-%r" % conf, call(conf=conf)) for conf in (-0.01, 1.0, 1.5, float("nan"), float("inf"))]
    cases += [("keypoints-without-sizes", call(sz=None)), ("descriptors-f32", call(descs=[_dev(a.astype(np.float32)), d[1]])),
              ("matches-f32", call(ms=[z((54, 3), np.float32)])), ("points-s32", call(ps=[z((54, 4), np.int32)])), ("counts-f32", call(cnt=z((1, 1), np.float32))),
              ("knn-f32", call(ks=[kn[0], z((30, 4), np.float32)])), ("keypoints-s32", call(kp=[k[0], _dev(kps[1].astype(np.int32))])),
              ("descriptors-64-columns", call(descs=[z((24, 64), np.uint8), d[1]])), ("descriptors-16-columns", call(descs=[z((24, 16), np.uint8), d[1]])),
              ("matches-53-rows", call(ms=[z((53, 3), np.int32)])), ("matches-2-columns", call(ms=[z((54, 2), np.int32)])),
              ("points-3-columns", call(ps=[z((54, 3), np.float32)])), ("knn-23-rows", call(ks=[z((23, 4), np.int32), kn[1]])),
              ("counts-hold-one-pair", call(pairs=((0, 1), (0, 1)), ms=[m, m], ps=[p, p], ks=kn + kn)), ("keypoints-29-rows", call(kp=[k[0], _dev(kps[1][:29])]))]
    # mats of the merged check's later branches, which the suite reaches through the C entry or not at all: null data, a short step, a
    # misaligned pointer, another device
    lib, IsxMat, as_mat = _lib.load(), _lib.IsxMat, _lib.as_mat

    def raw(matches=None, counts=None):
        mm = (IsxMat * 1)(as_mat(m) if matches is None else matches)
        cc = as_mat(c) if counts is None else counts
        return lambda: _lib.check(lib.isx_match_features(2, (IsxMat * 2)(as_mat(d[0]), as_mat(d[1])), None, None, 1, (C.c_int * 2)(0, 1), 0.3, mm, None,
                                                         C.byref(cc), None, None, 0, None))

    def edited(t, **kw):
        mat = as_mat(t)
        for key, v in kw.items():
            setattr(mat, key, v if key != "data" or v is None else mat.data + v)
        return mat
    cases += [("matches-null-data", raw(matches=edited(m, data=None))), ("matches-short-step", raw(matches=edited(m, step=8))),
              ("matches-misaligned", raw(matches=edited(m, data=2))), ("matches-odd-step", raw(matches=edited(m, step=14))),
              ("matches-other-device", raw(matches=edited(m, device=5))), ("counts-null-data", raw(counts=edited(c, data=None))),
              ("counts-other-device", raw(counts=edited(c, device=3)))]
    for name, fn in cases:
        _refused(rec, gpu, name, fn)
    _sync()
    assert all((_np(t) == S_I).all() for t in [m, p, c] + kn)
    return rec.done()


def _homography_errors(gpu, oracle):
    """the refused calls of tests/test_gpu_homography.py::test_errors_leave_the_outputs_untouched, in its order"""
    from imagestitch_amd import _lib
    from imagestitch_amd import homography as hg
    rec = _Rec()
    pts = NAMED["n64_half_noisy"][0]
    p, c = _dev(pts), _dev(np.array([[64]], np.int32))
    H, m = _dev(np.full((3, 3), S_F, np.float64)), _dev(np.full((64, 1), S_B, np.uint8))
    st, cf = _dev(np.full((1, 8), S_I, np.int32)), _dev(np.full((1, 1), S_F, np.float64))
    z = lambda shape, dt: _dev(np.zeros(shape, dt))      # noqa: E731

    def call(points=None, counts=c, H=H, masks=None, stats=st, conf=cf, **kw):
        return lambda: hg.find_homography([p] if points is None else points, counts, H, [m] if masks is None else masks, stats, conf, **kw)
    cases = [("confidence-%r" % v, call(confidence=v)) for v in (0.0, 1.0, -0.5, 1.5, float("nan"))]
    cases += [("max_iters-0", call(max_iters=0)), ("thresh1--1", call(num_matches_thresh1=-1)), ("thresh2--1", call(num_matches_thresh2=-1)),
              ("reproj-nan", call(reproj_thresh=float("nan"))), ("points-f64", call(points=[_dev(pts.astype(np.float64))])),
              ("counts-f32", call(counts=z((1, 1), np.float32))), ("H-f32", call(H=z((3, 3), np.float32))), ("masks-s32", call(masks=[z((64, 1), np.int32)])),
              ("stats-f32", call(stats=z((1, 8), np.float32))), ("conf-f32", call(conf=z((1, 1), np.float32))), ("points-3-columns", call(points=[_dev(pts[:, :3].copy())])),
              ("H-2-rows", call(H=z((2, 3), np.float64))), ("H-2-columns", call(H=z((3, 2), np.float64))), ("stats-7-columns", call(stats=z((1, 7), np.int32))),
              ("outputs-hold-one-pair", call(points=[p, p], masks=[m, m]))]
    lib, IsxMat, as_mat = _lib.load(), _lib.IsxMat, _lib.as_mat

    def raw(**kw):
        a = dict(points=as_mat(p), counts=as_mat(c), H=as_mat(H), masks=as_mat(m), stats=as_mat(st), conf=as_mat(cf))
        a.update(kw)
        return lambda: _lib.check(lib.isx_find_homography(1, (IsxMat * 1)(a["points"]), C.byref(a["counts"]), 3.0, 2000, 0.995, 6, 6, C.byref(a["H"]),
                                                          (IsxMat * 1)(a["masks"]), C.byref(a["stats"]), C.byref(a["conf"]), None, 0, None))

    def edited(t, **kw):
        mat = as_mat(t)
        for key, v in kw.items():
            setattr(mat, key, v if key != "data" or v is None else mat.data + v)
        return mat
    cases += [("H-misaligned", raw(H=edited(z((4, 3), np.float64), data=4))), ("H-null-data", raw(H=edited(H, data=None))), ("H-short-step", raw(H=edited(H, step=16))),
              ("H-other-device", raw(H=edited(H, device=2))), ("stats-odd-step", raw(stats=edited(st, step=34))), ("points-null-data", raw(points=edited(p, data=None))),
              ("points-misaligned", raw(points=edited(p, data=2))), ("points-short-step", raw(points=edited(p, step=12))), ("masks-other-device", raw(masks=edited(m, device=1))),
              ("masks-no-columns", raw(masks=edited(m, cols=0))), ("conf-misaligned", raw(conf=edited(z((1, 2), np.float64), data=4)))]
    for name, fn in cases:
        _refused(rec, gpu, name, fn)
    _sync()
    assert (_np(H) == S_F).all() and (_np(m) == S_B).all() and (_np(st) == S_I).all() and (_np(cf) == S_F).all()
    return rec.done()


def _estimator_errors(gpu, oracle):
    """the refused calls that _refusals() of tests/test_gpu_estimator_guard.py lists, in its order, and the capture refusal of that suite"""
    import torch
    import test_gpu_estimator_guard as EG
    from helpers.guarded import guarded
    rec = _Rec()
    c = EG._case()
    ins, outs = EG._mats(c, "device", "aligned", 20)
    big = dict(cameras=guarded((67, 16), np.float64, "device", "aligned", 31), kr32=guarded((67, 18), np.float32, "device", "aligned", 32),
               tree=guarded((67, 2), np.int32, "device", "aligned", 33), rig_stats=guarded((2, 8), np.int32, "device", "aligned", 34))
    for name, code, over in EG._refusals(c):
        # "65 images": outputs large enough, so that the rig's size alone is what is refused
        _refused(rec, gpu, name, lambda: EG._call(c, ins, big if "65 images" in name else outs, **over))
        assert rec.notes["errors"][-1][1] == code, rec.notes["errors"][-1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.zeros(4, device="cuda")
    _sync()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        _refused(rec, gpu, "a capturing stream", lambda: EG._call(c, ins, outs, stream=s))
    assert rec.notes["errors"][-1][1] == EG.ERR_STATE
    EG._untouched(ins, outs)
    EG._untouched({}, big)
    return rec.done()


CASES = {"match-dev": lambda g, o: _match(g, o, "dev"), "match-host": lambda g, o: _match(g, o, "host"), "match-mixed": lambda g, o: _match(g, o, "mixed"),
         "homography": _homography, "graphcut": _graphcut, "voronoi": _voronoi, "gain-feed": _gain_feed, "seam-estimate": _seam_estimate,
         "blend-pair-linear": _blend_pair_linear, "blocks-gain-apply": _blocks_gain_apply, "match-errors": _match_errors,
         "homography-errors": _homography_errors, "estimator-dev": lambda g, o: _estimator(g, o, "dev"),
         "estimator-host": lambda g, o: _estimator(g, o, "host"), "estimator-mixed": lambda g, o: _estimator(g, o, "mixed"),
         "estimator-errors": _estimator_errors}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_decisions_and_messages_equal_the_recorded_ones(gpu, oracle, golden, case):
    got, want = json.loads(json.dumps(CASES[case](gpu, oracle))), golden[case]
    print(case, json.dumps(got, sort_keys=True))
    assert got["notes"] == want["notes"], (case, got["notes"], want["notes"])
    assert [s[0] for s in got["steps"]] == [s[0] for s in want["steps"]], case
    for (step, launches), (_step, wlaunches) in zip(got["steps"], want["steps"]):
        assert sorted(launches) == sorted(wlaunches), (case, step, sorted(launches), sorted(wlaunches))
        for name, (n, by) in launches.items():
            wn, wby = wlaunches[name]
            if wn < 0:      # the count varies from run to run (see the docstring): the bytes of one launch do not
                by, n, wn = by / n, 0, 0
            assert n == wn, (case, step, name, n, wn)
            assert abs(by - wby) <= BYTES_RTOL * abs(wby), (case, step, name, by, wby)


# ---- part 2: the fence and the pinned buffer in use ----------------------------------------------------------------------------------------
def _mt_two():
    """(descriptors, keypoints, sizes, model) of the big and of the small problem; the small one's work fits in the big one's"""
    descs, kps, sizes = mt_problems()
    out = []
    for i, j in ((0, 1), (2, 3)):
        d, k, s = [descs[i], descs[j]], [kps[i], kps[j]], [sizes[i], sizes[j]]
        out.append((d, k, s, MM.match_model(d, [(0, 1)], 0.3, k, s)))
    return out


def _hg_two():
    return [([NAMED[name][0]], _hg_models([name])) for name in ("n300_half_noisy", "n64_half_noisy")]


def _chain_two():
    """two sets of synthetic features whose matches carry a planted homography, and the models of both stages"""
    from test_gpu_homography import _synthetic_features
    out = []
    for seed, rows in ((5, [90, 70]), (6, [60, 50])):
        descs, kps, sizes = _synthetic_features(seed, rows, 40)
        wm = MM.match_model(descs, [(0, 1)], 0.3, kps, sizes)
        wh = HM.find_homography_np(wm[0]["points"])
        assert wm[0]["count"] >= 30 and wh["margin"] >= 1e-9
        out.append((descs, kps, sizes, wm, wh))
    return out


def _chain_prepare(prob, where):
    """the homography reads the matcher's points and counts where the matcher leaves them: nothing in between"""
    descs, kps, sizes, _, _ = prob
    bm = mt_prepare(descs, [(0, 1)], 0.3, kps, sizes, where, False)
    w = "host" if where == "host" else "dev"
    return bm, hg_prepare([None], w, w, w, w, points=bm["p"], counts=bm["c"])


def _chain_check(bs, prob, what):
    mt_check(bs[0], prob[3], what)
    hg_check(bs[1], [prob[4]], what)


# ---- the adjusters and the wave correction: three entries on one per-thread BaScratch ------------------------------------------------------
_BA_OUTS = (((16,), np.float64, S_F), ((18,), np.float32, S_F), ((8,), np.int32, S_I), ((2,), np.float64, S_F))      # cameras, kr32, rig_stats, rig_err


@functools.lru_cache(maxsize=None)
def ba_problem(kind, name):
    """(case, model) of a named case of tests/bundle_cases.py (kind "ray") or tests/bundle_reproj_cases.py ("reproj")"""
    import fuzz_bundle
    import fuzz_bundle_reproj
    if kind == "ray":
        c = BC.named()[name]
        return c, fuzz_bundle.run_model(c)
    c = BRC.named()[name]
    return c, fuzz_bundle_reproj.run_model(c)


def _ba_outs(put, n, nrigs, k0=0):
    rows = (n, n, nrigs, nrigs)
    return [put(np.full((r,) + shape, fill, dt), k0 + k) for k, (r, (shape, dt, fill)) in enumerate(zip(rows, _BA_OUTS))]


def ba_prepare(prob, where, cameras_in=None):
    """cameras_in: a mat to read as it is (the cameras_out of the call before); otherwise the case's"""
    c = prob[0]
    put = _placer(where)
    n = len(c["sizes"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    b = dict(case=c)
    b["kp"] = [put(k, i) for i, k in enumerate(c["keypoints"])]
    b["m"] = [put(m, i + 1) for i, m in enumerate(c["matches"])]
    b["mk"] = [put(m, i) for i, m in enumerate(c["masks"])]
    b["c"], b["st"], b["cf"], b["est"] = put(c["counts"], 1), put(c["stats"], 2), put(c["conf"], 3), put(c["est_rig_stats"], 4)
    b["cin"] = put(c["cameras_in"], 5) if cameras_in is None else cameras_in
    b["outs"] = _ba_outs(put, n, nrigs, 6)
    return b


def ba_run(b, stream, kind):
    from imagestitch_amd import adjuster as adj
    c = b["case"]
    fn, kw = (adj.bundle_adjust_ray, {}) if kind == "ray" else (adj.bundle_adjust_reproj, dict(refine_flags=c["refine_flags"]))
    b["info"] = fn(c["sizes"], b["kp"], c["pairs"], b["m"], b["mk"], b["c"], b["st"], b["cf"], b["est"], b["cin"], *b["outs"], rig_first=c["rig_first"],
                   conf_thresh=c["conf_thresh"], max_iter=c["max_iter"], stream=stream, **kw)
    return b


def _same_outs(got, want, what):
    from fuzz_estimator import same
    for k, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert g.shape == w.shape and g.dtype == w.dtype and same(g, w), (what, k, g, w)


def ba_check(b, prob, what):
    nrigs = 1 if prob[0]["rig_first"] is None else len(prob[0]["rig_first"]) - 1
    assert b["info"] == (nrigs, 1), (what, b["info"])
    _same_outs(b["outs"], prob[1], what)


@functools.lru_cache(maxsize=None)
def wv_problem(name):
    """(cameras, model) of a rig of bundle_reproj_cases.wave_rigs(), horizontal"""
    cams = BRC.wave_rigs()[name]
    return cams, BRP.wave_correct(cams, None, BRP.WAVE_HORIZ)


def _wv_outs(put, n, k0=0):
    return [put(np.full((n, 16), S_F, np.float64), k0), put(np.full((n, 18), S_F, np.float32), k0 + 1), put(np.full((1, 2), S_I, np.int32), k0 + 2)]


def wv_prepare(prob, where, cameras_in=None):
    put = _placer(where)
    return dict(cin=put(prob[0], 0) if cameras_in is None else cameras_in, outs=_wv_outs(put, prob[0].shape[0], 1))


def wv_run(b, stream):
    from imagestitch_amd import adjuster as adj
    b["info"] = adj.wave_correct(b["cin"], *b["outs"], kind=adj.WAVE_CORRECT_HORIZ, stream=stream)
    return b


def wv_check(b, prob, what):
    assert b["info"] == (1, 1), (what, b["info"])
    _same_outs(b["outs"], prob[1], what)


@functools.lru_cache(maxsize=None)
def adjust_chain_problem(name):
    """BundleAdjusterRay, BundleAdjusterReproj on its cameras, waveCorrect on those, as cv::Stitcher runs them one after the other: (the Ray
    case, the three models, each fed the model's cameras of the one before)"""
    c = BC.named()[name]
    ray = BM.adjust(c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"], c["conf"], c["est_rig_stats"], c["cameras_in"],
                    c["rig_first"], c["conf_thresh"], c["max_iter"])
    reproj = BRP.adjust(c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"], c["conf"], c["est_rig_stats"], ray[0],
                        c["rig_first"], c["conf_thresh"], c["max_iter"])
    return dict(c, refine_flags=BRP.REFINE_ALL), ray, reproj, BRP.wave_correct(reproj[0], c["rig_first"], BRP.WAVE_HORIZ)


def _adjust_chain_prepare(prob, where):
    """each call reads the cameras_out of the one before where that call leaves it: nothing in between"""
    ray = ba_prepare(prob, where)
    reproj = dict(ray, cin=ray["outs"][0], outs=_ba_outs(_placer(where), len(prob[0]["sizes"]), 1))
    return ray, reproj, wv_prepare((prob[0]["cameras_in"],), where, cameras_in=reproj["outs"][0])


def _adjust_chain_run(bs, stream):
    return ba_run(bs[0], stream, "ray"), ba_run(bs[1], stream, "reproj"), wv_run(bs[2], stream)


def _adjust_chain_check(bs, prob, what):
    for b, want, stage in zip(bs, prob[1:], ("ray", "reproj", "wave")):
        assert b["info"] == (1, 1), (what, stage, b["info"])
        _same_outs(b["outs"], want, (what, stage))


def _stage(name):
    """(the big and the small problem, prepare(problem, where) -> buffers, run(buffers, stream), check(buffers, problem, what)) of a stage"""
    if name == "bundle_ray":      # 24 images and 276 edges, then 3 and 3
        return ([ba_problem("ray", "tiles_past_a_block"), ba_problem("ray", "max_iter_3")], ba_prepare, lambda b, s: ba_run(b, s, "ray"), ba_check)
    if name == "bundle_reproj":   # 37 images (259 unknowns), then 2
        return ([ba_problem("reproj", "chain_37"), ba_problem("reproj", "two_images_8_inliers")], ba_prepare, lambda b, s: ba_run(b, s, "reproj"), ba_check)
    if name == "wave":
        return [wv_problem("pan_64"), wv_problem("pan_3")], wv_prepare, wv_run, wv_check
    if name == "adjust_chain":    # three calls a run on one scratch: 5 images with edges of up to 129 inliers, then 2 images with 8
        return [adjust_chain_problem("tiles_5"), adjust_chain_problem("two_images_8_inliers")], _adjust_chain_prepare, _adjust_chain_run, _adjust_chain_check
    if name == "match":
        return (_mt_two(), lambda p, where: mt_prepare(p[0], [(0, 1)], 0.3, p[1], p[2], where, True), mt_run,
                lambda b, p, what: mt_check(b, p[3], what))
    if name == "homography":
        return _hg_two(), lambda p, where: hg_prepare(p[0], where, where, where, where), hg_run, lambda b, p, what: hg_check(b, p[1], what)
    if name == "estimator":      # 17 images and 136 pairs, then 5 and 10
        return [es_problem("complete_17"), es_problem("complete_5")], es_prepare, es_run, es_check
    return _chain_two(), _chain_prepare, lambda bs, s: (mt_run(bs[0], s), hg_run(bs[1], s)), _chain_check


def _release(gpu):
    from imagestitch_amd import adjuster as adj
    from imagestitch_amd import cameras as cam
    from imagestitch_amd import homography as hg
    gpu.FeaturesMatcher.release()
    hg.release()
    cam.release()
    adj.release()


STAGES = ["match", "homography", "chain", "estimator", "bundle_ray", "bundle_reproj", "wave", "adjust_chain"]


@pytest.mark.parametrize("stage", STAGES)
def test_two_problems_at_once_on_two_streams(gpu, stage):
    """A on s1, then at once B - another problem, whose work fits in A's allocation - on s2; no host synchronisation in between.  Both
    results equal the model.  This pins results only: without the fence B races with A, and a race need not fail."""
    import torch
    (A, B), prepare, run, check = _stage(stage)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _release(gpu)
    for round_ in range(3):                                       # the first round allocates; the later ones find everything in place
        a, b = prepare(A, "dev"), prepare(B, "dev")
        _sync()                                                   # the inputs are in place
        run(a, s1)
        run(b, s2)
        _sync()
        check(a, A, (stage, "A", round_)); check(b, B, (stage, "B", round_))
    _release(gpu)


@pytest.mark.parametrize("stage", STAGES)
def test_host_mats_right_after_device_mats(gpu, stage):
    """A with device mats, then at once B with host mats: B refills the pinned upload buffer, so it must wait for A's upload first.  Both
    results equal the model (results only: see the module's docstring)."""
    import torch
    (A, B), prepare, run, check = _stage(stage)
    s = torch.cuda.Stream()
    _release(gpu)
    for first, second in ((A, B), (B, A)):
        a, b = prepare(first, "dev"), prepare(second, "host")
        _sync()
        run(a, s)
        run(b, s)
        _sync()
        check(a, first, (stage, "device mats")); check(b, second, (stage, "host mats"))
    _release(gpu)


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("where", ["dev", "host"])
def test_big_small_release_small_big_release_twice(gpu, stage, where):
    (big, small), prepare, run, check = _stage(stage)
    _release(gpu)
    for what, prob in (("big", big), ("small", small), (None, None), ("small after release", small), ("big after release", big)):
        if prob is None:
            _release(gpu)
            continue
        b = prepare(prob, where)
        _sync()
        run(b, None)
        _sync()
        check(b, prob, (stage, where, what))
    _release(gpu)
    _release(gpu)


def test_ray_reproj_and_wave_on_three_streams(gpu):
    """The three entries that carve one per-thread BaScratch, back to back on three streams with no host synchronisation: Ray(A) on s1,
    Reproj(B) on s2, the wave correction (C) on s3.  k_ba_rigs keeps JtJ, L, the tiles and the per-edge matrices in `work` for its whole
    Levenberg-Marquardt loop, so each call must wait for the one before on another stream.  Three rounds: the first allocates (Ray, then the
    larger Reproj, which grows `work` with a hipFree that waits for the device); the later ones find everything in place, and only the
    fence orders them.  All three results equal their models (results only: see the module's docstring)."""
    import torch
    A, B, Cw = ba_problem("ray", "tiles_past_a_block"), ba_problem("reproj", "chain_37"), wv_problem("pan_64")
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    _release(gpu)
    for round_ in range(3):
        a, b, c = ba_prepare(A, "dev"), ba_prepare(B, "dev"), wv_prepare(Cw, "dev")
        _sync()                                                   # the inputs are in place
        ba_run(a, s1, "ray")
        ba_run(b, s2, "reproj")
        wv_run(c, s3)
        _sync()
        ba_check(a, A, ("ray", round_)); ba_check(b, B, ("reproj", round_)); wv_check(c, Cw, ("wave", round_))
    _release(gpu)


def test_two_threads_have_their_own_scratch(gpu):
    """The scratch is per calling thread (per_thread<BaScratch>()): two Python threads, each on its own stream, one running Ray on 276
    edges five times, the other Reproj and the wave correction twenty times, share nothing and need no fence between them.  Every result
    equals its model; each thread returns its own scratch at its end, since nothing frees it when the thread exits."""
    import threading
    import torch
    from imagestitch_amd import adjuster as adj
    A, B, Cw = ba_problem("ray", "tiles_past_a_block"), ba_problem("reproj", "max_iter_3"), wv_problem("pan_5_planted")
    _release(gpu)
    _sync()
    errors = []

    def worker(jobs, rounds):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            for round_ in range(rounds):
                with torch.cuda.stream(s):                        # the inputs are placed on the thread's own stream, which orders them before the call
                    bufs = [prepare(prob, "dev") for prob, prepare, _, _ in jobs]
                for (prob, _, run, _), b in zip(jobs, bufs):
                    run(b, s)
                s.synchronize()
                for (prob, _, _, check), b in zip(jobs, bufs):
                    check(b, prob, (threading.current_thread().name, round_))
            adj.release()
        except BaseException as e:      # noqa: BLE001 - handed to the main thread, which fails the test
            errors.append(e)

    threads = [threading.Thread(target=worker, name="ray", args=([(A, ba_prepare, lambda b, s: ba_run(b, s, "ray"), ba_check)], 5)),
               threading.Thread(target=worker, name="reproj-wave",
                                args=([(B, ba_prepare, lambda b, s: ba_run(b, s, "reproj"), ba_check), (Cw, wv_prepare, wv_run, wv_check)], 20))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    _sync()
    if errors:
        raise errors[0]
    _release(gpu)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_stage_scratch.py --record")
    import imagestitch_amd
    from oracle import capi
    imagestitch_amd.load()
    capi.lib()
    out = {}
    for case_id in sorted(CASES):
        out[case_id] = CASES[case_id](imagestitch_amd, capi)
        again = CASES[case_id](imagestitch_amd, capi)
        assert again["notes"] == out[case_id]["notes"], (case_id, "the notes differ between two passes")
        for (step, launches), (_s, launches2) in zip(out[case_id]["steps"], again["steps"]):
            assert sorted(launches) == sorted(launches2), (case_id, step)
            for name in launches:
                if launches[name][0] != launches2[name][0] or name in SWEEPS:
                    print("  %s / %s / %s: %d and %d launches, recorded as bytes per launch" % (case_id, step, name, launches[name][0], launches2[name][0]))
                    launches[name] = [-1, launches[name][1] / launches[name][0]]
        print(case_id, flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases in %s" % (len(out), GOLDEN))
