"""isx_find_homography (imagestitch_amd/homography.py) on the GPU against the NumPy model of tests/helpers/homography_np.py: masks and stats
with np.array_equal, H and conf through their uint64 views.  The named cases of tests/homography_cases.py (n = 0, 3, 4, 5, 6, 63, 64, 65,
300; exact, noisy, collinear, repeated, outliers to the end of the loop, loops that end or win either side of the kernel's chunk of 64),
several pairs in one call, host and device mats, strided points, the launch count, determinism, every error status, a capturing stream, and
BestOf2NearestMatcher end to end.  No case is fragile (margin >= 1e-9 in the model): tests/test_homography_model.py checks that.

A case where pass 2 fails: the named cases and the generator hold none.  Pass 2 draws from the inliers of pass 1, which contain the subset
that won pass 1 - a subset checkSubset accepted and whose own model fits it - so with at least five inliers it finds a model again."""
import functools
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import homography_cases as cases  # noqa: E402
from helpers import homography_np as hm  # noqa: E402
from imagestitch_amd import homography as hg  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_SIZE = 1, 2, 3, 7
SENT_I, SENT_F, SENT_B = -7777, -7777.25, 0xA5
NAMED = cases.named()


@functools.lru_cache(maxsize=None)
def model(name):
    pts, kw = NAMED[name]
    return hm.find_homography_np(pts, **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _sync():
    import torch
    torch.cuda.synchronize()


def run_raw(point_sets, counts=None, device=True, stream=None, extra_rows=0, wide=False, **kw):
    """isx_find_homography on mats pre-filled with sentinels.  point_sets: n_p x 4 arrays; counts default to their rows; extra_rows: rows of
    capacity past the count in points and masks; wide: points of 6 columns (a step of 24 bytes) and masks of 3.  Returns (per pair a dict of
    H, mask (the whole mat's first column), mask_rest (its other columns), stats, conf; info)."""
    put = _dev if device else (lambda a: np.array(a))
    n = len(point_sets)
    ps, ms = [], []
    for p in point_sets:
        full = np.full((p.shape[0] + extra_rows, 6 if wide else 4), SENT_F, np.float32)
        full[:p.shape[0], :4] = p
        ps.append(put(full))
        ms.append(put(np.full((p.shape[0] + extra_rows, 3 if wide else 1), SENT_B, np.uint8)))
    cnt = put(np.array([[p.shape[0] for p in point_sets] if counts is None else list(counts)], np.int32).reshape(1, n))
    H, stats, conf = put(np.full((3 * n, 3), SENT_F, np.float64)), put(np.full((n, 8), SENT_I, np.int32)), put(np.full((1, n), SENT_F, np.float64))
    info = hg.find_homography(ps, cnt, H, ms, stats, conf, device=0, stream=stream, **kw)
    _sync()
    out = []
    for k in range(n):
        m = _np(ms[k])
        out.append(dict(H=_np(H)[3 * k:3 * k + 3], mask=m[:, 0], mask_rest=m[:, 1:], stats=_np(stats)[k], conf=float(_np(conf)[0, k]),
                        points=_np(ps[k])))
    return out, info


def check(got, want, what=""):
    assert np.array_equal(got["stats"], want["stats"]), (what, got["stats"], want["stats"])
    assert np.array_equal(np.ascontiguousarray(got["H"]).view(np.uint64), np.ascontiguousarray(want["H"]).view(np.uint64)), (what, got["H"], want["H"])
    assert np.float64(got["conf"]).view(np.uint64) == np.float64(want["conf"]).view(np.uint64), (what, got["conf"], want["conf"])
    n = 0 if want["mask"] is None else len(want["mask"])
    assert np.array_equal(got["mask"][:n], want["mask"] if n else got["mask"][:0]), (what, "mask")
    assert (got["mask"][n:] == SENT_B).all() and (got["mask_rest"] == SENT_B).all(), (what, "mask bytes past the count were written")


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases_on_device_and_host_mats(gpu, name):
    pts, kw = NAMED[name]
    want = model(name)
    assert want["margin"] >= 1e-9
    for device in (True, False):
        got, info = run_raw([pts], device=device, **kw)
        check(got[0], want, (name, device))
        assert info == (1, 1)


def test_the_cases_are_what_their_names_say(gpu):
    st = {k: model(k)["stats"] for k in NAMED}
    assert st["n6_exact"][hg.ITERS1] == 1 and st["n300_exact"][hg.ITERS1] == 1                   # ep = 0 ends the loop after iteration 1
    assert st["collinear_40"][hg.ATTEMPTS] == 10000 and st["collinear_40"][hg.STATUS] == 0     # getSubset fails at iteration 0
    assert st["outliers_to_the_end"][hg.ITERS1] == 70 and st["outliers_one_chunk"][hg.ITERS1] == 64
    assert [st["stop_at_%d" % k][hg.ITERS1] for k in (63, 64, 65)] == [63, 64, 65]
    assert [st["win_at_%d" % k][hg.WIN1] for k in (63, 64)] == [63, 64]
    assert st["n4_thresh1_4"][hg.STATUS] == hg.ST_H | hg.ST_PASS2 and st["n5_below_thresh1"].tolist() == [0] * 8
    assert not any(s[hg.STATUS] & hg.ST_PASS2_FAILED for s in st.values())                     # (the docstring says why)


def test_strided_points_spare_capacity_and_wide_masks(gpu):
    for name in ("n65_half_noisy", "n5_below_thresh1", "n4_thresh1_4"):
        pts, kw = NAMED[name]
        for device in (True, False):
            got, _ = run_raw([pts], device=device, extra_rows=7, wide=True, **kw)
            check(got[0], model(name), (name, device))
            assert np.array_equal(got[0]["points"][:len(pts), :4], pts) and (got[0]["points"][len(pts):] == np.float32(SENT_F)).all()


def test_a_count_past_the_capacity_is_clamped_and_flagged(gpu):
    pts = NAMED["n65_half_noisy"][0]
    want = hm.find_homography_np(pts, count=80)
    assert want["stats"][0] & hg.ST_CLAMPED and np.array_equal(want["stats"][1:], model("n65_half_noisy")["stats"][1:])
    for device in (True, False):
        got, _ = run_raw([pts], counts=[80], device=device)
        check(got[0], want, device)
    got, _ = run_raw([pts], counts=[-3])
    assert got[0]["stats"].tolist() == [0] * 8 and (got[0]["mask"] == SENT_B).all()
    want = hm.find_homography_np(pts, count=40)                       # fewer than the rows: the rest is capacity
    got, _ = run_raw([pts], counts=[40])
    check(got[0], want)


SEVEN = ["n65_half_noisy", "n0", "n6_exact", "collinear_40", "n5_below_thresh1", "win_at_64", "n300_half_noisy"]


def test_several_pairs_in_one_call_and_the_launch_count(gpu):
    sets = [NAMED[k][0] for k in SEVEN]
    for device in (True, False):
        got, info7 = run_raw(sets, device=device)
        for k, name in enumerate(SEVEN):
            check(got[k], model(name), (name, device))
        one, info1 = run_raw(sets[:1], device=device)
        assert info7 == (7, 1) and info1 == (1, 1)                    # one launch for one pair and for seven
    again, _ = run_raw(sets)
    for a, b in zip(got, again):                                      # host mats, then device mats: identical bytes
        assert all(np.array_equal(a[key], b[key]) for key in ("H", "mask", "stats")) and a["conf"] == b["conf"]


def test_two_calls_give_identical_bytes_and_release_is_idempotent(gpu):
    import torch
    pts = NAMED["n300_half_noisy"][0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a, _ = run_raw([pts], stream=s)
    b, _ = run_raw([pts])                                             # another stream: waits for the thread's previous call
    hg.release()
    c, _ = run_raw([pts, NAMED["n6_exact"][0]])
    hg.release()
    hg.release()
    for r in (a[0], b[0], c[0]):
        check(r, model("n300_half_noisy"))
    assert a[0]["H"].tobytes() == b[0]["H"].tobytes() == c[0]["H"].tobytes()


def test_num_inliers_one_below_and_at_thresh2(gpu):
    pts = NAMED["n64_half_noisy"][0]
    k = int(model("n64_half_noisy")["stats"][hg.NUM_INLIERS])
    for thresh2, ran in ((k, True), (k + 1, False)):
        want = hm.find_homography_np(pts, num_matches_thresh2=thresh2)
        assert bool(want["stats"][0] & hg.ST_PASS2) == ran and want["stats"][hg.NUM_INLIERS] == k
        got, _ = run_raw([pts], num_matches_thresh2=thresh2)
        check(got[0], want, thresh2)


def _expect(code, fn):
    with pytest.raises(hg._lib.IsxError) as e:
        fn()
    assert e.value.code == code, (e.value.code, e.value.msg)


def test_errors_leave_the_outputs_untouched(gpu):
    import ctypes as C
    pts = NAMED["n64_half_noisy"][0]
    p, c = _dev(pts), _dev(np.array([[64]], np.int32))
    H, m = _dev(np.full((3, 3), SENT_F, np.float64)), _dev(np.full((64, 1), SENT_B, np.uint8))
    st, cf = _dev(np.full((1, 8), SENT_I, np.int32)), _dev(np.full((1, 1), SENT_F, np.float64))

    def call(points=None, counts=c, H=H, masks=None, stats=st, conf=cf, **kw):
        return lambda: hg.find_homography([p] if points is None else points, counts, H, [m] if masks is None else masks, stats, conf, **kw)
    for confidence in (0.0, 1.0, -0.5, 1.5, float("nan")):
        _expect(ERR_INVALID, call(confidence=confidence))
    _expect(ERR_INVALID, call(max_iters=0))
    _expect(ERR_INVALID, call(num_matches_thresh1=-1))
    _expect(ERR_INVALID, call(num_matches_thresh2=-1))
    _expect(ERR_INVALID, call(reproj_thresh=float("nan")))
    _expect(ERR_TYPE, call(points=[_dev(pts.astype(np.float64))]))
    _expect(ERR_TYPE, call(counts=_dev(np.zeros((1, 1), np.float32))))
    _expect(ERR_TYPE, call(H=_dev(np.zeros((3, 3), np.float32))))
    _expect(ERR_TYPE, call(masks=[_dev(np.zeros((64, 1), np.int32))]))
    _expect(ERR_TYPE, call(stats=_dev(np.zeros((1, 8), np.float32))))
    _expect(ERR_TYPE, call(conf=_dev(np.zeros((1, 1), np.float32))))
    _expect(ERR_SIZE, call(points=[_dev(pts[:, :3].copy())]))
    _expect(ERR_SIZE, call(H=_dev(np.zeros((2, 3), np.float64))))
    _expect(ERR_SIZE, call(H=_dev(np.zeros((3, 2), np.float64))))
    _expect(ERR_SIZE, call(stats=_dev(np.zeros((1, 7), np.int32))))
    _expect(ERR_SIZE, call(points=[p, p], masks=[m, m]))                        # counts, H, stats and conf hold one pair
    _expect(ERR_INVALID, call(masks=[m, m]))                                   # one points mat, two masks
    lib, IsxMat, as_mat = hg._lib.load(), hg._lib.IsxMat, hg._lib.as_mat
    mis = as_mat(_dev(np.zeros((4, 3), np.float64)))
    mis.data += 4                                                              # a misaligned H
    mats = [(IsxMat * 1)(as_mat(p)), C.byref(as_mat(c)), C.byref(as_mat(H)), (IsxMat * 1)(as_mat(m)), C.byref(as_mat(st)), C.byref(as_mat(cf))]

    def raw(args):
        return lib.isx_find_homography(1, args[0], args[1], 3.0, 2000, 0.995, 6, 6, args[2], args[3], args[4], args[5], None, 0, None)
    assert raw(mats[:2] + [C.byref(mis)] + mats[3:]) == ERR_INVALID
    for null in range(6):                                                      # null points, counts, H, inlier_masks, stats, conf
        args = list(mats)
        args[null] = None
        assert raw(args) == ERR_INVALID, null
    assert lib.isx_find_homography(-1, None, None, 3.0, 2000, 0.995, 6, 6, None, None, None, None, None, 0, None) == ERR_INVALID
    for name in ("isx_resize", "isx_convert_to"):                              # CV_64FC1 is this entry's alone
        src, dst = as_mat(H), as_mat(_dev(np.zeros((3, 3), np.float64)))
        rc = lib.isx_resize(C.byref(src), C.byref(dst), 1, 0, None) if name == "isx_resize" else lib.isx_convert_to(C.byref(src), C.byref(dst), 0, None)
        assert rc != 0, name
    _sync()
    assert (_np(H) == SENT_F).all() and (_np(m) == SENT_B).all() and (_np(st) == SENT_I).all() and (_np(cf) == SENT_F).all()
    assert np.array_equal(_np(p), pts) and int(_np(c)[0, 0]) == 64
    got, _ = run_raw([pts])                                                    # still usable
    check(got[0], model("n64_half_noisy"))


def test_a_capturing_stream_is_refused_with_nothing_enqueued(gpu):
    import torch
    pts = NAMED["n6_exact"][0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p, c = _dev(pts), _dev(np.array([[6]], np.int32))
        H, m = _dev(np.full((3, 3), SENT_F, np.float64)), _dev(np.full((6, 1), SENT_B, np.uint8))
        st, cf = _dev(np.full((1, 8), SENT_I, np.int32)), _dev(np.full((1, 1), SENT_F, np.float64))
        x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            hg.find_homography([p], c, H, [m], st, cf, stream=s)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0                                      # captured, not run; the capture is intact
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0 and (_np(H) == SENT_F).all() and (_np(st) == SENT_I).all() and (_np(m) == SENT_B).all()
    hg.find_homography([p], c, H, [m], st, cf, stream=s)           # the same stream works after the capture
    s.synchronize()
    want = model("n6_exact")
    assert np.array_equal(_np(st)[0], want["stats"]) and np.array_equal(_np(H), want["H"]) and np.array_equal(_np(m)[:, 0], want["mask"])


def _synthetic_features(seed, rows, shared):
    """Three images: the first `shared` keypoints of image 0 reappear in 1 and 2 under H_TRUE with their descriptors (a few bits flipped);
    the other rows are random.  Returns (descriptors, keypoints, sizes)."""
    r = np.random.default_rng(seed)
    sizes = [(800, 600)] * len(rows)
    base_kp = r.uniform(-250, 250, (shared, 2)).astype(np.float32)
    base_d = r.integers(0, 256, (shared, 32), dtype=np.uint8)
    descs, kps = [], []
    for i, n in enumerate(rows):
        d = r.integers(0, 256, (n, 32), dtype=np.uint8)
        kp = r.uniform(-380, 380, (n, 2)).astype(np.float32) * np.float32(0.7)
        k = min(shared, n)
        d[:k] = base_d[:k]
        d[np.arange(k), r.integers(0, 32, k)] ^= np.uint8(1 << i)
        kp[:k] = base_kp[:k] if i == 0 else (cases.project(base_kp[:k]) if i == 1 else cases.project(cases.project(base_kp[:k]))).astype(np.float32)
        perm = r.permutation(n)
        descs.append(np.ascontiguousarray(d[perm]))
        kps.append(np.ascontiguousarray(kp[perm] + np.array([400, 300], np.float32)))
    return descs, kps, sizes


def test_best_of_2_nearest_matcher_end_to_end(gpu):
    from helpers import match_np as M
    rows = [90, 70, 110, 0]
    descs, kps, sizes = _synthetic_features(5, rows, 40)
    pairs = M.near_pairs(rows)
    want_m = M.match_model(descs, pairs, 0.3, kps, sizes)
    bm = gpu.BestOf2NearestMatcher(0.3, 6, 6)
    for place in (_dev, np.array):
        recs = bm.match([place(d) for d in descs], [place(k) for k in kps], sizes)
        assert [(r.src_img_idx, r.dst_img_idx) for r in recs] == pairs and bm.last_info[0] == len(pairs) and bm.last_homography_info == (len(pairs), 1)
        for r, w in zip(recs, want_m):
            assert np.array_equal(_np(r.matches), w["matches"]) and w["count"] >= 30
            want = hm.find_homography_np(w["points"])
            assert want["margin"] >= 1e-9
            check(dict(H=np.zeros((3, 3)) if r.H is None else r.H, mask=_np(r.inliers_mask), mask_rest=np.zeros(0, np.uint8), stats=r.stats,
                       conf=r.confidence), want)
            planted = cases.H_TRUE if r.dst_img_idx - r.src_img_idx == 1 else cases.H_TRUE @ cases.H_TRUE
            assert r.num_inliers == want["stats"][1] >= 30 and np.allclose(r.H, planted / planted[2, 2], rtol=1e-4, atol=1e-6)
            d = r.dual()
            assert (d.src_img_idx, d.dst_img_idx) == (r.dst_img_idx, r.src_img_idx) and np.array_equal(d.matches[:, 0], _np(r.matches)[:, 1])
            assert np.allclose(d.H @ r.H, np.eye(3), atol=1e-9) and d.num_inliers == r.num_inliers
    fm = gpu.FeaturesMatcher(0.3)                                     # the base class is as before
    rec = fm.match(descs, kps, sizes)[0]
    assert rec.H is None and rec.inliers_mask is None and rec.num_inliers == 0 and rec.confidence == 0.0
    with pytest.raises(gpu.IsxError):
        bm.match(descs)                                               # no keypoints: no homography
    bm.release()
