"""The SIFT finder on the GPU (isx_sift_find, imagestitch_amd/features.py) against the NumPy model of tests/helpers/sift_np.py:
np.array_equal on the count, the status, the keypoints, meta and descriptors, for every case of tests/sift_cases.py; nfeatures and cap below,
at and above the count; the candidate limit; host, device, strided and unaligned mats; a side stream; several sizes on one scratch; a captured
find; every refusal; the device compilation of sift_math.hpp."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sift_cases as cases  # noqa: E402
from helpers import sift_np as M  # noqa: E402
from imagestitch_amd import _lib, features  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 123
ROOM = 16               # rows past the model's count


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def params_of(nfeatures=0, contrast_threshold=0.04, edge_threshold=10.0):
    q = features.sift_default_params()
    q.nfeatures, q.contrast_threshold, q.edge_threshold = nfeatures, contrast_threshold, edge_threshold
    return q


def outputs(cap, put):
    return (put(np.full((cap, 2), SENTINEL, np.float32)), put(np.full((cap, 5), SENTINEL, np.float32)), put(np.full((cap, 128), SENTINEL, np.float32)),
            put(np.full((1, 2), SENTINEL, np.int32)))


def run_raw(image, kw, cap, device=True, stream=None):
    """isx_sift_find on dense mats pre-filled with a sentinel: (keypoints, meta, descriptors, count_status) as NumPy arrays, whole mats"""
    import torch
    put = _dev if device else (lambda a: np.array(a))
    kp, meta, desc, cs = outputs(cap, put)
    features.sift_find(put(image), params_of(**kw), kp, meta, desc, cs, 0, stream)
    torch.cuda.synchronize()
    return _np(kp), _np(meta), _np(desc), _np(cs)


def check(got, want, what=""):
    kp, meta, desc, cs = got
    n = int(cs[0, 0])
    print(what, "count", n, "model", want["count"], "status", int(cs[0, 1]), "model", want["status"])
    assert n == want["count"] and int(cs[0, 1]) == want["status"], (what, n, want["count"], int(cs[0, 1]), want["status"])
    assert np.array_equal(kp[:n], want["keypoints"]), what
    assert np.array_equal(meta[:n], want["meta"]), what
    assert np.array_equal(desc[:n], want["descriptors"]), what
    assert (kp[n:] == SENTINEL).all() and (meta[n:] == SENTINEL).all() and (desc[n:] == SENTINEL).all(), what + ": rows from count on were written"


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case_equals_the_model(gpu, name):
    want = cases.want(name)
    check(run_raw(cases.image(name), cases.CASES[name][1], want["count"] + ROOM), want, name)


def test_cases_reach_what_they_are_for():
    """no octave below side 6, one from there; the strips have one narrow octave; 33 x 47 halves oddly twice; the edge blobs sit on the first
    and the last searched row; the thresholds open and close the finder"""
    octs = {n: cases.traced(n)[1]["octaves"] for n in ("side-1", "side-5", "side-6", "side-7", "strip-6x200", "strip-200x6", "odd-33x47")}
    assert octs["side-1"] == [] and octs["side-5"] == [] and octs["side-6"] == [(12, 12)] and octs["side-7"] == [(14, 14)]
    assert octs["strip-6x200"] == [(12, 400)] and octs["strip-200x6"] == [(400, 12)] and octs["odd-33x47"] == [(66, 94), (33, 47), (16, 23)]
    assert cases.want("strip-6x200")["count"] > 0 and cases.want("strip-200x6")["count"] > 0
    assert cases.traced("edge-blob-top")[1]["candidates"]["r"].tolist() == [5] and cases.traced("edge-blob-bottom")[1]["candidates"]["r"].tolist() == [96 - 6]
    assert cases.want("contrast-0")["count"] > 0 and cases.want("contrast-huge")["count"] == 0 and cases.want("nfeatures-1")["count"] == 1
    assert {int(o) for o in cases.want("rig-gray")["meta"][:, 3]} >= {-1, 0, 1, 2} and {int(v) for v in cases.want("rig-gray")["meta"][:, 4]} == {1, 2, 3}


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_nfeatures_below_at_and_above_the_count(gpu, delta):
    name = "odd-33x47"
    full = cases.want(name)
    nf = full["count"] + delta
    want = cases.want(name, None, nf)
    assert want["count"] == min(nf, full["count"]) and want["status"] == 0 and np.array_equal(want["descriptors"], full["descriptors"][:nf])
    check(run_raw(cases.image(name), dict(cases.CASES[name][1], nfeatures=nf), full["count"] + ROOM), want, "nfeatures %d" % nf)


@pytest.mark.parametrize("delta", [None, -1, 0, 1])
def test_cap_below_at_and_above_the_count(gpu, delta):
    name = "rig-gray"
    n = cases.want(name)["count"]
    cap = 1 if delta is None else n + delta
    want = cases.want(name, cap)
    assert want["count"] == min(cap, n) and want["status"] == (M.STATUS_TRUNCATED if cap < n else 0)
    assert np.array_equal(want["descriptors"], cases.want(name)["descriptors"][:cap])       # a prefix of the canonical order
    check(run_raw(cases.image(name), {}, cap), want, "cap %d" % cap)


def test_nfeatures_at_the_cap_is_not_truncated(gpu):
    """count = min(total, nfeatures, cap): ISX_SIFT_TRUNCATED only where the cap cut what nfeatures left"""
    name = "rig-gray"
    want = cases.want(name, 7, 7)
    assert want["count"] == 7 and want["status"] == 0
    check(run_raw(cases.image(name), dict(nfeatures=7), 7), want, "nfeatures = cap")
    want = cases.want(name, 7, 8)
    assert want["count"] == 7 and want["status"] == M.STATUS_TRUNCATED
    check(run_raw(cases.image(name), dict(nfeatures=8), 7), want, "nfeatures = cap + 1")


def test_more_candidates_than_the_limit(gpu):
    """the smallest image that passes ISX_SIFT_MAX_CANDIDATES at contrast_threshold 0 (found with the model; a lattice of small blobs, since
    white noise stays below the limit up to ISX_SIFT_MAX_PIXELS): the first in scan order are kept and ISX_SIFT_CANDIDATES_DROPPED is set;
    one period less stays below the limit"""
    cap = 64
    for side, status in ((cases.DROPPED_SIDE, M.STATUS_CANDIDATES | M.STATUS_TRUNCATED), (cases.DROPPED_SIDE - cases.DROPPED_STEP, M.STATUS_TRUNCATED)):
        img = cases.dots(side)
        want = M.find(img, M.Params(contrast_threshold=0.0), cap)
        assert want["status"] == status, (side, want["status"])
        check(run_raw(img, dict(contrast_threshold=0.0), cap), want, "dots %d" % side)


def test_host_mats(gpu):
    name = "contrast-0"
    want = cases.want(name)
    check(run_raw(cases.image(name), cases.CASES[name][1], want["count"] + ROOM, device=False), want, name)


def test_strided_and_unaligned_mats(gpu):
    """an image at an odd byte offset with an odd pitch; outputs that are column windows of wider mats (a pitch wider than the row), one float
    off a 16-byte boundary; the outputs differ in their row counts and the smallest is the cap"""
    import torch
    name = "rig-bgr"
    want, img = cases.want(name), cases.image(name)
    n, (h, w) = want["count"], img.shape[:2]
    for device in (True, False):
        if device:
            flat = torch.zeros(h * (w * 3 + 7) + 1, dtype=torch.uint8, device="cuda")
            view = torch.as_strided(flat, (h, w, 3), (w * 3 + 7, 3, 1), 1)
            view.copy_(torch.from_numpy(np.array(img)).cuda())
            big = [torch.full((n + r, c + 3), SENTINEL, dtype=torch.float32, device="cuda") for r, c in ((ROOM, 2), (ROOM + 5, 5), (ROOM + 9, 128))]
            cs = torch.full((1, 2), SENTINEL, dtype=torch.int32, device="cuda")
        else:
            flat = np.zeros(h * (w * 3 + 7) + 1, np.uint8)
            view = np.lib.stride_tricks.as_strided(flat[1:], (h, w, 3), (w * 3 + 7, 3, 1))
            view[...] = img
            big = [np.full((n + r, c + 3), SENTINEL, np.float32) for r, c in ((ROOM, 2), (ROOM + 5, 5), (ROOM + 9, 128))]
            cs = np.full((1, 2), SENTINEL, np.int32)
        kp, meta, desc = big[0][:, 1:3], big[1][:, 1:6], big[2][:, 1:129]
        features.sift_find(view, params_of(), kp, meta, desc, cs, 0, None)
        torch.cuda.synchronize()
        check((_np(kp), _np(meta), _np(desc), _np(cs)), want, "strided device=%s" % device)
        for b, c in zip(big, (2, 5, 128)):
            b = _np(b)
            assert (b[:, 0] == SENTINEL).all() and (b[:, c + 1:] == SENTINEL).all(), "columns outside the window were written"


def test_side_stream(gpu):
    import torch
    s = torch.cuda.Stream()
    name = "blob-1-3"
    want = cases.want(name)
    with torch.cuda.stream(s):
        got = run_raw(cases.image(name), {}, want["count"] + ROOM, stream=s)
    check(got, want, "side stream")


def test_several_sizes_on_one_scratch(gpu):
    features.SiftFeaturesFinder.release()
    for name in ("rig-gray", "side-6", "odd-33x47", "strip-6x200", "side-1", "rig-gray"):
        want = cases.want(name)
        check(run_raw(cases.image(name), cases.CASES[name][1], want["count"] + ROOM), want, name)


def test_finder_class(gpu):
    """SiftFeaturesFinder.find on device and host images: ImageFeatures with 128 float32 a row and a meta of five columns"""
    views = [cases.image(n) for n in ("rig-bgr", "rig-gray")]
    wants = [cases.want(n) for n in ("rig-bgr", "rig-gray")]
    finder = features.SiftFeaturesFinder()
    for put in (_dev, lambda a: a):
        feats = finder.find([put(v) for v in views])
        for f, w, v in zip(feats, wants, views):
            assert f.img_size == (v.shape[1], v.shape[0]) and f.status == 0
            assert np.array_equal(_np(f.keypoints), w["keypoints"]) and np.array_equal(_np(f.meta), w["meta"]) and np.array_equal(_np(f.descriptors), w["descriptors"])
    few = features.SiftFeaturesFinder(max_keypoints=50).find([_dev(views[1])])[0]
    assert few.status == features.SIFT_TRUNCATED and np.array_equal(_np(few.descriptors), wants[1]["descriptors"][:50])
    best = features.SiftFeaturesFinder(nfeatures=20).find([_dev(views[1])])[0]
    assert best.status == 0 and np.array_equal(_np(best.descriptors), wants[1]["descriptors"][:20])


def test_captured_find_replays(gpu):
    """reserve, one eager find, the same find captured and replayed twice on a rewritten image: every replay equals the eager find of that
    image and the model"""
    import torch
    imgs = [cases.rig_view(1, 1), cases.rig_view(0, 1)]            # two 320 x 240 one-channel images
    wants = [cases.want("rig-gray"), M.find(imgs[1], M.Params())]
    cap = max(w["count"] for w in wants) + ROOM
    q = params_of()
    s = torch.cuda.Stream()
    features.SiftFeaturesFinder.release()
    features.sift_reserve(q, 320, 240, cap, 0)
    image = _dev(imgs[0])
    kp, meta, desc, cs = outputs(cap, _dev)
    with torch.cuda.stream(s):
        features.sift_find(image, q, kp, meta, desc, cs, 0, s)
    torch.cuda.synchronize()
    check((_np(kp), _np(meta), _np(desc), _np(cs)), wants[0], "eager")
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        features.sift_find(image, q, kp, meta, desc, cs, 0, s)
    for k in (1, 0):
        with torch.cuda.stream(s):
            image.copy_(torch.from_numpy(np.ascontiguousarray(imgs[k])).cuda())
            for t in (kp, meta, desc):
                t.fill_(SENTINEL)
        s.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check((_np(kp), _np(meta), _np(desc), _np(cs)), wants[k], "replay of image %d" % k)


def test_captured_find_refuses_host_mats_and_a_small_scratch(gpu):
    import torch
    q = params_of()
    s = torch.cuda.Stream()
    features.SiftFeaturesFinder.release()
    features.sift_reserve(q, 47, 33, 8, 0)
    small, large = _dev(cases.image("odd-33x47")), _dev(cases.image("rig-gray"))
    kp, meta, desc, cs = outputs(8, _dev)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        for img, outs in ((large, (kp, meta, desc, cs)), (small, (kp, meta, desc, np.zeros((1, 2), np.int32))), (np.zeros((33, 47), np.uint8), (kp, meta, desc, cs))):
            with pytest.raises(_lib.IsxError) as e:
                features.sift_find(img, q, *outs, 0, s)
            assert e.value.code == 3, e.value
        features.sift_find(small, q, kp, meta, desc, cs, 0, s)
    g.replay()
    torch.cuda.synchronize()
    want = M.find(_np(small), M.Params(), 8)
    check((_np(kp), _np(meta), _np(desc), _np(cs)), want, "captured after the refusals")
    features.SiftFeaturesFinder.release()


def _refusals():
    f32, i32 = np.float32, np.int32

    def setp(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a["q"], k, v)
        return f

    def seta(**kw):
        def f(a):
            a.update({k: v() for k, v in kw.items()})
        return f
    INVALID, TYPE, UNSUPPORTED, SIZE = 1, 2, 6, 7
    nan = float("nan")
    return [
        ("nfeatures -1", setp(nfeatures=-1), INVALID), ("contrast_threshold < 0", setp(contrast_threshold=-1e-9), INVALID),
        ("contrast_threshold nan", setp(contrast_threshold=nan), INVALID), ("edge_threshold 0", setp(edge_threshold=0.0), INVALID),
        ("edge_threshold nan", setp(edge_threshold=nan), INVALID), ("sigma nan", setp(sigma=nan), INVALID),
        ("n_octave_layers 2", setp(n_octave_layers=2), UNSUPPORTED), ("n_octave_layers 4", setp(n_octave_layers=4), UNSUPPORTED),
        ("sigma 1.5", setp(sigma=1.5), UNSUPPORTED),
        ("side past the limit", seta(image=lambda: np.zeros((1, features.SIFT_MAX_SIDE + 1), np.uint8)), UNSUPPORTED),
        ("pixels past the limit", seta(image=lambda: np.zeros((2048, 4097), np.uint8)), UNSUPPORTED),
        ("image type", seta(image=lambda: np.zeros((40, 40), f32)), TYPE), ("empty image", seta(image=lambda: np.zeros((1, 40), np.uint8)[:0]), SIZE),
        ("keypoints type", seta(kp=lambda: np.full((4, 2), SENTINEL, i32)), TYPE), ("descriptors type", seta(desc=lambda: np.full((4, 128), SENTINEL, np.uint8)), TYPE),
        ("meta 4 wide", seta(meta=lambda: np.full((4, 4), SENTINEL, f32)), SIZE), ("descriptors 127 wide", seta(desc=lambda: np.full((4, 127), SENTINEL, f32)), SIZE),
        ("keypoints 1 wide", seta(kp=lambda: np.full((4, 1), SENTINEL, f32)), SIZE), ("no rows", seta(meta=lambda: np.full((1, 5), SENTINEL, f32)[:0]), SIZE),
        ("count_status 1 x 1", seta(cs=lambda: np.full((1, 1), SENTINEL, i32)), SIZE),
        ("misaligned descriptors", seta(desc=lambda: np.full(4 * 128 * 4 + 8, SENTINEL, np.uint8)[2:2 + 4 * 128 * 4].view(f32).reshape(4, 128)), INVALID),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_refusals_leave_the_outputs_untouched(gpu, case):
    what, change, code = case
    img = cases.image("contrast-0")
    a = dict(image=np.array(img), q=params_of(), kp=np.full((4, 2), SENTINEL, np.float32), meta=np.full((4, 5), SENTINEL, np.float32),
             desc=np.full((4, 128), SENTINEL, np.float32), cs=np.full((1, 2), SENTINEL, np.int32))
    change(a)
    before = {k: a[k].copy() for k in ("kp", "meta", "desc", "cs")}
    with pytest.raises(_lib.IsxError) as e:
        features.sift_find(a["image"], a["q"], a["kp"], a["meta"], a["desc"], a["cs"], 0, None)
    assert e.value.code == code, (what, e.value)
    for k, b in before.items():
        assert a[k].tobytes() == b.tobytes(), (what, k)


def test_limits_are_admitted_at_the_limit(gpu):
    """one step inside either limit is planned: isx_sift_reserve of the widest and of the largest image succeeds on the host side's checks
    (the reservation itself is not made: cap 0 is refused after them)"""
    lib, q = _lib.load(), params_of()
    assert lib.isx_sift_reserve(C.byref(q), features.SIFT_MAX_SIDE, 1, 0, 0) == 7 and lib.isx_sift_reserve(C.byref(q), 4096, 2048, 0, 0) == 7
    assert lib.isx_sift_reserve(C.byref(q), 3840, 2160, 0, 0) == 7


def test_null_arguments_and_device_mismatch(gpu):
    lib = _lib.load()
    img, q = np.array(cases.image("contrast-0")), params_of()
    kp, meta, desc, cs = outputs(4, lambda a: np.array(a))
    mats = [C.byref(_lib.as_mat(a)) for a in (img, kp, meta, desc, cs)]
    for hole in range(6):
        args = [mats[0], C.byref(q)] + mats[1:]
        args[hole] = None
        assert lib.isx_sift_find(*args, 0, None) == 1, hole
    assert lib.isx_sift_default_params(None) == 1
    assert lib.isx_sift_reserve(C.byref(q), 0, 10, 4, 0) == 7 and lib.isx_sift_reserve(C.byref(q), 10, 10, 0, 0) == 7
    assert lib.isx_sift_reserve(C.byref(q), features.SIFT_MAX_SIDE + 1, 1, 4, 0) == 6
    wrong = _lib.as_mat(_dev(img))
    wrong.device = 1
    assert lib.isx_sift_find(C.byref(wrong), C.byref(q), *mats[1:], 0, None) == 1
    assert (kp == SENTINEL).all() and (cs == SENTINEL).all()


@pytest.mark.parametrize("fn", sorted(M.MATH_FUNCS))
def test_device_math_equals_the_host_and_the_model(gpu, fn):
    """isx_selftest_sift_math_device (the device compilation of sift_math.hpp) against isx_selftest_sift_math and sift_np, bit for bit, on
    the arguments the finder can produce and on the edges of the defined range"""
    lib, F = _lib.load(), C.POINTER(C.c_float)
    lo, hi = ((-32.0, 0.0), (0.0, 2.0))[fn]
    x = np.concatenate([np.linspace(lo, hi, 200001), np.linspace(-110, 95, 4001), [-200, -104.5, -152, 89.5, 130, np.nan, np.inf, -np.inf, 1e-30, -0.0]]).astype(np.float32)
    host, dev = np.empty_like(x), np.empty_like(x)
    assert lib.isx_selftest_sift_math(fn, len(x), x.ctypes.data_as(F), host.ctypes.data_as(F)) == 0
    assert lib.isx_selftest_sift_math_device(fn, len(x), x.ctypes.data_as(F), dev.ctypes.data_as(F)) == 0
    want = M.MATH_FUNCS[fn][1](x)
    assert np.array_equal(host.view(np.uint32), want.view(np.uint32)) and np.array_equal(dev.view(np.uint32), want.view(np.uint32))
