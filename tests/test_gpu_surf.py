"""The SURF finder on the GPU (isx_surf_find, imagestitch_amd/features.py) against the NumPy model of tests/helpers/surf_np.py:
np.array_equal on the count, the status, the keypoints, meta and descriptors, for every case of tests/surf_cases.py; cap below, at and above
the count; host, device, strided and unaligned mats; a side stream; two sizes on one scratch; a captured find; every refusal."""
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import surf_cases as cases  # noqa: E402
from helpers import surf_np as M  # noqa: E402
from imagestitch_amd import _lib, features  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 123
ROOM = 16               # rows past the model's count


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def params_of(hess_thresh=300.0, num_octaves=3, num_layers=4):
    q = features.surf_default_params()
    q.hess_thresh, q.num_octaves, q.num_layers, q.num_octaves_descr, q.num_layers_descr = hess_thresh, num_octaves, num_layers, num_octaves, num_layers
    return q


def outputs(cap, put):
    return (put(np.full((cap, 2), SENTINEL, np.float32)), put(np.full((cap, 5), SENTINEL, np.float32)), put(np.full((cap, 64), SENTINEL, np.float32)),
            put(np.full((1, 2), SENTINEL, np.int32)))


def run_raw(image, kw, cap, device=True, stream=None):
    """isx_surf_find on dense mats pre-filled with a sentinel: (keypoints, meta, descriptors, count_status) as NumPy arrays, whole mats"""
    import torch
    put = _dev if device else (lambda a: np.array(a))
    kp, meta, desc, cs = outputs(cap, put)
    features.surf_find(put(image), params_of(**kw), kp, meta, desc, cs, 0, stream)
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
    """the large blobs give sizes of the top octave and windows longer than LDS could hold; the border scene has a keypoint within 11.5 px of
    every border (the search margin of the 15-filter keeps a maximum 10 px inside), so windows and orientation discs leave the image"""
    big = cases.want("large-blobs")["meta"]
    assert (big[:, 3] == 2).sum() >= 3 and big[:, 0].max() >= 120
    k, (h, w) = cases.want("border")["keypoints"], cases.image("border").shape
    assert k[:, 0].min() < 11.5 and k[:, 1].min() < 11.5 and w - 1 - k[:, 0].max() < 11.5 and h - 1 - k[:, 1].max() < 11.5
    assert cases.want("thresh-0")["count"] > 0 and cases.want("thresh-huge")["count"] == 0 and cases.want("large-blobs-4-octaves")["meta"][:, 3].max() == 3


@pytest.mark.parametrize("delta", [None, -1, 0, 1])
def test_cap_below_at_and_above_the_count(gpu, delta):
    name = "rig-gray"
    n = cases.want(name)["count"]
    cap = 1 if delta is None else n + delta
    want = cases.want(name, cap)
    assert want["count"] == min(cap, n) and want["status"] == (M.STATUS_TRUNCATED if cap < n else 0)
    assert np.array_equal(want["descriptors"], cases.want(name)["descriptors"][:cap])       # a prefix of the canonical order
    check(run_raw(cases.image(name), {}, cap), want, "cap %d" % cap)


def test_host_mats(gpu):
    name = "border"
    want = cases.want(name)
    check(run_raw(cases.image(name), cases.CASES[name][1], want["count"] + ROOM, device=False), want, name)


def test_strided_and_unaligned_mats(gpu):
    """an image at an odd byte offset with an odd pitch; outputs that are column windows of wider mats, one float off a 16-byte boundary;
    the outputs differ in their row counts and the smallest is the cap"""
    import torch
    name = "rig-bgr"
    want, img = cases.want(name), cases.image(name)
    n, (h, w) = want["count"], img.shape[:2]
    for device in (True, False):
        if device:
            flat = torch.zeros(h * (w * 3 + 7) + 1, dtype=torch.uint8, device="cuda")
            view = torch.as_strided(flat, (h, w, 3), (w * 3 + 7, 3, 1), 1)
            view.copy_(torch.from_numpy(img).cuda())
            big = [torch.full((n + r, c + 3), SENTINEL, dtype=torch.float32, device="cuda") for r, c in ((ROOM, 2), (ROOM + 5, 5), (ROOM + 9, 64))]
            cs = torch.full((1, 2), SENTINEL, dtype=torch.int32, device="cuda")
        else:
            flat = np.zeros(h * (w * 3 + 7) + 1, np.uint8)
            view = np.lib.stride_tricks.as_strided(flat[1:], (h, w, 3), (w * 3 + 7, 3, 1))
            view[...] = img
            big = [np.full((n + r, c + 3), SENTINEL, np.float32) for r, c in ((ROOM, 2), (ROOM + 5, 5), (ROOM + 9, 64))]
            cs = np.full((1, 2), SENTINEL, np.int32)
        kp, meta, desc = big[0][:, 1:3], big[1][:, 1:6], big[2][:, 1:65]
        features.surf_find(view, params_of(), kp, meta, desc, cs, 0, None)
        torch.cuda.synchronize()
        check((_np(kp), _np(meta), _np(desc), _np(cs)), want, "strided device=%s" % device)
        for b, c in zip(big, (2, 5, 64)):
            b = _np(b)
            assert (b[:, 0] == SENTINEL).all() and (b[:, c + 1:] == SENTINEL).all(), "columns outside the window were written"


def test_side_stream(gpu):
    import torch
    s = torch.cuda.Stream()
    name = "large-blobs"
    want = cases.want(name)
    with torch.cuda.stream(s):
        got = run_raw(cases.image(name), {}, want["count"] + ROOM, stream=s)
    check(got, want, "side stream")


def test_two_sizes_on_one_scratch(gpu):
    features.SurfFeaturesFinder.release()
    for name in ("rig-gray", "side-40", "large-blobs", "strip-33x200", "rig-gray"):
        want = cases.want(name)
        check(run_raw(cases.image(name), cases.CASES[name][1], want["count"] + ROOM), want, name)


def test_finder_class(gpu):
    """SurfFeaturesFinder.find on device and host images: ImageFeatures with 64 float32 a row and a meta of five columns"""
    views = [cases.image(n) for n in ("rig-bgr", "rig-gray")]
    wants = [cases.want(n) for n in ("rig-bgr", "rig-gray")]
    finder = features.SurfFeaturesFinder()
    for put in (_dev, lambda a: a):
        feats = finder.find([put(v) for v in views])
        for f, w, v in zip(feats, wants, views):
            assert f.img_size == (v.shape[1], v.shape[0]) and f.status == 0
            assert np.array_equal(_np(f.keypoints), w["keypoints"]) and np.array_equal(_np(f.meta), w["meta"]) and np.array_equal(_np(f.descriptors), w["descriptors"])
    few = features.SurfFeaturesFinder(max_keypoints=50).find([_dev(views[1])])[0]
    assert few.status == features.SURF_TRUNCATED and np.array_equal(_np(few.descriptors), wants[1]["descriptors"][:50])


def test_captured_find_replays(gpu):
    """reserve, one eager find, the same find captured and replayed twice on a rewritten image: every replay equals the eager find of that
    image and the model"""
    import torch
    names = ("rig-gray", "octaves-1")            # two 320 x 240 one-channel images
    imgs = [cases.image(n) for n in names]
    wants = [cases.want("rig-gray"), M.find(imgs[1], M.Params())]
    cap = max(w["count"] for w in wants) + ROOM
    q = params_of()
    s = torch.cuda.Stream()
    features.SurfFeaturesFinder.release()
    features.surf_reserve(q, 320, 240, cap, 0)
    image = _dev(imgs[0])
    kp, meta, desc, cs = outputs(cap, _dev)
    with torch.cuda.stream(s):
        features.surf_find(image, q, kp, meta, desc, cs, 0, s)
    torch.cuda.synchronize()
    check((_np(kp), _np(meta), _np(desc), _np(cs)), wants[0], "eager")
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        features.surf_find(image, q, kp, meta, desc, cs, 0, s)
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
    features.SurfFeaturesFinder.release()
    features.surf_reserve(q, 64, 48, 8, 0)
    small, large = _dev(cases.blobs(48, 64, 3, (2.5,), 4)), _dev(cases.image("rig-gray"))
    kp, meta, desc, cs = outputs(8, _dev)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        for img, outs in ((large, (kp, meta, desc, cs)), (small, (kp, meta, desc, np.zeros((1, 2), np.int32))), (np.zeros((48, 64), np.uint8), (kp, meta, desc, cs))):
            with pytest.raises(_lib.IsxError) as e:
                features.surf_find(img, q, *outs, 0, s)
            assert e.value.code == 3, e.value
        features.surf_find(small, q, kp, meta, desc, cs, 0, s)
    g.replay()
    torch.cuda.synchronize()
    want = M.find(_np(small), M.Params(), 8)
    check((_np(kp), _np(meta), _np(desc), _np(cs)), want, "captured after the refusals")
    features.SurfFeaturesFinder.release()


def _refusals():
    img = cases.image("side-40")
    f32, i32 = np.float32, np.int32

    def base():
        return dict(image=np.array(img), q=params_of(), kp=np.full((4, 2), SENTINEL, f32), meta=np.full((4, 5), SENTINEL, f32), desc=np.full((4, 64), SENTINEL, f32),
                    cs=np.full((1, 2), SENTINEL, i32))

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
    return [
        ("num_octaves 0", setp(num_octaves=0, num_octaves_descr=0), INVALID), ("num_octaves 5", setp(num_octaves=5, num_octaves_descr=5), INVALID),
        ("num_layers 0", setp(num_layers=0, num_layers_descr=0), INVALID), ("num_layers 5", setp(num_layers=5, num_layers_descr=5), INVALID),
        ("hess_thresh < 0", setp(hess_thresh=-1.0), INVALID), ("hess_thresh nan", setp(hess_thresh=float("nan")), INVALID),
        ("descr octaves", setp(num_octaves_descr=4), UNSUPPORTED), ("descr layers", setp(num_layers_descr=2), UNSUPPORTED),
        ("extended", setp(extended=1), UNSUPPORTED), ("upright", setp(upright=1), UNSUPPORTED),
        ("side past the limit", seta(image=lambda: np.zeros((1, features.SURF_MAX_SIDE + 1), np.uint8)), UNSUPPORTED),
        ("pixels past the limit", seta(image=lambda: np.zeros((4096, 4097), np.uint8)), UNSUPPORTED),
        ("image type", seta(image=lambda: np.zeros((40, 40), f32)), TYPE), ("empty image", seta(image=lambda: np.zeros((1, 40), np.uint8)[:0]), SIZE),
        ("keypoints type", seta(kp=lambda: np.full((4, 2), SENTINEL, i32)), TYPE), ("descriptors type", seta(desc=lambda: np.full((4, 64), SENTINEL, np.uint8)), TYPE),
        ("meta 4 wide", seta(meta=lambda: np.full((4, 4), SENTINEL, f32)), SIZE), ("descriptors 63 wide", seta(desc=lambda: np.full((4, 63), SENTINEL, f32)), SIZE),
        ("keypoints 1 wide", seta(kp=lambda: np.full((4, 1), SENTINEL, f32)), SIZE), ("no rows", seta(meta=lambda: np.full((1, 5), SENTINEL, f32)[:0]), SIZE),
        ("count_status 1 x 1", seta(cs=lambda: np.full((1, 1), SENTINEL, i32)), SIZE),
        ("misaligned descriptors", seta(desc=lambda: np.full(4 * 64 * 4 + 8, SENTINEL, np.uint8)[2:2 + 4 * 64 * 4].view(f32).reshape(4, 64)), INVALID),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_refusals_leave_the_outputs_untouched(gpu, case):
    what, change, code = case
    img = cases.image("side-40")
    a = dict(image=np.array(img), q=params_of(), kp=np.full((4, 2), SENTINEL, np.float32), meta=np.full((4, 5), SENTINEL, np.float32),
             desc=np.full((4, 64), SENTINEL, np.float32), cs=np.full((1, 2), SENTINEL, np.int32))
    change(a)
    before = {k: a[k].copy() for k in ("kp", "meta", "desc", "cs")}
    with pytest.raises(_lib.IsxError) as e:
        features.surf_find(a["image"], a["q"], a["kp"], a["meta"], a["desc"], a["cs"], 0, None)
    assert e.value.code == code, (what, e.value)
    for k, b in before.items():
        assert a[k].tobytes() == b.tobytes(), (what, k)


def test_null_arguments_and_device_mismatch(gpu):
    import ctypes as C
    lib = _lib.load()
    img, q = np.array(cases.image("side-40")), params_of()
    kp, meta, desc, cs = outputs(4, lambda a: np.array(a))
    mats = [C.byref(_lib.as_mat(a)) for a in (img, kp, meta, desc, cs)]
    for hole in range(6):
        args = [mats[0], C.byref(q)] + mats[1:]
        args[hole] = None
        assert lib.isx_surf_find(*args, 0, None) == 1, hole
    assert lib.isx_surf_default_params(None) == 1
    assert lib.isx_surf_reserve(C.byref(q), 0, 10, 4, 0) == 7 and lib.isx_surf_reserve(C.byref(q), 10, 10, 0, 0) == 7
    assert lib.isx_surf_reserve(C.byref(q), features.SURF_MAX_SIDE + 1, 1, 4, 0) == 6
    wrong = _lib.as_mat(_dev(img))
    wrong.device = 1
    assert lib.isx_surf_find(C.byref(wrong), C.byref(q), *mats[1:], 0, None) == 1
    assert (kp == SENTINEL).all() and (cs == SENTINEL).all()
