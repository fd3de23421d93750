"""isx_orb_find at its edges: every refusal leaves every mat as it was, outputs inside guard bands are written in rows [0, count) only, a
call captured after isx_orb_reserve replays to what the eager call gives, and a captured call that would have to grow the scratch, or that
is handed a host mat, is refused with nothing enqueued."""
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
from helpers import guarded  # noqa: E402
from helpers import orb_np as M  # noqa: E402
from imagestitch_amd import _lib, features  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7
P = M.Params(grid=(2, 1), n_features=120, nlevels=3)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _params(p=P):
    q = features.default_params()
    q.grid_width, q.grid_height, q.n_features, q.scale_factor, q.nlevels, q.fast_threshold = p.grid[0], p.grid[1], p.n_features, p.scale_factor, p.nlevels, p.fast_threshold
    return q


@pytest.fixture(scope="module")
def scene():
    img = cases.scene(150, 200, 21, 3)
    return img, M.find(img, P)


def _outputs(where, cap, seed=30):
    return [guarded.guarded((cap, 2), np.float32, where, "aligned", seed, "keypoints"), guarded.guarded((cap, 4), np.float32, where, "aligned", seed + 1, "meta"),
            guarded.guarded((cap, 32), np.uint8, where, "odd", seed + 2, "descriptors"), guarded.guarded((1, 2), np.int32, where, "aligned", seed + 3, "count_status")]


@pytest.mark.parametrize("where", ["device", "host"])
def test_every_refusal_writes_nothing(gpu, scene, where):
    import torch
    img, _ = scene
    cap = features.capacity(_params())
    g_img = guarded.guarded_like(img, where, "odd", 29, "image")
    outs = _outputs(where, cap)
    pat = np.ascontiguousarray(M.default_pattern())

    def refused(code, image=None, params=None, pattern=None, views=None, word=None):
        v = views or [g.view for g in outs]
        with pytest.raises(_lib.IsxError) as e:
            features.orb_find(g_img.view if image is None else image, params or _params(), v[0], v[1], v[2], v[3], pattern)
        assert e.value.code == code, e.value
        assert word is None or word in e.value.msg, e.value.msg
        torch.cuda.synchronize()
        g_img.check(written=guarded.NOTHING)
        for g in outs:
            g.check(written=guarded.NOTHING)

    def with_field(field, value):
        q = _params()
        setattr(q, field, value)
        return q

    put = _dev if where == "device" else np.array
    for field, value, code in (("grid_width", 0, ERR_INVALID), ("n_features", -1, ERR_INVALID), ("scale_factor", 1.0, ERR_INVALID), ("nlevels", 0, ERR_INVALID),
                               ("nlevels", 9, ERR_INVALID), ("fast_threshold", 255, ERR_INVALID), ("patch_size", 29, ERR_UNSUPPORTED), ("edge_threshold", 30, ERR_UNSUPPORTED),
                               ("wta_k", 4, ERR_UNSUPPORTED), ("first_level", 1, ERR_UNSUPPORTED), ("score_type", features.FAST_SCORE, ERR_UNSUPPORTED),
                               ("n_features", 30000, ERR_UNSUPPORTED), ("grid_width", 400, ERR_UNSUPPORTED), ("grid_width", 201, ERR_INVALID)):
        refused(code, params=with_field(field, value))
    refused(ERR_TYPE, image=put(np.zeros((150, 200), np.float32)), word="image")
    refused(ERR_TYPE, pattern=put(pat.astype(np.float32)), word="pattern")
    refused(ERR_SIZE, pattern=put(pat[:511]), word="512 x 2")
    views = [g.view for g in outs]
    refused(ERR_TYPE, views=[put(np.zeros((cap, 2), np.int32))] + views[1:], word="keypoints")
    refused(ERR_TYPE, views=views[:2] + [put(np.zeros((cap, 32), np.float32))] + views[3:], word="descriptors")
    refused(ERR_SIZE, views=[views[0][:cap - 1]] + views[1:], word="keypoints")
    refused(ERR_SIZE, views=[views[0], views[1][:, :3]] + views[2:], word="meta")
    refused(ERR_SIZE, views=views[:2] + [views[2][:cap - 1]] + views[3:], word="descriptors")
    refused(ERR_SIZE, views=views[:3] + [views[3][:, :1]], word="count_status")
    bad = pat.copy()
    bad[511, 0] = 16
    if where == "host":
        refused(ERR_INVALID, pattern=bad, word="outside the 31 x 31 patch")
    if where == "device":
        import ctypes as C
        wrong_device = features.as_mat(views[0])
        wrong_device.device = 1                                         # a mat of another device
        with pytest.raises(_lib.IsxError) as e:
            _lib.check(_lib.load().isx_orb_find(C.byref(features.as_mat(g_img.view)), C.byref(_params()), None, C.byref(wrong_device), C.byref(features.as_mat(views[1])),
                                                C.byref(features.as_mat(views[2])), C.byref(features.as_mat(views[3])), 0, None))
        assert e.value.code == ERR_INVALID and "device" in e.value.msg
    # and the call that is not refused, on the same mats
    features.orb_find(g_img.view, _params(), *views)
    torch.cuda.synchronize()
    n = scene[1].count
    assert tuple(outs[3].get()[0]) == (n, scene[1].status) and n > 0
    rows = np.zeros((cap, 1), bool)
    rows[:n] = True
    g_img.check(written=guarded.NOTHING)
    for g, w in zip(outs[:3], (2, 4, 32)):
        g.check(written=np.repeat(rows, w, 1))
    assert np.array_equal(outs[0].get()[:n], scene[1].keypoints) and np.array_equal(outs[1].get()[:n], scene[1].meta) and np.array_equal(outs[2].get()[:n], scene[1].descriptors)


def test_a_captured_call_replays_to_the_eager_one(gpu, scene):
    """reserve, capture one find on a side stream, replay it on rewritten images: every replay equals the eager call and the model"""
    import torch
    img, want = scene
    q = _params()
    cap = features.capacity(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    features.OrbFeaturesFinder.release()
    features.orb_reserve(q, img.shape[1], img.shape[0])
    with torch.cuda.stream(s):
        d_img = _dev(img)
        kp, meta = torch.zeros((cap, 2), dtype=torch.float32, device="cuda"), torch.zeros((cap, 4), dtype=torch.float32, device="cuda")
        desc, cs = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda"), torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        features.orb_find(d_img, q, kp, meta, desc, cs, None, 0, s)
    for k, other in enumerate((img, cases.scene(150, 200, 22, 3), np.zeros_like(img))):
        w = M.find(other, P)
        with torch.cuda.stream(s):
            d_img.copy_(torch.from_numpy(other).cuda())
            for t in (kp, meta, desc, cs):
                t.zero_()
        s.synchronize()
        g.replay()
        torch.cuda.synchronize()
        n = int(_np(cs)[0, 0])
        got = [_np(kp)[:n].copy(), _np(meta)[:n].copy(), _np(desc)[:n].copy()]
        assert (n, int(_np(cs)[0, 1])) == (w.count, w.status), k
        assert np.array_equal(got[0], w.keypoints) and np.array_equal(got[1], w.meta) and np.array_equal(got[2], w.descriptors), k
        with torch.cuda.stream(s):
            e_kp, e_meta, e_desc, e_cs = (torch.zeros_like(t) for t in (kp, meta, desc, cs))
            features.orb_find(d_img, q, e_kp, e_meta, e_desc, e_cs, None, 0, s)      # the eager call on the same image
        s.synchronize()
        assert int(_np(e_cs)[0, 0]) == n and np.array_equal(_np(e_kp)[:n], got[0]) and np.array_equal(_np(e_meta)[:n], got[1]) and np.array_equal(_np(e_desc)[:n], got[2]), k
    assert want.count > 0
    del g
    features.OrbFeaturesFinder.release()


def test_a_captured_call_that_would_grow_the_scratch_is_refused(gpu, scene):
    """On a capturing stream: nothing reserved, a host mat, an image larger than what was reserved -> ISX_ERR_STATE with nothing enqueued;
    the capture stays usable and a find that fits is captured after them."""
    import torch
    img, want = scene
    big = np.zeros((1200, 1500, 3), np.uint8)             # four pyramids of it pass what the scratch holds, rounded up as it is
    q = _params()
    cap = features.capacity(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    features.OrbFeaturesFinder.release()
    with torch.cuda.stream(s):
        d_img, d_big = _dev(img), _dev(big)
        outs = [torch.full((cap, 2), 5.0, device="cuda"), torch.full((cap, 4), 5.0, device="cuda"), torch.full((cap, 32), 5, dtype=torch.uint8, device="cuda"),
                torch.full((1, 2), 5, dtype=torch.int32, device="cuda")]
        x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(_lib.IsxError) as e:                         # nothing reserved at all
            features.orb_find(d_img, q, *outs, None, 0, s)
        assert e.value.code == ERR_STATE and "reserve" in e.value.msg, e.value.msg
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0 and all(bool((t == 5).all()) for t in outs)
    features.orb_reserve(q, img.shape[1], img.shape[0])
    host_kp = np.full((cap, 2), 5, np.float32)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(_lib.IsxError) as e:
            features.orb_find(d_img, q, host_kp, *outs[1:], None, 0, s)
        assert e.value.code == ERR_STATE and "host" in e.value.msg, e.value.msg
        with pytest.raises(_lib.IsxError) as e:
            features.orb_find(d_img, q, *outs, M.default_pattern(), 0, s)      # a host pattern is a host mat
        assert e.value.code == ERR_STATE and "host" in e.value.msg, e.value.msg
        with pytest.raises(_lib.IsxError) as e:
            features.orb_find(d_big, q, *outs, None, 0, s)
        assert e.value.code == ERR_STATE and "reserve" in e.value.msg, e.value.msg
        features.orb_find(d_img, q, *outs, None, 0, s)
    assert (host_kp == 5).all()
    g.replay()
    torch.cuda.synchronize()
    n = want.count
    assert float(x[0]) == 2.0 and tuple(_np(outs[3])[0]) == (n, want.status)
    assert np.array_equal(_np(outs[0])[:n], want.keypoints) and np.array_equal(_np(outs[2])[:n], want.descriptors) and bool((outs[0][n:] == 5).all())
    del g
    features.OrbFeaturesFinder.release()
