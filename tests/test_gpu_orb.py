"""The features finder on the GPU (isx_orb_find, imagestitch_amd/features.py) against the NumPy model of tests/helpers/orb_np.py,
np.array_equal for every output, the count and the status: noise over blobs on one cell and on three, one channel, three and four, levels
that are empty or too narrow, an image without a keypoint, ties at both cuts with and without ISX_ORB_TRUNCATED, widths either side of a
multiple of 64, host and device mats, an unaligned pitch, a caller's pattern and cell 0 of the reference's own image."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
from helpers import guarded  # noqa: E402
from helpers import orb_np as M  # noqa: E402
from imagestitch_amd import features  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 123


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def params_of(p):
    q = features.default_params()
    q.grid_width, q.grid_height, q.n_features, q.scale_factor, q.nlevels, q.fast_threshold = p.grid[0], p.grid[1], p.n_features, p.scale_factor, p.nlevels, p.fast_threshold
    return q


def run_raw(image, p, pattern=None, device=True, stream=None):
    """isx_orb_find on dense mats pre-filled with a sentinel: (keypoints, meta, descriptors, count_status) as NumPy arrays, whole mats"""
    import torch
    put = _dev if device else (lambda a: np.array(a))
    q = params_of(p)
    cap = features.capacity(q)
    assert cap == M.capacity(p)
    kp, meta = put(np.full((cap, 2), SENTINEL, np.float32)), put(np.full((cap, 4), SENTINEL, np.float32))
    desc, cs = put(np.full((cap, 32), SENTINEL, np.uint8)), put(np.full((1, 2), SENTINEL, np.int32))
    features.orb_find(put(image), q, kp, meta, desc, cs, None if pattern is None else put(pattern), 0, stream)
    torch.cuda.synchronize()
    return _np(kp), _np(meta), _np(desc), _np(cs)


def check(got, want, what=""):
    kp, meta, desc, cs = got
    n = int(cs[0, 0])
    print(what, "count", n, "model", want.count, "status", int(cs[0, 1]), "model", want.status)
    assert n == want.count and int(cs[0, 1]) == want.status, (what, n, want.count, int(cs[0, 1]), want.status)
    assert np.array_equal(kp[:n], want.keypoints), what
    assert np.array_equal(meta[:n].view(np.uint32), want.meta.view(np.uint32).reshape(n, 4)), what      # bits: -0.f and 0.f differ
    assert np.array_equal(desc[:n], want.descriptors), what
    assert (kp[n:] == SENTINEL).all() and (meta[n:] == SENTINEL).all() and (desc[n:] == SENTINEL).all(), what + ": rows from count on were written"


CASES = {
    # 256 x 224 noise over blobs: one cell and three (cells of 85 columns leave levels >= 2 empty), one channel, three and four;
    # at the defaults nothing is cut, with fewer features both cuts act
    "blobs-1x1": (lambda: cases.scene(224, 256, 1), dict(grid=(1, 1))),
    "blobs-1x1-cut": (lambda: cases.scene(224, 256, 1), dict(grid=(1, 1), n_features=200)),
    "blobs-3x1-bgr": (lambda: cases.scene(224, 256, 2, 3), dict(grid=(3, 1))),
    "blobs-3x1-bgr-cut": (lambda: cases.scene(224, 256, 2, 3), dict(grid=(3, 1), n_features=60)),
    "blobs-2x2-bgra": (lambda: cases.scene(224, 256, 7, 4), dict(grid=(2, 2), n_features=300, nlevels=3, scale_factor=1.2)),
    # the top level is 67 x 56: narrower than 63 in one direction, it finds nothing
    "192x160": (lambda: cases.scene(160, 192, 3), dict(grid=(1, 1))),
    # no pixel is 31 from every edge
    "64x64": (lambda: cases.scene(64, 64, 4), dict(grid=(1, 1))),
    # a periodic grid of identical corners: ties at both cuts, more than the room (a checkerboard itself has no 9-arc)
    "ties-truncated": (lambda: cases.dots(224, 256), dict(grid=(1, 1), n_features=100)),
    "ties-final-truncated": (lambda: cases.dots(224, 256, count=100), dict(grid=(1, 1), n_features=50)),
    "ties-fit": (lambda: cases.dots(224, 256, count=40), dict(grid=(1, 1), n_features=50)),
    "plateau": (lambda: cases.squares(224, 256), dict(grid=(1, 1))),
    # one over and one under a multiple of 64; scale 2 takes the 2 x 2 area rule where both sides are even
    "w257": (lambda: cases.scene(130, 257, 5), dict(grid=(1, 1))),
    "w255-2x1": (lambda: cases.scene(130, 255, 6), dict(grid=(2, 1))),
    "scale2": (lambda: cases.scene(200, 256, 8), dict(grid=(1, 1), scale_factor=2.0, nlevels=3, n_features=150)),
    "threshold7": (lambda: cases.scene(160, 192, 9), dict(grid=(1, 1), fast_threshold=7, n_features=400)),
}
_WANT = {}


def want_of(name):
    if name not in _WANT:
        make, kw = CASES[name]
        img, p = make(), M.Params(**kw)
        _WANT[name] = (img, p, M.find(img, p))
    return _WANT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_mats_match_the_model(gpu, name):
    img, p, want = want_of(name)
    check(run_raw(img, p), want, name)


def test_the_cases_cover_the_paths():
    """the model's own counts: the cases do what their comments say"""
    assert want_of("64x64")[2].count == 0 and want_of("64x64")[2].status == 0
    assert want_of("ties-truncated")[2].status == M.STATUS_TRUNCATED and want_of("ties-final-truncated")[2].status == M.STATUS_TRUNCATED
    assert want_of("ties-fit")[2].status == 0 and want_of("ties-fit")[2].count > 40
    octaves = lambda n: set(want_of(n)[2].meta[:, 3].astype(int))      # noqa: E731
    assert octaves("blobs-1x1") == {0, 1, 2, 3, 4} and octaves("blobs-3x1-bgr") == {0, 1} and 4 not in octaves("192x160")
    assert 0 not in octaves("plateau") and want_of("blobs-1x1-cut")[2].count < want_of("blobs-1x1")[2].count


@pytest.mark.parametrize("name", ["blobs-3x1-bgr-cut", "ties-truncated", "64x64"])
def test_host_mats_match_the_model(gpu, name):
    img, p, want = want_of(name)
    check(run_raw(img, p, device=False), want, name + " (host)")


def test_unaligned_pitch_and_guarded_outputs(gpu):
    """the image and every output inside guard bands at odd addresses and pitches: nothing is written outside the rows the count names"""
    import torch
    img, p, want = want_of("blobs-3x1-bgr-cut")
    q = params_of(p)
    cap = features.capacity(q)
    for where in ("device", "host"):
        g_img = guarded.guarded_like(img, where, "odd", 11, "image")
        g_kp, g_meta = guarded.guarded((cap, 2), np.float32, where, "odd", 12, "keypoints"), guarded.guarded((cap, 4), np.float32, where, "odd", 13, "meta")
        g_desc, g_cs = guarded.guarded((cap, 32), np.uint8, where, "odd", 14, "descriptors"), guarded.guarded((1, 2), np.int32, where, "odd", 15, "count_status")
        features.orb_find(g_img.view, q, g_kp.view, g_meta.view, g_desc.view, g_cs.view)
        torch.cuda.synchronize()
        n = want.count
        assert tuple(g_cs.get()[0]) == (n, want.status)
        rows = np.zeros((cap, 1), bool)
        rows[:n] = True
        g_img.check(written=guarded.NOTHING)
        g_kp.check(written=np.repeat(rows, 2, 1)); g_meta.check(written=np.repeat(rows, 4, 1)); g_desc.check(written=np.repeat(rows, 32, 1)); g_cs.check()
        assert np.array_equal(g_kp.get()[:n], want.keypoints) and np.array_equal(g_meta.get()[:n], want.meta) and np.array_equal(g_desc.get()[:n], want.descriptors)


def test_a_callers_pattern(gpu):
    """a pattern of the caller's (here: another seed), as a host mat and as a device mat; a device pattern outside the patch is reported in
    the status word and writes no row"""
    img, p, _ = want_of("blobs-1x1-cut")
    rng = np.random.default_rng(5)
    pattern = rng.integers(-15, 16, (512, 2)).astype(np.int32)
    pattern[:4] = [[15, 15], [-15, -15], [15, -15], [-15, 15]]
    want = M.find(img, p, pattern)
    assert not np.array_equal(want.descriptors, want_of("blobs-1x1-cut")[2].descriptors)
    check(run_raw(img, p, pattern), want, "device pattern")
    check(run_raw(img, p, pattern, device=False), want, "host pattern")
    check(run_raw(img, p), want_of("blobs-1x1-cut")[2], "the default again")
    bad = pattern.copy()
    bad[300, 1] = 16
    check(run_raw(img, p, bad), M.find(img, p, bad), "bad device pattern")
    assert M.find(img, p, bad).status == M.STATUS_BAD_PATTERN


def test_the_finder_class(gpu):
    """OrbFeaturesFinder.find on host and CUDA images: row-sliced views, ready for FeaturesMatcher"""
    imgs = [want_of(n)[0] for n in ("blobs-3x1-bgr", "blobs-3x1-bgr")]
    want = want_of("blobs-3x1-bgr")[2]
    f = features.OrbFeaturesFinder()
    for put in (_dev, np.array):
        feats = f.find([put(i) for i in imgs])
        for k, ft in enumerate(feats):
            assert ft.img_idx == k and ft.img_size == (256, 224) and ft.status == want.status
            assert np.array_equal(_np(ft.keypoints), want.keypoints) and np.array_equal(_np(ft.meta), want.meta) and np.array_equal(_np(ft.descriptors), want.descriptors)
    f.release()


def test_cell_0_of_the_reference_image(gpu):
    """the fixture of tests/test_orb_ref_artifact.py: cell 0 of src1.bmp (367 columns) at the F defaults on one cell"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_orb_artifact.npz"))
    img = np.ascontiguousarray(z["gray"][:, :z["gray"].shape[1] // 3] if bool(z["whole"]) else z["gray"])
    p = M.Params(grid=(1, 1), n_features=510)
    check(run_raw(img, p), M.find(img, p), "cell 0")
