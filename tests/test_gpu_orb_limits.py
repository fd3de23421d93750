"""isx_orb_find where tests/test_gpu_orb.py never goes (DESIGN.md §8 "Features finder", "What the limit tests pin"): more than one pass of
k_orb_final_cut's 1024 candidates with and without ties, keypoints in layers past k_orb_describe's first stride of 256 and launches of 1024
layers, sides of 1, 62, 63 and ISX_ORB_MAX_SIDE, the refusals one step past each limit, and every mat with a caller-given step at a pitch
of 2^24 + 64 bytes and across spans of 2^31 and 2^32 bytes (tests/helpers/guarded_wide.py).  Every served case equals
tests/helpers/orb_np.py through test_gpu_orb.check: count, status, keypoints, descriptors, the bits of meta, the sentinel from count on."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
import test_gpu_orb as T  # noqa: E402  (run_raw, check, params_of)
from helpers import guarded  # noqa: E402
from helpers import guarded_wide as W  # noqa: E402
from helpers import orb_np as M  # noqa: E402
from imagestitch_amd import _lib, features  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED = 1, 6
P23, P24 = 1 << 23, 1 << 24
HOST_CASES = ["passes-2", "passes-ties-cut", "layers-264"] + cases.SIDE_CASES


@pytest.fixture(scope="module", autouse=True)
def release_the_large_buffers():
    yield
    import torch
    features.OrbFeaturesFinder.release()
    torch.cuda.empty_cache()


# ---- 1. the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.LIMIT_CASES))
def test_device_mats_match_the_model(gpu, name):
    img, p, want, _, _ = cases.limit_want(name)
    T.check(T.run_raw(img, p), want, name)


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_mats_match_the_model(gpu, name):
    img, p, want, _, _ = cases.limit_want(name)
    T.check(T.run_raw(img, p, device=False), want, name + " (host)")


# ---- 2. one step past each limit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
def test_refusals_at_the_edges_write_nothing(gpu, where):
    import torch
    strip = dict(nlevels=8, scale_factor=1.05, fast_threshold=5)
    one = dict(grid=(1, 1), nlevels=1)
    # (image h x w, Params keywords, the code, a word of the message); each has a served neighbour among the cases above
    edges = [((1, 16385), one, ERR_UNSUPPORTED, "16384"), ((16385, 1), one, ERR_UNSUPPORTED, "16384"),
             ((70, 129 * 70), dict(grid=(129, 1), n_features=129 * 40, **strip), ERR_UNSUPPORTED, "1024 layers"),
             ((200, 200), dict(n_features=1921, **one), ERR_UNSUPPORTED, "4096"),
             ((5, 3), dict(grid=(5, 3), nlevels=4, n_features=10), ERR_INVALID, "grid"), ((70, 128), dict(grid=(129, 1), nlevels=1), ERR_INVALID, "grid")]
    cap = features.capacity(features.default_params())
    outs = [guarded.guarded((cap, 2), np.float32, where, "aligned", 40, "keypoints"), guarded.guarded((cap, 4), np.float32, where, "aligned", 41, "meta"),
            guarded.guarded((cap, 32), np.uint8, where, "odd", 42, "descriptors"), guarded.guarded((1, 2), np.int32, where, "aligned", 43, "count_status")]
    for k, (shape, kw, code, word) in enumerate(edges):
        g_img = guarded.guarded_like(cases.noise(shape[0], shape[1], 50 + k), where, "odd", 44 + k, "image")
        with pytest.raises(_lib.IsxError) as e:
            features.orb_find(g_img.view, T.params_of(M.Params(**kw)), *[g.view for g in outs])
        assert e.value.code == code and word in e.value.msg, (shape, kw, e.value)
        del e
        torch.cuda.synchronize()
        g_img.check(written=guarded.NOTHING)
        for g in outs:
            g.check(written=guarded.NOTHING)


# ---- 3. addressing: one large operand a call ---------------------------------------------------------------------------------------------
def big(shape, dtype, spec, seed, name, content=None):
    """tests/test_gpu_addressing_limits.big without its 8-24 rows for a wide layout (a keypoint needs 63): spec = (layout, pitch or None), None
    for an ordinary guarded mat.  A tall layout skips only when the device has less free memory than the mat needs plus 2 GiB."""
    if spec is None:
        g = guarded.guarded(shape, dtype, "device", "odd" if seed % 2 else "aligned", seed, name)
    else:
        import torch
        layout, pitch = spec
        if layout.startswith("tall"):
            need = W.bytes_needed(shape, dtype, layout, pitch)
            if torch.cuda.mem_get_info()[0] < need + (2 << 30):
                torch.cuda.empty_cache()
            free = torch.cuda.mem_get_info()[0]
            if free < need + (2 << 30):
                pytest.skip("%s of %d rows needs %.1f GiB + 2 GiB, the device has %.1f GiB free" % (layout, shape[0], need / 2.0**30, free / 2.0**30))
        g = W.wide_guarded(shape, dtype, layout, seed, name, pitch)
        m = _lib.as_mat(g.view)
        assert m.step == g.pitch and m.rows == shape[0] and m.data == g.view.data_ptr()
    return g.set(content) if content is not None else g


def rows_mask(cap, n, width):
    rows = np.zeros((cap, width), bool)
    rows[:n] = True
    return rows


def boundaries(pitch, rows, row_bytes):
    """the rows at which the byte offset from the mat's first byte passes 2^31 and 2^32: (k, the first row that starts at or past 2^k)"""
    out = [(k, -(-(1 << k) // pitch)) for k in (31, 32) if (rows - 1) * pitch + row_bytes > 1 << k]
    assert all((b - 1) * pitch + row_bytes <= 1 << k <= b * pitch for k, b in out)      # no row straddles: a row lies on one side
    return out


def find_on(g_img, p, outs):
    """isx_orb_find on guarded mats (outs: keypoints, meta, descriptors, count_status): the whole mats, as run_raw gives them"""
    import torch
    features.orb_find(g_img.view, T.params_of(p), *[g.view for g in outs])
    torch.cuda.synchronize()
    return tuple(g.get() for g in outs)


def outputs(cap, seed, large=None, spec=None):
    shapes = (("keypoints", (cap, 2), np.float32), ("meta", (cap, 4), np.float32), ("descriptors", (cap, 32), np.uint8), ("count_status", (1, 2), np.int32))
    outs = [big(shape, dt, spec if name == large else None, seed + k, name) for k, (name, shape, dt) in enumerate(shapes)]
    for g in outs[:3]:
        g.set(np.full(g.shape, T.SENTINEL, g.dtype))
    return outs


def check_written(outs, cap, n):
    for g, width in zip(outs[:3], (2, 4, 32)):
        g.check(written=rows_mask(cap, n, width))
    outs[3].check()


# the image: 96 columns (keypoints in columns 31 - 64), rows enough for a keypoint whose patch lies on both sides of each boundary
IMAGES = {"pitch_2p24_64": (("wide", P24 + 64), 70), "tall31": (("tall31", P23), 300), "tall32": (("tall32", P23), 560), "tall32_below_2p24": (("tall32", P24 - 64), 300)}
IMAGE_PARAMS = dict(grid=(1, 1), nlevels=2, scale_factor=1.2, n_features=500, fast_threshold=20)
_image_want = {}


def image_want(rows, cn):
    if (rows, cn) not in _image_want:
        rng = np.random.default_rng(700 + rows + cn)
        img = rng.integers(0, 256, (rows, 96) if cn == 1 else (rows, 96, cn), dtype=np.uint8)
        _image_want[(rows, cn)] = (img, M.find(img, M.Params(**IMAGE_PARAMS)))
    return _image_want[(rows, cn)]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("layout", sorted(IMAGES))
def test_the_image_at_the_addressing_limits(gpu, layout, cn):
    spec, rows = IMAGES[layout]
    img, want = image_want(rows, cn)
    p = M.Params(**IMAGE_PARAMS)
    plan = W.plan(img.shape, np.uint8, *spec)
    y0 = want.keypoints[want.meta[:, 3] == 0, 1]
    assert plan.pitch == spec[1] and want.count > 20 and y0.min() < 40 and y0.max() > rows - 40
    bounds = boundaries(plan.pitch, rows, plan.row_bytes)
    assert [k for k, _ in bounds] == {"pitch_2p24_64": [], "tall31": [31], "tall32": [31, 32], "tall32_below_2p24": [31, 32]}[layout]
    for k, b in bounds:         # a level-0 keypoint whose 31 x 31 patch reads rows b - 1 and b
        assert ((y0 >= b - 15) & (y0 <= b + 14)).any(), (layout, k, b)
    cap = M.capacity(p)
    g_img = big(img.shape, np.uint8, spec, 60 + cn, "image", img)
    outs = outputs(cap, 70)
    T.check(find_on(g_img, p, outs), want, "%s x %d" % (layout, cn))
    check_written(outs, cap, want.count)
    g_img.check(written=guarded.NOTHING)


OUT_PARAMS = dict(grid=(1, 1), nlevels=1, n_features=600, fast_threshold=20)
OUTPUTS = {"tall31": ("tall31", P23), "tall32_below_2p24": ("tall32", P24 - 64)}


@pytest.mark.parametrize("layout", sorted(OUTPUTS))
@pytest.mark.parametrize("operand", ["keypoints", "meta", "descriptors"])
def test_an_output_at_the_addressing_limits(gpu, operand, layout):
    """600 rows of noise 200 x 200: at a pitch of 2^23 the rows pass 2^31 at row 256 and 2^32 at row 512, at 2^24 - 64 at rows 129 and 257
    (and 8 GiB at row 513)"""
    spec = OUTPUTS[layout]
    if "out" not in _image_want:
        img = cases.noise(200, 200, 106)
        _image_want["out"] = (img, M.find(img, M.Params(**OUT_PARAMS)))
    img, want = _image_want["out"]
    p = M.Params(**OUT_PARAMS)
    cap = M.capacity(p)
    assert want.count == 600 and cap == 632
    width, dt = {"keypoints": (2, np.float32), "meta": (4, np.float32), "descriptors": (32, np.uint8)}[operand]
    plan = W.plan((cap, width), dt, *spec)
    bounds = boundaries(plan.pitch, want.count, plan.row_bytes)                # rows the count names, not the capacity's
    assert [k for k, _ in bounds] == [31, 32] and all(b + 1 < want.count for _, b in bounds), bounds
    g_img = big(img.shape, np.uint8, None, 80, "image", img)
    outs = outputs(cap, 81, operand, spec)
    T.check(find_on(g_img, p, outs), want, "%s on %s" % (operand, layout))
    check_written(outs, cap, want.count)
    g_img.check(written=guarded.NOTHING)
