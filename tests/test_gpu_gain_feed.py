"""GainCompensator::feed on the GPU (isx_gain_compensator_feed) against the NumPy model of tests/test_gain_model.py: N exactly, I bit for
bit (the GPU's exact sums give math.fsum of the terms, and both sides divide that double by N once), gains to 1e-12 relative - on warped
tiles of the config-2 geometry, on many tiles with awkward overlaps, on host and device mats, pitched and unaligned views, on every
RGB colour once, run to run, and end to end through gain_apply."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import guarded  # noqa: E402
from imagestitch_amd import synth  # noqa: E402
from test_gain_model import THREE_I, THREE_N, feed_model, terms, three_tiles_gains, three_tiles_one_pair_apart

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _check(gpu, corners, images, masks, model=None):
    comp = gpu.GainCompensator().feed(corners, images, masks)
    N, I, _, _, _, g = model if model is not None else feed_model(corners, [_np(a) for a in images], [_np(m) for m in masks])
    assert np.array_equal(comp.N, N), (comp.N, N)
    assert np.array_equal(comp.I.view(np.uint64), I.view(np.uint64)), (comp.I, I)
    np.testing.assert_allclose(comp.gains(), g, rtol=1e-12, atol=0)
    return comp


def _oracle_pair(oracle, W, H, F, seed=0):
    K, Rs = synth.camera_pair(W, H, F)
    corners, wis, wms = [], [], []
    for i in range(2):
        img = synth.make_tile(H, W, seed + i)
        c, wi, _ = oracle.warp_u8(oracle.CYL, F, K, Rs[i], img, oracle.LINEAR, oracle.BORDER_REFLECT)
        _, wm, _ = oracle.warp_u8(oracle.CYL, F, K, Rs[i], np.full((H, W), 255, np.uint8), oracle.NEAREST, oracle.BORDER_CONSTANT)
        corners.append(c); wis.append(wi); wms.append(wm)
    return corners, wis, wms


@pytest.mark.parametrize("where", ["host", "device"])
def test_config2_geometry_reduced(gpu, oracle, where):
    """The config-2 pair (2 tiles, cylindrical, yaw 0.36) at a quarter of 4K, warped by the oracle; the two tiles differ in exposure."""
    corners, wis, wms = _oracle_pair(oracle, 960, 540, 750.0)
    wis[1] = np.clip(wis[1].astype(np.int32) * 5 // 4, 0, 255).astype(np.uint8)
    model = feed_model(corners, wis, wms)
    assert model[0][0, 1] > 1000
    imgs, masks = (wis, wms) if where == "host" else ([_dev(a) for a in wis], [_dev(m) for m in wms])
    comp = _check(gpu, corners, imgs, masks, model)
    g = comp.gains()
    assert g[0] > 1.0 > g[1]


def test_config2_full_size_pair_warped_on_gpu(gpu):
    """One 4K pair (3840 x 2160, f = 3000) warped on the GPU, device-resident, against the model."""
    import torch
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    warper = gpu.CylindricalWarper().create(F)
    corners, wis, wms = [], [], []
    for i in range(2):
        c, wi, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, 10 + i)).cuda(), K, Rs[i])
        corners.append(c); wis.append(wi); wms.append(wm)
    torch.cuda.synchronize()
    _check(gpu, corners, wis, wms)


def _many_tiles(n, seed):
    """n tiles of assorted sizes with negative corners, non-adjacent overlaps, 1-pixel overlaps and masks holding 0 / 254 / 255."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(30, 90)), int(rng.integers(20, 70))) for _ in range(n)]     # (w, h)
    corners = [(int(rng.integers(-60, 60)), int(rng.integers(-40, 40))) for _ in range(n)]
    # tile n-1 touches tile 0 in exactly one pixel (its top-left on tile 0's bottom-right pixel), tile n-2 tile 0 in one column
    w0, h0 = sizes[0]
    corners[n - 1] = (corners[0][0] + w0 - 1, corners[0][1] + h0 - 1)
    corners[n - 2] = (corners[0][0] + w0 - 1, corners[0][1] - 5)
    imgs, masks = [], []
    for k, (w, h) in enumerate(sizes):
        lo = int(rng.integers(0, 80))
        imgs.append(rng.integers(lo, 256, (h, w, 3), dtype=np.uint8))
        m = rng.choice(np.array([0, 254, 255, 255, 255, 255], np.uint8), size=(h, w))
        masks.append(m)
    masks[0][-1, -1] = 255
    masks[n - 1][0, 0] = 255
    return corners, imgs, masks


@pytest.mark.parametrize("n", [5, 6, 7])
@pytest.mark.parametrize("where", ["host", "device"])
def test_many_tiles(gpu, n, where):
    corners, imgs, masks = _many_tiles(n, 100 + n)
    model = feed_model(corners, imgs, masks)
    assert model[0][0, n - 1] == 1 and model[1][0, n - 1] != 0.0     # the 1-pixel overlap counts
    if where == "device":
        imgs, masks = [_dev(a) for a in imgs], [_dev(m) for m in masks]
    _check(gpu, corners, imgs, masks, model)


@pytest.mark.parametrize("where", ["host", "device"])
def test_three_tiles_one_pair_apart_by_hand(gpu, where):
    """The hand-worked system of tests/test_gain_model.py: the pair that does not overlap has N = 0 and adds nothing to A or b."""
    corners, imgs, masks = three_tiles_one_pair_apart()
    if where == "device":
        imgs, masks = [_dev(a) for a in imgs], [_dev(m) for m in masks]
    comp = gpu.GainCompensator().feed(corners, imgs, masks)
    assert np.array_equal(comp.N, THREE_N)
    assert np.array_equal(comp.I, THREE_I)
    np.testing.assert_allclose(comp.gains(), three_tiles_gains(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("where", ["host", "device"])
def test_pitched_and_unaligned_views(gpu, where):
    """Views into larger buffers (tests/helpers/guarded.py): every tile in the "odd" layout (row pitches that are no multiple of 4,
    first pixels off a dword: offsets 1, 2 and 3 occur, the images' and the masks' differ), every tile in the "aligned" one, and the
    two mixed tile by tile, image against mask; seeded random bytes around the images and 255 around the masks (a mask read past its
    view would count) - and feed() writes none of it."""
    corners, imgs, masks = _many_tiles(6, 7)
    model = feed_model(corners, imgs, masks)
    odd, aligned = guarded.LAYOUTS
    offsets = set()
    for p, (li, lm) in enumerate(((odd, odd), (aligned, aligned), (odd, aligned), (aligned, odd))):
        mixed = p >= 2
        gi = [guarded.guarded_like(a, where, (lm if mixed and k % 2 else li), 100 * p + 10 + k) for k, a in enumerate(imgs)]
        gm = [guarded.guarded_like(m, where, (li if mixed and k % 2 else lm), 100 * p + 20 + k) for k, m in enumerate(masks)]
        for g, m in zip(gm, masks):
            g.buf[...] = 255                                            # 255 all around a mask: a read past the view would count
            g.set(m)
        _check(gpu, corners, [g.view for g in gi], [g.view for g in gm], model)
        for g in gi + gm:
            g.check(guarded.NOTHING)
            offsets.add(((g.buf.ctypes.data if where == "host" else g.buf.data_ptr()) + g.offset) % 4)
    assert offsets == {0, 1, 2, 3}


def test_every_rgb_colour_once(gpu):
    """A 4096 x 4096 image holding each of the 2^24 colours once, over a shuffled copy of itself: every r^2 + g^2 + b^2 there is, through
    the per-pixel sqrt and the exact sum."""
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    shuf = img.reshape(-1, 3)[np.random.default_rng(5).permutation(1 << 24)].reshape(4096, 4096, 3)
    mask = np.full((4096, 4096), 255, np.uint8)
    t = terms(img).ravel().tolist()
    isum = math.fsum(t)
    comp = gpu.GainCompensator().feed([(0, 0), (0, 0)], [_dev(img), _dev(shuf)], [_dev(mask), _dev(mask)])
    assert comp.N[0, 1] == 1 << 24 and comp.N[0, 0] == 1 << 24
    want = isum / (1 << 24)
    assert comp.I[0, 1] == want and comp.I[1, 0] == want, (comp.I, want)
    assert np.all(comp.gains() == comp.gains()[0])


def test_deterministic(gpu, oracle):
    corners, wis, wms = _oracle_pair(oracle, 960, 540, 750.0, seed=20)
    imgs, masks = [_dev(a) for a in wis], [_dev(m) for m in wms]
    runs = [gpu.GainCompensator().feed(corners, imgs, masks) for _ in range(20)]
    for c in runs[1:]:
        assert np.array_equal(c.N, runs[0].N)
        assert np.array_equal(c.I.view(np.uint64), runs[0].I.view(np.uint64))
        assert np.array_equal(c.gains().view(np.uint64), runs[0].gains().view(np.uint64))


def test_end_to_end_warp_feed_apply(gpu, oracle):
    """W:229-244 on the GPU: warp a pair, feed the compensator, apply its gains - byte for byte the oracle's warp times the model's gain."""
    import torch
    W, H, F = 800, 450, 620.0
    K, Rs = synth.camera_pair(W, H, F)
    srcs = [synth.make_tile(H, W, 30 + i) for i in range(2)]
    srcs[0] = (srcs[0] // 2 + 20).astype(np.uint8)
    warper = gpu.CylindricalWarper().create(F)
    corners, wis, wms = [], [], []
    for i in range(2):
        c, wi, wm = warper.warp_with_mask(torch.from_numpy(srcs[i]).cuda(), K, Rs[i])
        corners.append(c); wis.append(wi); wms.append(wm)
    comp = gpu.GainCompensator().feed(corners, wis, wms)
    o_corners, o_wis, o_wms = [], [], []
    for i in range(2):
        c, owi, _ = oracle.warp_u8(oracle.CYL, F, K, Rs[i], srcs[i], oracle.LINEAR, oracle.BORDER_REFLECT)
        _, owm, _ = oracle.warp_u8(oracle.CYL, F, K, Rs[i], np.full((H, W), 255, np.uint8), oracle.NEAREST, oracle.BORDER_CONSTANT)
        o_corners.append(c); o_wis.append(owi); o_wms.append(owm)
    assert o_corners == corners
    _, _, _, _, _, g = feed_model(o_corners, o_wis, o_wms)
    np.testing.assert_allclose(comp.gains(), g, rtol=1e-12, atol=0)
    assert g[0] > 1.0
    for i in range(2):
        comp.apply(i, corners[i], wis[i], wms[i])
        assert np.array_equal(wis[i].cpu().numpy(), oracle.gain_apply(o_wis[i], g[i])), i


def test_cpp_gain_demo(gpu, tmp_path):
    """isx::GainCompensator (include/imagestitch.hpp) and HipGainCompensator through cv::detail::ExposureCompensator
    (include/imagestitch_cv_exposure.hpp, compiled against tests/cpp/opencv_stub with -Werror=suggest-override) against the model."""
    exe = str(tmp_path / "gain_demo")
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Wsuggest-override", "-Woverloaded-virtual", "-Werror=suggest-override",
                           "-Werror=overloaded-virtual", "-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gain_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    corners, imgs, masks = _many_tiles(5, 55)
    for k in range(5):
        imgs[k].tofile(str(tmp_path / ("img%d.raw" % k)))
        masks[k].tofile(str(tmp_path / ("mask%d.raw" % k)))
    args = [exe, str(tmp_path), "5"] + ["%d %d %d %d" % (c[0], c[1], m.shape[1], m.shape[0]) for c, m in zip(corners, masks)]
    out = subprocess.check_output(" ".join(args).split(), text=True, timeout=300)
    _, _, _, _, _, g = feed_model(corners, imgs, masks)
    got = {}
    for line in out.splitlines():
        t = line.split()
        if t and t[0] in ("mirror", "adapter"):
            got[t[0]] = np.array([float.fromhex(x) for x in t[1:]])
    for leg in ("mirror", "adapter"):
        np.testing.assert_allclose(got[leg], g, rtol=1e-12, atol=0)
    assert np.array_equal(got["mirror"], got["adapter"])
    assert "apply OK" in out and "throws 7" in out


def test_mixed_residency(gpu):
    """Tiles 0 and 2 on the host, tile 1 on the device, every pair overlapping (tile 2 meets tile 0 in one pixel, tile 1 tile 0 in one
    column): N, I and the gains of the model, and feed leaves images and masks as they were."""
    corners, imgs, masks = _many_tiles(3, 103)
    model = feed_model(corners, imgs, masks)
    assert model[0][0, 1] > 1 and model[0][0, 2] == 1
    src = [_dev(a) if k == 1 else a.copy() for k, a in enumerate(imgs)]
    mk = [_dev(m) if k == 1 else m.copy() for k, m in enumerate(masks)]
    _check(gpu, corners, src, mk, model)
    for k in range(3):
        assert np.array_equal(_np(src[k]), imgs[k]) and np.array_equal(_np(mk[k]), masks[k]), k
