"""The fisheye and stereographic projectors on the GPU against the NumPy model tests/helpers/polar_np.py: every entry a handle of the two
kinds serves, bit for bit (np.array_equal, no tolerance) - detectResultRoi and warpPoint on every rig, buildMaps with the (-1, -1)
sentinel, warp over four pixel types x NEAREST / LINEAR / TIES_EVEN x every border mode, the fused image + mask warp with and without a
mask, CV_16SC3 and the gain, host / device / strided mats, windows that hold the destination origin (the pole: r = 0, atan2f(0, 0),
atanf(inf)) and windows far outside it, the ROI cache, two handles of different kinds on one stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402

from imagestitch_amd._lib import as_mat, check, f9  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]
RIGS = [(s, r) for s in P.SIZES for r in P.ROTATIONS]


def _ids(v):
    return "%dx%d" % v[:2] if isinstance(v, tuple) else str(v)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _warper(gpu, kind, scale, by_name=False):
    if by_name:
        return gpu.RotationWarper(PC.KIND_NAMES[kind], scale)
    return (gpu.FisheyeWarper if kind == P.FISHEYE else gpu.StereographicWarper)().create(scale)


def _fused_roi(warper, img, mask, K, R, roi, dimg, dmask):
    """isx_warper_warp_with_mask_roi with the caller's rectangle and mats"""
    mi, mdi, mdm = as_mat(img), as_mat(dimg), as_mat(dmask)
    mm = as_mat(mask) if mask is not None else None
    check(warper._lib.isx_warper_warp_with_mask_roi(warper._h, C.byref(mi), C.byref(mm) if mm is not None else None, f9(K)[1], f9(R)[1],
                                                    (C.c_int * 4)(*[int(v) for v in roi]), C.byref(mdi), C.byref(mdm)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size,rname", RIGS, ids=_ids)
def test_roi_and_warp_point_equal_the_model(gpu, kind, size, rname):
    w, h, f, K, R = P.rig(size, rname)
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f, by_name=(w == 64))
    mroi, mmm = m.detect_roi(w, h)
    for cache in (False, True, False):                       # the scan, the remembered answer, and the scan again behind the re-armed keys
        warper.set_roi_cache(cache)
        for _ in range(2):
            roi, mm = warper.warpRoi((w, h), K, R, with_minmax=True)
            assert roi == tuple(int(v) for v in mroi) and np.array_equal(mm, mmm), (roi, mroi, mm, mmm)
    r_kinv, k_rinv = warper.camera(K, R)
    assert np.array_equal(r_kinv, m.r_kinv) and np.array_equal(k_rinv, m.k_rinv)
    for x, y in [(0, 0), (w - 1, h - 1), (w / 2, h / 2), (-3.25, h + 7.5), (w / 2 + 0.125, 1e4)]:
        u, v = warper.warpPoint((x, y), K, R)
        mu, mv = m.map_forward(F(x), F(y))
        assert PC.same_bits(np.array([u, v], F), np.array([mu, mv], F)), (x, y, u, v, mu, mv)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rname", list(P.ROTATIONS))
def test_maps_and_every_warp_on_the_smallest_rig(gpu, oracle, kind, rname):
    import torch
    w, h, f, K, R = P.rig(P.SIZES[0], rname)
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    roi = warper.warpRoi((w, h), K, R)
    blown = PC.window_of(roi) != roi
    rng = np.random.default_rng(500 + kind)
    like = torch.empty(1, device="cuda")
    for win in ([PC.window_of(roi)] + ([PC.window_of(roi, far=True), (40000, -70000, 40063, -69990)] if blown else [])):
        xm, ym = m.build_maps(win)
        gx, gy = warper.buildMapsRoi(K, R, win)
        dx, dy = warper.buildMapsRoi(K, R, win, like=like)
        assert PC.same_bits(gx, xm) and PC.same_bits(gy, ym) and PC.same_bits(_np(dx), xm) and PC.same_bits(_np(dy), ym), win
        if not blown:
            r2, bx, by = warper.buildMaps((w, h), K, R)
            assert r2 == roi and PC.same_bits(bx, xm) and PC.same_bits(by, ym)
        shape = xm.shape
        for cn, dtype in ((3, np.uint8), (1, np.uint8), (3, np.float32), (1, np.float32)):
            src = PC.image(rng, h, w, cn, dtype)
            dev = torch.from_numpy(src).cuda()
            for interp in (PC.NEAREST, PC.LINEAR, PC.LINEAR | PC.TIES_EVEN):
                for border in (PC.CONST, PC.REPL, PC.REFLECT, PC.WRAP, PC.REFLECT101):
                    if interp & PC.TIES_EVEN or border == PC.WRAP:      # the oracle has neither: the library's own remap over the MODEL's maps
                        want = gpu.remap(src, xm, ym, interp, border)
                    else:
                        want = oracle.remap(src, xm, ym, interp, border)
                    got = warper.warp_roi(src, K, R, interp, border, win, np.empty(shape + src.shape[2:], src.dtype))
                    assert got.dtype == want.dtype and np.array_equal(got, want), (win, cn, dtype, interp, border, np.argwhere(got != want)[:4])
                    if border in (PC.CONST, PC.REFLECT):
                        gd = warper.warp_roi(dev, K, R, interp, border, win, torch.empty(shape + src.shape[2:], dtype=dev.dtype, device="cuda"))
                        assert np.array_equal(_np(gd), want), (win, cn, dtype, interp, border)
        if not blown:                                         # RotationWarper::warp itself: detectResultRoi inside the call, the corner back
            src = PC.image(rng, h, w)
            want = oracle.remap(src, xm, ym, PC.LINEAR, PC.REFLECT)
            c, got = warper.warp(src, K, R, PC.LINEAR, PC.REFLECT)
            assert c == roi[:2] and np.array_equal(got, want)
            c, got = warper.warp(torch.from_numpy(src).cuda(), K, R, PC.LINEAR, PC.REFLECT, dst=torch.empty(want.shape, dtype=torch.uint8, device="cuda"))
            assert c == roi[:2] and np.array_equal(_np(got), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size,rname", [(s, r) for s in (P.SIZES[0], P.SIZES[2]) for r in P.ROTATIONS], ids=_ids)
def test_fused_warp_with_and_without_a_mask(gpu, oracle, kind, size, rname):
    import torch
    w, h, f, K, R = P.rig(size, rname)
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    roi = warper.warpRoi((w, h), K, R)
    win = PC.window_of(roi)
    rng = np.random.default_rng(900 + w + kind)
    img = PC.image(rng, h, w)
    holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
    xm, ym = m.build_maps(win)
    wi = oracle.remap(img, xm, ym, PC.LINEAR, PC.REFLECT)
    wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST)
    wh = oracle.remap(holes, xm, ym, PC.NEAREST, PC.CONST)
    dh, dw = wm.shape
    for where in ("host", "device", "strided"):
        if where == "host":
            s, hm = img, holes
            mk = lambda shape, dt: np.zeros(shape, dt)          # noqa: E731
        elif where == "device":
            s, hm = torch.from_numpy(img).cuda(), torch.from_numpy(holes).cuda()
            mk = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")          # noqa: E731
        else:                                                   # rows that are views into wider mats, source and destinations
            wide = np.zeros((h, w + 5, 3), np.uint8)
            wide[:, 2:2 + w] = img
            wideh = np.zeros((h, w + 7), np.uint8)
            wideh[:, 3:3 + w] = holes
            s, hm = wide[:, 2:2 + w], wideh[:, 3:3 + w]
            mk = lambda shape, dt: np.zeros((shape[0], shape[1] + 3) + tuple(shape[2:]), dt)[:, 1:1 + shape[1]]          # noqa: E731
        for out16 in (False, True):
            for mask, want_mask in ((None, wm), (hm, wh)):
                di, dm = mk((dh, dw, 3), np.int16 if out16 else np.uint8), mk((dh, dw), np.uint8)
                _fused_roi(warper, s, mask, K, R, win, di, dm)
                assert np.array_equal(_np(di), wi.astype(np.int16) if out16 else wi) and np.array_equal(_np(dm), want_mask), (where, out16, mask is None)
        if win == roi:                                          # the entries that find the ROI themselves
            c, gi, gm = warper.warp_with_mask(s, K, R, mask=hm)
            assert c == roi[:2] and np.array_equal(_np(gi), wi) and np.array_equal(_np(gm), wh)
            c, gi, gm = warper.warp_with_mask(s, K, R, dst_img=mk((dh, dw, 3), np.uint8), dst_mask=mk((dh, dw), np.uint8))
            assert c == roi[:2] and np.array_equal(_np(gi), wi) and np.array_equal(_np(gm), wm)
    # the gain folded into the store: on the remapped byte, all-255 mask only
    for gain in (1.37, 0.5):
        warper.set_gain(gain)
        for out16 in (False, True):
            di, dm = np.zeros((dh, dw, 3), np.int16 if out16 else np.uint8), np.zeros((dh, dw), np.uint8)
            _fused_roi(warper, img, None, K, R, win, di, dm)
            assert np.array_equal(di, PC.gained(wi, gain).astype(di.dtype)) and np.array_equal(dm, wm), (gain, out16)
        with pytest.raises(gpu.IsxError) as e:
            _fused_roi(warper, img, holes, K, R, win, np.zeros((dh, dw, 3), np.uint8), np.zeros((dh, dw), np.uint8))
        assert e.value.code == 6
    warper.set_gain(1.0)
    di, dm = np.zeros((dh, dw, 3), np.uint8), np.zeros((dh, dw), np.uint8)
    _fused_roi(warper, img, None, K, R, win, di, dm)
    assert np.array_equal(di, wi)


@pytest.mark.parametrize("kind,rname", [(P.FISHEYE, "pitch+pi/2"), (P.FISHEYE, "pitch-pi/2"), (P.STEREOGRAPHIC, "pitch-pi/2"), (P.STEREOGRAPHIC, "pitch+pi/2")])
def test_a_window_with_the_destination_origin_on_the_pole_rigs(gpu, oracle, kind, rname):
    """(0, 0) of the destination: r = 0, atan2f(0, 0) = 0, and for the stereographic map 1.f / 0 = inf, atanf(inf) = pi / 2."""
    w, h, f, K, R = P.rig(P.SIZES[1], rname)
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    win = (-37, -20, 41, 22)
    xm, ym = m.build_maps(win)
    gx, gy = warper.buildMapsRoi(K, R, win)
    assert PC.same_bits(gx, xm) and PC.same_bits(gy, ym)
    ox, oy = m.map_backward(F(0), F(0))
    assert PC.same_bits(gx[20, 37], ox) and PC.same_bits(gy[20, 37], oy) and np.isfinite(ox)
    src = PC.image(np.random.default_rng(3), h, w)
    got = warper.warp_roi(src, K, R, PC.LINEAR, PC.REFLECT, win, np.empty(xm.shape + (3,), np.uint8))
    assert np.array_equal(got, oracle.remap(src, xm, ym, PC.LINEAR, PC.REFLECT))


@pytest.mark.parametrize("kind", KINDS)
def test_the_sentinel_behind_the_camera(gpu, oracle, kind):
    """The ROI mirrored through the destination origin looks behind the camera: z <= 0 there, the maps hold (-1, -1) (W:61)."""
    w, h, f, K, R = P.rig(P.SIZES[1], "identity")
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    roi = warper.warpRoi((w, h), K, R)
    win = (-roi[2], -roi[3], -roi[0] + 30, -roi[1])
    xm, ym = m.build_maps(win)
    behind = (xm == -1) & (ym == -1)
    assert behind.sum() > 5000 and (kind == P.FISHEYE or not behind.all())
    gx, gy = warper.buildMapsRoi(K, R, win)
    assert PC.same_bits(gx, xm) and PC.same_bits(gy, ym)
    src = PC.image(np.random.default_rng(4), h, w)
    for interp, border in ((PC.LINEAR, PC.CONST), (PC.NEAREST, PC.REFLECT)):
        got = warper.warp_roi(src, K, R, interp, border, win, np.empty(xm.shape + (3,), np.uint8))
        assert np.array_equal(got, oracle.remap(src, xm, ym, interp, border))


def test_roi_on_each_side_of_the_remap_limit(gpu):
    """ROI only: 261 x 67 stereographic pitch +pi/2 is 32 394 a side (under cv::remap's 32 767), 64 x 48 pitch +pi/3 is 50 202 wide (over it)."""
    for size, rname, span in ((P.SIZES[2], "pitch+pi/2", (32394, 32394)), (P.SIZES[1], "pitch+pi/3", (50201, 7332))):
        w, h, f, K, R = P.rig(size, rname)
        roi = _warper(gpu, P.STEREOGRAPHIC, f).warpRoi((w, h), K, R)
        assert roi == tuple(int(v) for v in P.from_rig(P.STEREOGRAPHIC, f, K, R).detect_roi(w, h)[0])
        assert (roi[2] - roi[0], roi[3] - roi[1]) == span, roi


def test_two_handles_of_different_kinds_on_one_stream(gpu, oracle):
    import torch
    st = torch.cuda.Stream()
    w, h, f, K, R = P.rig(P.SIZES[1], "yaw0.52")
    src = torch.from_numpy(PC.image(np.random.default_rng(8), h, w)).cuda()
    torch.cuda.synchronize()
    handles = [(k, _warper(gpu, k, f)) for k in KINDS] + [(None, gpu.CylindricalWarper().create(f))]
    outs = []
    with torch.cuda.stream(st):
        for rep in range(3):
            for kind, wp in handles:
                wp.set_stream(st)
                outs.append((kind, wp.warp_with_mask(src, K, R)))
    st.synchronize()
    for kind, (c, gi, gm) in outs:
        if kind is None:
            oc, owi, _ = oracle.warp_u8(oracle.CYL, float(f), K, R, src.cpu().numpy(), oracle.LINEAR, oracle.BORDER_REFLECT)
            assert c == oc and np.array_equal(gi.cpu().numpy(), owi)
            continue
        m = P.from_rig(kind, f, K, R)
        roi, _ = m.detect_roi(w, h)
        xm, ym = m.build_maps(roi)
        assert c == (int(roi[0]), int(roi[1])) and np.array_equal(gi.cpu().numpy(), oracle.remap(src.cpu().numpy(), xm, ym, PC.LINEAR, PC.REFLECT))
        assert np.array_equal(gm.cpu().numpy(), oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST))


def test_the_stitchers_refuse_the_kinds_cleanly(gpu):
    """PairStitcher / SplitStitcher plan their warps: the library's UNSUPPORTED error, raised before anything is built."""
    from imagestitch_amd import pipeline, synth
    W, H, Fo = 320, 200, 250.0
    K, Rs = synth.camera_pair(W, H, Fo)
    imgs = [synth.make_tile(H, W, i) for i in range(2)]
    for name in ("fisheye", "stereographic"):
        for cls in (pipeline.PairStitcher, pipeline.SplitStitcher):
            with pytest.raises(gpu.IsxError) as e:
                cls(imgs, K, Rs, Fo, kind=name)
            assert e.value.code == 6 and name in str(e.value)
