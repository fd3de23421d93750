#!/usr/bin/env python3
"""Randomised parity sweep: HIP path vs the CPU oracle on random geometries (run on the GPU box).
    python tools/fuzz_parity.py [seconds] [seed] [summary.json]
Every failure prints the seed of the case so that it can be replayed; exit code = number of failing cases.  With a third argument the
summary (cases, seconds, seed, mismatches per family) is also written as JSON - the file kept under profiles/.
tests/test_gpu_fuzz_slice.py runs run(20 s, fixed seed) under -m gpu.
28 families (CASES); ISX_FUZZ_ONLY=case_a,case_b runs only those; ISX_FUZZ_STOP_AT_FIRST=1 ends the run at the first failing case.
The 26th, case_resize: cv::resize and the scaled mask stage (isx_resize, isx_mask_dilate_resize_and) against tests/helpers/resize_np.py
over the shape classes RESIZE_CLASSES.  The 27th, case_graphcut_grad: GraphCutSeamFinder(COST_COLOR_GRAD) against
tests/helpers/graphcut_grad_np.py over GRAPHCUT_GRAD_CLASSES, the structured patterns of tools/graphcut_patterns.py among them.  The 28th,
case_plan_verify: the planned warp's ROI verification (isx_warper_queue_verify, isx_warper_verify, isx_warper_plan_status) against the
three-valued model tests/helpers/plan_verify_np.py over PLAN_VERIFY_CLASSES, with the true plan or one bound of it moved."""
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import imagestitch_amd as G  # noqa: E402
from oracle import capi as O  # noqa: E402


def rot(rng, amp):
    a, b, c = rng.uniform(-amp, amp, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return (Ry @ Rx @ Rz).astype(np.float32)


def case_warp(rng):
    w, h = int(rng.integers(2, 400)), int(rng.integers(2, 300))
    f = float(rng.uniform(0.3, 3.0) * max(w, h))
    K = np.array([[f, 0, w / 2 + rng.uniform(-3, 3)], [0, f * rng.uniform(0.9, 1.1), h / 2 + rng.uniform(-3, 3)], [0, 0, 1]], np.float32)
    R = rot(rng, 0.5)
    kind = int(rng.integers(0, 2))
    cn = int(rng.choice([1, 3]))
    src = rng.integers(0, 256, (h, w, 3) if cn == 3 else (h, w)).astype(np.uint8)
    interp, border = int(rng.integers(0, 2)), int(rng.choice([0, 1, 2, 4]))
    roi, _ = O.detect_roi(kind, f, K, R, w, h)
    if (roi[2] - roi[0] + 1) * (roi[3] - roi[1] + 1) > 4_000_000 or roi[2] < roi[0] or roi[3] < roi[1]:
        return "skip"
    wp = (G.CylindricalWarper() if kind == 0 else G.SphericalWarper()).create(f)
    c, d = wp.warp(src, K, R, interp, border)
    oc, od, _ = O.warp_u8(kind, f, K, R, src, interp, border)
    assert tuple(c) == tuple(oc), (c, oc)
    assert np.array_equal(d, od), np.argwhere(d != od)[:3]
    if cn == 3:
        c2, wi, wm = wp.warp_with_mask(src, K, R)
        _, oi, _ = O.warp_u8(kind, f, K, R, src, 1, 2)
        _, om, _ = O.warp_u8(kind, f, K, R, np.full((h, w), 255, np.uint8), 0, 0)
        assert np.array_equal(wi, oi) and np.array_equal(wm, om)


def case_blend(rng):
    n = int(rng.integers(1, 5))
    sizes = [(int(rng.integers(1, 180)), int(rng.integers(1, 150))) for _ in range(n)]
    corners = [(int(rng.integers(-60, 120)), int(rng.integers(-40, 90))) for _ in range(n)]
    bands, prec = int(rng.integers(0, 7)), int(rng.integers(0, 3))
    tiles = [(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) > rng.uniform(0, 0.6)).astype(np.uint8) * 255) for (w, h) in sizes]
    deferred = bool(rng.integers(0, 2))
    u8 = bool(rng.integers(0, 2))
    mb = G.MultiBandBlender(False, bands, prec)
    mb.set_deferred_level0(deferred)
    ob = O.MultiBand(bands, prec)
    mb.prepare(corners, sizes)
    ob.prepare(corners, sizes)
    for (img, mask), c in zip(tiles, corners):
        if u8:
            mb.feed_u8(img, mask, c)
        else:
            mb.feed(img.astype(np.int16), mask, c)
        ob.feed(img.astype(np.int16), mask, c)
    of32 = prec != 0 and bool(rng.integers(0, 2))
    d, m = mb.blend(out_f32=of32)
    od, om = ob.blend(of32)
    assert np.array_equal(m, om)
    assert np.array_equal(d, od), (bands, prec, deferred, np.argwhere(d != od)[:3])


def case_feather(rng):
    n = int(rng.integers(1, 4))
    sizes = [(int(rng.integers(1, 200)), int(rng.integers(1, 160))) for _ in range(n)]
    corners = [(int(rng.integers(-60, 120)), int(rng.integers(-40, 90))) for _ in range(n)]
    sharp = float(rng.choice([0.02, 0.1, 0.5, 1.7]))
    fb, ob = G.FeatherBlender(False, sharp), O.Feather(sharp)
    fb.set_deferred_level0(bool(rng.integers(0, 2)))
    fb.prepare(corners, sizes)
    ob.prepare(corners, sizes)
    keep = []
    for (w, h), c in zip(sizes, corners):
        img = rng.integers(-300, 600, (h, w, 3)).astype(np.int16)
        mask = np.full((h, w), 255, np.uint8)
        mask[rng.random((h, w)) < rng.choice([0.0, 0.002, 0.3])] = 0
        keep.append((img, mask))
        fb.feed(img, mask, c)
        ob.feed(img, mask, c)
    d, m = fb.blend()
    od, om = ob.blend()
    assert np.array_equal(m, om) and np.array_equal(d, od)


def case_prep(rng):
    h, w = int(rng.integers(1, 300)), int(rng.integers(1, 400))
    kw, kh = int(rng.integers(1, 45)), int(rng.integers(1, 45))
    m = (rng.random((h, w)) < rng.choice([0.001, 0.05, 0.5])).astype(np.uint8) * int(rng.integers(1, 256))
    other = rng.integers(0, 256, (h, w)).astype(np.uint8)
    assert np.array_equal(G.dilate_and(m, kw, kh, other=other), O.dilate_rect(m, kw, kh) & other)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    g = float(rng.choice([rng.uniform(0.2, 3.0), 1.0, 0.5, 2.0]))
    assert np.array_equal(G.gain_apply(img.copy(), g), O.gain_apply(img, g))


def case_seam(rng):
    from seam_cases import make_case
    try:
        c = _seam_case(rng, make_case)
    except AssertionError:
        return "skip"          # the generator rejects tiles that barely overlap
    ref, rh = O.seam_estimate(c["img1"], c["img2"], c["tl1"], c["tl2"], c["union_tl"], c["labels"], c["label"], c["roi"], c["p1"], c["p2"])
    got, gh = G.seam_estimate(c["img1"], c["img2"], c["tl1"], c["tl2"], c["union_tl"], c["labels"], c["label"], c["roi"], c["p1"], c["p2"])
    assert gh == rh and np.array_equal(got, ref)


def _seam_case(rng, make_case):
    return make_case(int(rng.integers(0, 1 << 30)), size1=(int(rng.integers(30, 200)), int(rng.integers(40, 260))), size2=(int(rng.integers(30, 200)), int(rng.integers(40, 260))),
                  tl1=(int(rng.integers(-40, 0)), int(rng.integers(-10, 10))), tl2=(int(rng.integers(0, 30)), int(rng.integers(-10, 10))), u8=bool(rng.integers(0, 2)),
                  horizontal=bool(rng.integers(0, 2)), swap=bool(rng.integers(0, 2)), holes=bool(rng.integers(0, 2)))


def case_blend_float_and_many(rng):
    """CV_32FC3 feeds in the float precisions, CV_8UC3 / CV_32FC3 outputs, up to 11 tiles (beyond one Cover / one TileSet)."""
    n = int(rng.integers(1, 12))
    sizes = [(int(rng.integers(2, 90)), int(rng.integers(2, 80))) for _ in range(n)]
    corners = [(int(rng.integers(-30, 200)), int(rng.integers(-30, 120))) for _ in range(n)]
    bands, prec = int(rng.integers(0, 6)), int(rng.integers(1, 3))
    mb = G.MultiBandBlender(False, bands, prec)
    mb.set_deferred_level0(bool(rng.integers(0, 2)))
    ob = O.MultiBand(bands, prec)
    mb.prepare(corners, sizes)
    ob.prepare(corners, sizes)
    for (w, h), c in zip(sizes, corners):
        img = (rng.random((h, w, 3)) * 300 - 20).astype(np.float32)
        mask = (rng.random((h, w)) > 0.2).astype(np.uint8) * 255
        mb.feed(img, mask, c)
        ob.feed(img, mask, c)
    d, m = mb.blend(out_f32=True)
    od, om = ob.blend(True)
    assert np.array_equal(m, om) and np.array_equal(d, od), (n, bands, prec, np.argwhere(d != od)[:3])


def case_pipeline(rng):
    """PairStitcher: planned step (ROI verified on the device, scans scheduled inside blend) == host-synchronous step == oracle."""
    import torch
    from imagestitch_amd import synth
    from imagestitch_amd.pipeline import PairStitcher
    W, H = int(rng.integers(200, 900)), int(rng.integers(150, 600))
    F = float(rng.uniform(0.6, 1.5) * W)
    K, Rs = synth.camera_pair(W, H, F, yaw=float(rng.uniform(0.1, 0.35)))
    imgs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    bands, prec = int(rng.integers(1, 6)), int(rng.integers(0, 3))
    t = [torch.from_numpy(a).cuda() for a in imgs]
    ps = PairStitcher(t, K, Rs, F, "cylindrical", bands, prec, 0, None, "int16", verify_at=int(rng.integers(-1, 4)))
    a, am = [x.clone() for x in ps.step()]
    a2, am2 = [x.clone() for x in ps.step()]
    b, bm = ps.step_sync()
    assert ps.check_plan() == 0
    assert torch.equal(a, b) and torch.equal(am, bm) and torch.equal(a2, b)
    corners, warped, seam = [], [], [s.cpu().numpy() for s in ps.seam]
    for i in range(2):
        c, wi, _ = O.warp_u8(O.CYL, F, K, Rs[i], imgs[i], 1, 2)
        corners.append(c); warped.append(wi)
    ob = O.MultiBand(bands, prec)
    ob.prepare(corners, [(w.shape[1], w.shape[0]) for w in warped])
    for i in range(2):
        ob.feed(warped[i].astype(np.int16), seam[i], corners[i])
    od, om = ob.blend(False)
    assert np.array_equal(b.cpu().numpy(), od) and np.array_equal(bm.cpu().numpy(), om)


def case_find(rng):
    """The whole DP seam finder: isx_dp_seam_find vs oracle/dpseam_np.py on 2-4 tiles with barrel-shaped, holed masks."""
    from oracle.dpseam_np import DpSeamFinder as OracleFinder
    from seam_cases import make_find_case
    n, u8 = int(rng.integers(2, 5)), bool(rng.integers(0, 2))
    images, corners, masks = make_find_case(int(rng.integers(0, 1 << 30)), n, u8, holes=bool(rng.integers(0, 2)),
                                            size=(int(rng.integers(20, 160)), int(rng.integers(30, 200))))
    ref = [m.copy() for m in masks]
    OracleFinder().find(images, corners, ref)
    got = [m.copy() for m in masks]
    G.DpSeamFinder().find(images, corners, got)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b), np.argwhere(a != b)[:3]


def case_warp_fused(rng):
    """The hot fused tile kernel (image LINEAR / REFLECT + mask NEAREST / CONSTANT of an all-255 mask, W:229 + W:232) on device
    tensors: dense and pitched destinations (per-pixel / dword stores), CV_8UC3 and CV_16SC3 outputs, cameras that look past the
    image (reflected taps on every side) and far past it (z <= 0 columns), both projectors."""
    import torch
    w, h = int(rng.integers(2, 700)), int(rng.integers(2, 500))
    f = float(rng.uniform(0.25, 3.0) * max(w, h))
    K = np.array([[f, 0, w / 2 + rng.uniform(-5, 5)], [0, f * rng.uniform(0.9, 1.1), h / 2 + rng.uniform(-5, 5)], [0, 0, 1]], np.float32)
    R = rot(rng, float(rng.choice([0.2, 0.6, 1.2])))
    kind = int(rng.integers(0, 2))
    src = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    roi, _ = O.detect_roi(kind, f, K, R, w, h)
    dw, dh = int(roi[2]) - int(roi[0]) + 1, int(roi[3]) - int(roi[1]) + 1
    if dw < 1 or dh < 1 or dw > 60000 or dh > 60000 or dw * dh > 4_000_000:
        return "skip"
    out16, pitched = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    wp = (G.CylindricalWarper() if kind == 0 else G.SphericalWarper()).create(f)
    t = torch.from_numpy(src).cuda()
    if pitched:
        es = 2 if out16 else 1
        pit = (dw * 3 * es + 63) // 64 * 64
        di = torch.zeros((dh * pit // es,), dtype=torch.int16 if out16 else torch.uint8, device="cuda").as_strided((dh, dw, 3), (pit // es, 3, 1))
        pm = (dw + 63) // 64 * 64
        dm = torch.zeros((dh * pm,), dtype=torch.uint8, device="cuda").as_strided((dh, dw), (pm, 1))
        c, wi, wm = wp.warp_with_mask(t, K, R, dst_img=di, dst_mask=dm)
    else:
        c, wi, wm = wp.warp_with_mask(t, K, R, out16=out16)
    oc, oi, _ = O.warp_u8(kind, f, K, R, src, 1, 2)
    _, om, _ = O.warp_u8(kind, f, K, R, np.full((h, w), 255, np.uint8), 0, 0)
    assert tuple(c) == tuple(oc)
    assert np.array_equal(wi.cpu().numpy(), oi.astype(np.int16) if out16 else oi), np.argwhere(wi.cpu().numpy() != oi)[:3]
    assert np.array_equal(wm.cpu().numpy(), om)


def case_linear_pair(rng):
    """A13, the reference's in-tree linear-ramp pair blend (B:141-717): random sizes (up to several LDS seam windows wide), offsets
    of either sign, dark regions so that every overlap class occurs."""
    import ctypes as C
    from imagestitch_amd import _lib
    big = rng.random() < 0.15
    h1, w1 = int(rng.integers(20, 900 if big else 200)), int(rng.integers(40, 1400 if big else 260))
    h2, w2 = h1 + int(rng.integers(-6, 7)), int(rng.integers(40, 1400 if big else 260))
    if h2 < 8:
        return "skip"
    img1 = rng.random((h1, w1, 3)).astype(np.float32) * 255
    img2 = rng.random((h2, w2, 3)).astype(np.float32) * 255
    for im in (img1, img2):                       # dark patches: the 1/0, 0/1 and 1/1 overlap classes (B:332-470)
        for _ in range(int(rng.integers(0, 4))):
            y, x = int(rng.integers(0, im.shape[0])), int(rng.integers(0, im.shape[1]))
            im[y:y + int(rng.integers(2, 40)), x:x + int(rng.integers(2, 60))] = float(rng.uniform(0, 8))
    ov = int(rng.integers(8, max(9, min(w1, w2) - 4)))
    tl1 = (int(rng.integers(-50, 50)), int(rng.integers(-50, 50)))
    tl2 = (tl1[0] + w1 - ov, tl1[1] + int(rng.integers(-6, 7)))
    rc, opano, oseam = O.blend_pair_linear(img1, img2, tl1, tl2)
    lib = _lib.load()
    pr, pc = C.c_int(), C.c_int()
    _lib.check(lib.isx_blend_pair_linear_size(h1, w1, h2, w2, tl1[0], tl1[1], tl2[0], tl2[1], C.byref(pr), C.byref(pc)))
    assert (pr.value, pc.value) == opano.shape[:2]
    pano = np.empty_like(opano)
    seam = np.zeros(opano.shape[0], np.int32)
    m1, m2, mp = _lib.as_mat(img1), _lib.as_mat(img2), _lib.as_mat(pano)
    grc = lib.isx_blend_pair_linear(C.byref(m1), C.byref(m2), tl1[0], tl1[1], tl2[0], tl2[1], C.byref(mp), seam.ctypes.data_as(_lib._IP), 0, None)
    assert (grc == 0) == (rc == 0), (grc, rc)
    if rc != 0:
        return "skip"                            # no overlap: both sides return without a panorama (B:182-183)
    assert np.array_equal(seam, oseam)
    assert np.array_equal(pano, opano, equal_nan=True), np.argwhere(pano != opano)[:5]


def case_strip(rng):
    """One column strip of a row of tiles (isx_blender_set_window) against the ORACLE's whole blend: random tiles, bands, precision,
    input type and window; only the tiles mosaic.tiles_for_window lists are fed to the HIP blender."""
    from imagestitch_amd import mosaic
    n = int(rng.integers(1, 7))
    sizes = [(int(rng.integers(40, 260)), int(rng.integers(8, 90))) for _ in range(n)]
    x, corners = int(rng.integers(-50, 50)), []
    for w, _ in sizes:
        corners.append((x, int(rng.integers(-12, 12))))
        x += int(rng.integers(max(w // 4, 1), w + 20))
    bands, prec = int(rng.integers(1, 6)), int(rng.integers(0, 3))
    as_f32 = prec != 0 and bool(rng.integers(0, 2))
    imgs, masks = [], []
    for w, h in sizes:
        imgs.append((rng.random((h, w, 3)) * 300 - 20).astype(np.float32) if as_f32 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        m = (rng.random((h, w)) > 0.15).astype(np.uint8) * 255
        masks.append(m)
    ob = O.MultiBand(bands, prec)
    ob.prepare(corners, sizes)
    for im, m, c in zip(imgs, masks, corners):
        ob.feed(im if as_f32 else im.astype(np.int16), m, c)
    out_f32 = prec != 0 and bool(rng.integers(0, 2))
    od, om = ob.blend(out_f32)
    fw = od.shape[1]
    x0 = int(rng.integers(0, (fw - 1) // 128 + 1)) * 128
    x1 = x0 + int(rng.integers(1, 4)) * 128 if rng.integers(0, 2) else x0 + int(rng.integers(1, 400))
    act = mosaic.tiles_for_window(corners, sizes, bands, x0, x1)
    mb = G.MultiBandBlender(False, bands, prec)
    mb.set_deferred_level0(True)
    mb.set_window(x0, x1)
    mb.prepare(corners, sizes)
    if not act:
        return "skip"
    as_u8 = bool(rng.integers(0, 2))      # one input type per cycle: a tile of another type ends the deferred cycle, and with it the window
    for i in act:
        if as_f32:
            mb.feed(imgs[i], masks[i], corners[i])
        elif as_u8:
            mb.feed_u8(imgs[i], masks[i], corners[i])
        else:
            mb.feed(imgs[i].astype(np.int16), masks[i], corners[i])
    d, m = mb.blend(out_f32=out_f32)
    xe = min(x1, fw)
    assert d.shape[1] == x1 - x0
    assert np.array_equal(m[:, :xe - x0], om[:, x0:xe]) and np.array_equal(d[:, :xe - x0], od[:, x0:xe]), (n, bands, prec, x0, x1, act)


def case_batch(rng):
    """isx_blender_blend_batch: 2-7 blenders of one rig family (same bands / precision / input type, different tiles, sizes and corners;
    now and then one that cannot share the chain: eager, windowed, or other bands) blended in ONE call - every result against the ORACLE's."""
    from imagestitch_amd.blender import blend_batch
    nb = int(rng.integers(2, 8))
    bands, prec = int(rng.integers(1, 6)), int(rng.integers(0, 3))
    as_u8 = bool(rng.integers(0, 2))
    out_f32 = prec != 0 and bool(rng.integers(0, 2))
    blenders, expect, dsts, dmasks = [], [], [], []
    for b in range(nb):
        odd = int(rng.integers(0, 8)) == 0                     # a blender that does not qualify for the shared chain
        n = int(rng.integers(1, 4))
        sizes = [(int(rng.integers(40, 220)), int(rng.integers(8, 90))) for _ in range(n)]
        x, corners = int(rng.integers(-50, 50)), []
        for w, _ in sizes:
            corners.append((x, int(rng.integers(-12, 12))))
            x += int(rng.integers(max(w // 4, 1), w + 20))
        bb = bands if not (odd and rng.integers(0, 2)) else int(rng.integers(1, 6))
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
        masks = [(rng.random((h, w)) > 0.15).astype(np.uint8) * 255 for w, h in sizes]
        ob = O.MultiBand(bb, prec)
        ob.prepare(corners, sizes)
        for im, m, c in zip(imgs, masks, corners):
            ob.feed(im.astype(np.int16), m, c)
        expect.append(ob.blend(out_f32))
        mb = G.MultiBandBlender(False, bb, prec)
        mb.set_deferred_level0(not (odd and bb == bands))      # the odd one with the family's bands runs the eager cycle
        mb.prepare(corners, sizes)
        for im, m, c in zip(imgs, masks, corners):
            if as_u8:
                mb.feed_u8(im, m, c)
            else:
                mb.feed(im.astype(np.int16), m, c)
        blenders.append(mb)
        w, h = mb.result_size()
        dsts.append(np.full((h, w, 3), -5, np.float32 if out_f32 else np.int16))
        dmasks.append(np.full((h, w), 7, np.uint8))
    blend_batch(blenders, dsts, dmasks)
    for b in range(nb):
        assert np.array_equal(dmasks[b], expect[b][1]) and np.array_equal(dsts[b], expect[b][0]), (nb, b, bands, prec, as_u8, out_f32)


def case_strip_feather(rng):
    """One column strip of a FeatherBlender mosaic against the oracle's whole blend; only the tiles that overlap the strip are fed."""
    n = int(rng.integers(1, 7))
    sizes = [(int(rng.integers(30, 260)), int(rng.integers(8, 90))) for _ in range(n)]
    x, corners = int(rng.integers(-50, 50)), []
    for w, _ in sizes:
        corners.append((x, int(rng.integers(-12, 12))))
        x += int(rng.integers(max(w // 4, 1), w + 20))
    sharp = float(rng.choice([0.02, 0.1, 0.5]))
    u8 = bool(rng.integers(0, 2))
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if u8 else rng.integers(-300, 600, (h, w, 3)).astype(np.int16) for w, h in sizes]
    masks = []
    for w, h in sizes:
        m = np.full((h, w), 255, np.uint8)
        m[rng.random((h, w)) < rng.choice([0.0, 0.002, 0.3])] = 0
        masks.append(m)
    ob = O.Feather(sharp)
    ob.prepare(corners, sizes)
    for im, m, c in zip(imgs, masks, corners):
        ob.feed(im.astype(np.int16), m, c)
    od, om = ob.blend()
    fw = od.shape[1]
    x0 = int(rng.integers(0, (fw - 1) // 128 + 1)) * 128
    x1 = x0 + int(rng.integers(1, 400))
    rx = min(c[0] for c in corners)
    act = [i for i in range(n) if corners[i][0] - rx < x1 and corners[i][0] - rx + sizes[i][0] > x0]
    if not act:
        return "skip"
    fb = G.FeatherBlender(False, sharp)
    fb.set_deferred_level0(True)
    fb.set_window(x0, x1)
    fb.prepare(corners, sizes)
    for i in act:
        (fb.feed_u8 if u8 else fb.feed)(imgs[i], masks[i], corners[i])
    d, m = fb.blend()
    xe = min(x1, fw)
    assert d.shape[1] == x1 - x0
    assert np.array_equal(m[:, :xe - x0], om[:, x0:xe]) and np.array_equal(d[:, :xe - x0], od[:, x0:xe]), (n, x0, x1, act)


def case_s16_tiles(rng):
    """Round 4: CV_16SC3 tiles of the whole int16 range through the deferred cycle (k_pyr_down0 / k_collapse_roll take them), device mats at
    odd alignments, masks that are not just 0 / 255, two to five tiles over one place, every precision and result type."""
    import torch
    n = int(rng.integers(1, 6))
    big = bool(rng.integers(0, 2))
    sizes = [(int(rng.integers(2, 420 if big else 120)), int(rng.integers(2, 300 if big else 100))) for _ in range(n)]
    spread = 260 if big else 70
    corners = [(int(rng.integers(-spread, spread)), int(rng.integers(-40, 60))) for _ in range(n)]
    bands, prec = int(rng.integers(1, 7)), int(rng.integers(0, 3))
    lo, hi = [(-32768, 32767), (0, 255), (-2000, 3000)][int(rng.integers(0, 3))]
    mode = [True, "copy", False][int(rng.integers(0, 3))]
    mb = G.MultiBandBlender(False, bands, prec)
    mb.set_deferred_level0(mode)
    ob = O.MultiBand(bands, prec)
    mb.prepare(corners, sizes)
    ob.prepare(corners, sizes)
    keep = []
    dev = bool(rng.integers(0, 2))
    for (w, h), c in zip(sizes, corners):
        img = rng.integers(lo, hi + 1, (h, w, 3)).astype(np.int16)
        mask = rng.integers(0, 256, (h, w)).astype(np.uint8)
        mask[rng.random((h, w)) < rng.uniform(0, 0.7)] = 0
        mask[rng.random((h, w)) < rng.uniform(0, 0.7)] = 255
        ob.feed(img, mask, c)
        if dev:
            pad, off = int(rng.integers(0, 9)), int(rng.integers(0, 4))
            pitch = w * 3 + pad
            buf = torch.zeros((h * pitch + off + 8,), dtype=torch.int16, device="cuda")
            ti = buf[off:].as_strided((h, w, 3), (pitch, 3, 1))
            ti.copy_(torch.from_numpy(img).cuda())
            tm = torch.from_numpy(mask).cuda()
            keep.append((buf, ti, tm))
            mb.feed(ti, tm, c)
        else:
            mb.feed(img, mask, c)
    kind = int(rng.integers(0, 3)) if prec != 0 else int(rng.integers(0, 2)) * 2
    d, m = mb.blend(out_f32=kind == 1, out_u8=kind == 2)
    d = d.cpu().numpy() if hasattr(d, "cpu") else d
    m = m.cpu().numpy() if hasattr(m, "cpu") else m
    od, om = ob.blend(kind == 1)
    if kind == 2:
        od = np.clip(od, 0, 255).astype(np.uint8)
    assert np.array_equal(m, om)
    assert np.array_equal(d, od), (bands, prec, mode, n, np.argwhere(d != od)[:3])


def case_round4_calls(rng):
    """Round 4's new entries: Blender::NO, isx_convert_to, the gain folded into the fused warp, the mask preparation folded into the feed, and
    the two warps of a tile as calls of their own (image-only / mask-only tile kernels) - each against the oracle's separate stages."""
    which = int(rng.integers(0, 4))
    if which == 0:      # Blender::NO
        n = int(rng.integers(1, 5))
        sizes = [(int(rng.integers(1, 150)), int(rng.integers(1, 120))) for _ in range(n)]
        corners = [(int(rng.integers(-50, 90)), int(rng.integers(-40, 60))) for _ in range(n)]
        nb, ob = G.NoBlender(), O.NoBlend()
        nb.prepare(corners, sizes); ob.prepare(corners, sizes)
        for (w, h), c in zip(sizes, corners):
            img = rng.integers(-32768, 32768, (h, w, 3)).astype(np.int16)
            mask = rng.integers(0, 256, (h, w)).astype(np.uint8) * (rng.random((h, w)) < 0.6)
            nb.feed(img, mask.astype(np.uint8), c); ob.feed(img, mask.astype(np.uint8), c)
        d, m = nb.blend(); od, om = ob.blend()
        assert np.array_equal(m, om) and np.array_equal(d, od)
    elif which == 1:    # convertTo
        h, w, cn = int(rng.integers(1, 90)), int(rng.integers(1, 130)), int(rng.choice([1, 3]))
        f = (rng.standard_normal((h, w, cn) if cn == 3 else (h, w)) * float(rng.choice([3.0, 300.0, 40000.0, 1e12]))).astype(np.float32)
        f.flat[::17] = np.round(f.flat[::17]) + 0.5
        if cn == 3:
            assert np.array_equal(G.convert_to(f, np.int16), O.convert_f32(f, np.int16))
            u = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            assert np.array_equal(G.convert_to(u, np.int16), u.astype(np.int16)) and np.array_equal(G.convert_to(u, np.float32), u.astype(np.float32))
            s16 = rng.integers(-500, 900, (h, w, 3)).astype(np.int16)
            assert np.array_equal(G.convert_to(s16, np.uint8), np.clip(s16, 0, 255).astype(np.uint8))
        else:
            u = rng.integers(0, 256, (h, w)).astype(np.uint8)
            assert np.array_equal(G.convert_to(u, np.float32), u.astype(np.float32))
    elif which == 2:    # gain in the warp + dilate in the feed, through a blend
        w, h = int(rng.integers(8, 300)), int(rng.integers(8, 220))
        f = float(rng.uniform(0.5, 2.0) * max(w, h))
        K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], np.float32)
        kind = int(rng.integers(0, 2))
        Rs = [rot(rng, 0.15), rot(rng, 0.15)]
        wp = (G.CylindricalWarper() if kind == 0 else G.SphericalWarper()).create(f)
        gains = [float(rng.uniform(0.6, 1.6)), 1.0]
        kw, kh = int(rng.integers(1, 34)), int(rng.integers(1, 34))
        typ = int(rng.integers(0, 3))
        nbands = int(rng.integers(1, 5))
        b = [G.MultiBandBlender(False, nbands, 0), G.FeatherBlender(False, 0.1), G.NoBlender()][typ]
        if typ < 2:
            b.set_deferred_level0([False, True, "copy"][int(rng.integers(0, 3))])
        corners, sizes, parts = [], [], []
        for i in range(2):
            src = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            roi, _ = O.detect_roi(kind, f, K, Rs[i], w, h)
            if (roi[2] - roi[0] + 1) * (roi[3] - roi[1] + 1) > 2_000_000 or roi[2] < roi[0] or roi[3] < roi[1]:
                return "skip"
            wp.set_gain(gains[i])
            c, wi, wm = wp.warp_with_mask(src, K, Rs[i])
            oc, owi, _ = O.warp_u8(kind, f, K, Rs[i], src, 1, 2)
            _, owm, _ = O.warp_u8(kind, f, K, Rs[i], np.full((h, w), 255, np.uint8), 0, 0)
            owi = O.gain_apply(owi, gains[i])
            assert tuple(c) == tuple(oc) and np.array_equal(wi, owi) and np.array_equal(wm, owm)
            seam = (rng.random(wm.shape) < rng.choice([0.001, 0.02, 0.4])).astype(np.uint8) * 255
            corners.append(tuple(c)); sizes.append((wm.shape[1], wm.shape[0])); parts.append((wi, seam, wm))
        ob = [O.MultiBand(nbands, 0), O.Feather(0.1), O.NoBlend()][typ]
        b.prepare(corners, sizes)
        ob.prepare(corners, sizes)
        for (wi, seam, wm), c in zip(parts, corners):
            b.feed_dilated(wi.astype(np.int16), seam, wm, kw, kh, c)
            ob.feed(wi.astype(np.int16), O.dilate_rect(seam, kw, kh) & wm, c)
        d, m = b.blend()
        od, om = ob.blend(False) if typ == 0 else ob.blend()
        assert np.array_equal(m, om) and np.array_equal(d, od), (typ, kw, kh)
    else:               # the two warps of a tile as calls of their own, device mats with odd pitches
        import torch
        w, h = int(rng.integers(2, 500)), int(rng.integers(3, 360))
        f = float(rng.uniform(0.3, 3.0) * max(w, h))
        K = np.array([[f, 0, w / 2 + rng.uniform(-3, 3)], [0, f * rng.uniform(0.9, 1.1), h / 2 + rng.uniform(-3, 3)], [0, 0, 1]], np.float32)
        R = rot(rng, 0.6)
        kind = int(rng.integers(0, 2))
        roi, _ = O.detect_roi(kind, f, K, R, w, h)
        if (roi[2] - roi[0] + 1) * (roi[3] - roi[1] + 1) > 3_000_000 or roi[2] < roi[0] or roi[3] < roi[1]:
            return "skip"
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        mask = rng.integers(0, 256, (h, w)).astype(np.uint8)
        wp = (G.CylindricalWarper() if kind == 0 else G.SphericalWarper()).create(f)
        _, owi, _ = O.warp_u8(kind, f, K, R, img, 1, 2)
        _, owm, _ = O.warp_u8(kind, f, K, R, mask, 0, 0)
        dh, dw = owm.shape
        pi, pm = dw * 3 + int(rng.integers(0, 7)), dw + int(rng.integers(0, 7))
        di = torch.zeros((dh * pi + 5,), dtype=torch.uint8, device="cuda")[int(rng.integers(0, 4)):][:dh * pi].as_strided((dh, dw, 3), (pi, 3, 1))
        dm = torch.zeros((dh * pm + 5,), dtype=torch.uint8, device="cuda")[int(rng.integers(0, 4)):][:dh * pm].as_strided((dh, dw), (pm, 1))
        wp.warp(torch.from_numpy(img).cuda(), K, R, 1, 2, dst=di)
        wp.warp(torch.from_numpy(mask).cuda(), K, R, 0, 0, dst=dm)
        assert np.array_equal(di.cpu().numpy(), owi) and np.array_equal(dm.cpu().numpy(), owm)




def case_many_tiles(rng):
    """Round 4: more than 20 tiles in one deferred multi-band cycle - blend() cuts the result into column strips that at most 20 tiles reach
    (run_blend_deferred_strips), or falls back to the eager cycle when a strip is reached by more (tiles stacked); rows with random overlaps,
    sometimes two rows, both tile types, every precision, references and private copies, sometimes inside a caller's column window."""
    import torch
    n = int(rng.integers(21, 45))
    s16 = bool(rng.integers(0, 2))
    rows = int(rng.integers(1, 3))
    corners, sizes, x = [], [], 0
    for i in range(n):
        w, h = int(rng.integers(8, 90)), int(rng.integers(6, 70))
        corners.append((x, int(rng.integers(-10, 11)) + (i % rows) * int(rng.integers(20, 60))))
        sizes.append((w, h))
        x += int(w * rng.uniform(0.0, 0.9))         # 0: a tile over its neighbour (many over one place)
    bands, prec = int(rng.integers(1, 6)), int(rng.integers(0, 3))
    mode = [True, "copy"][int(rng.integers(0, 2))]
    # round 5: one chain over a device-resident table of the tiles (default); one case in three runs round 4's column strips (ISX_TAB=0, read per blend)
    os.environ["ISX_TAB"] = "0" if rng.integers(0, 3) == 0 else "1"
    mb = G.MultiBandBlender(False, bands, prec)
    mb.set_deferred_level0(mode)
    ob = O.MultiBand(bands, prec)
    mb.prepare(corners, sizes)
    ob.prepare(corners, sizes)
    fw, _ = mb.result_size()
    win = None
    if fw > 400 and rng.integers(0, 3) == 0:
        x0 = int(rng.integers(0, fw // 256)) * 128
        x1 = min(x0 + int(rng.integers(1, 6)) * 128, (fw // 128) * 128)
        if x1 > x0:
            win = (x0, x1)
            mb.set_window(x0, x1)
    keep = []
    for (w, h), c in zip(sizes, corners):
        img = rng.integers(-3000, 3001, (h, w, 3)).astype(np.int16) if s16 else rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        mask = rng.integers(0, 256, (h, w)).astype(np.uint8)
        mask[rng.random((h, w)) < rng.uniform(0, 0.5)] = 0
        mask[rng.random((h, w)) < rng.uniform(0, 0.7)] = 255
        ob.feed(img.astype(np.int16), mask, c)
        ti, tm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
        keep.append((ti, tm))
        if s16:
            mb.feed(ti, tm, c)
        else:
            mb.feed_u8(ti, tm, c)
        if mode == "copy":
            ti.fill_(1), tm.fill_(2)
    f32 = prec != 0 and bool(rng.integers(0, 2))
    try:
        d, m = mb.blend(out_f32=f32)
    except Exception as e:      # the one refusal of the path: a caller's window with more than 20 tiles over one 128-column strip (no eager cycle to fall back to)
        if win and "more than 20 tiles reach" in str(e):
            return "skip"
        raise
    finally:
        os.environ.pop("ISX_TAB", None)
    d, m = d.cpu().numpy(), m.cpu().numpy()
    od, om = ob.blend(f32)
    if win:
        od, om = od[:, win[0]:win[1]], om[:, win[0]:win[1]]
    assert np.array_equal(m, om)
    assert np.array_equal(d, od), (n, bands, prec, mode, win, mb.last_path(), np.argwhere(d != od)[:3])


def case_fused_feed(rng):
    """Round 5: feed() of mode 2 as ONE pass (k_feed_strip / k_feed_pd0: level 1 + the private copy out of one read of the caller's tile) with the
    copy of a CV_16SC3 tile narrowed to CV_8UC3 while its values are bytes.  Two to four CYCLES of one blender whose tiles are all bytes, bytes but
    for one value somewhere (an escaped segment: the cycle is widened before the last step), or full-range shorts (the blender keeps wide copies
    from the first violation on), CV_16SC3 or CV_8UC3 tiles, random sizes and offsets (rim strips everywhere), 1-6 bands, every precision, the
    caller's mats poisoned after feed(), now and then a column window or level introspection between feed and blend."""
    import torch
    n = int(rng.integers(1, 5))
    big = bool(rng.integers(0, 3))
    sizes = [(int(rng.integers(2, 700 if big else 90)), int(rng.integers(2, 400 if big else 80))) for _ in range(n)]
    spread = 420 if big else 60
    corners = [(int(rng.integers(-spread, spread)), int(rng.integers(-50, 70))) for _ in range(n)]
    bands, prec = int(rng.integers(1, 7)), int(rng.integers(0, 3))
    u8 = rng.integers(0, 4) == 0
    mb = G.MultiBandBlender(False, bands, prec)
    mb.set_deferred_level0("copy")
    violated = False
    for cycle in range(int(rng.integers(2, 5))):
        kind = "bytes" if u8 else ["bytes", "bytes", "one", "full"][int(rng.integers(0, 4))]
        ob = O.MultiBand(bands, prec)
        mb.prepare(corners, sizes)
        ob.prepare(corners, sizes)
        fw, _ = mb.result_size()
        win = None
        if fw >= 256 and rng.integers(0, 4) == 0:
            x0 = int(rng.integers(0, fw // 128)) * 128
            x1 = min(x0 + int(rng.integers(1, 4)) * 128, fw + 64)
            win = (x0, x1)
        any_bad = False
        for (w, h), c in zip(sizes, corners):
            if kind == "full":
                img = rng.integers(-32768, 32768, (h, w, 3)).astype(np.int16)
            else:
                img = rng.integers(0, 256, (h, w, 3)).astype(np.int16)
                if kind == "one" and rng.integers(0, 2):
                    img[int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, 3))] = [256, -1, 32767, -32768, 300][int(rng.integers(0, 5))]
            any_bad = any_bad or bool(((img < 0) | (img > 255)).any())
            mask = rng.integers(0, 256, (h, w)).astype(np.uint8)
            mask[rng.random((h, w)) < rng.uniform(0, 0.7)] = 0
            mask[rng.random((h, w)) < rng.uniform(0, 0.7)] = 255
            ob.feed(img, mask, c)
            if u8:
                ti = torch.from_numpy(img.astype(np.uint8)).cuda()
            else:       # a device view at an odd alignment (a 2-byte aligned row start is all the windows may assume)
                pad, off = int(rng.integers(0, 9)), int(rng.integers(0, 4))
                pitch = w * 3 + pad
                buf = torch.zeros((h * pitch + off + 8,), dtype=torch.int16, device="cuda")
                ti = buf[off:].as_strided((h, w, 3), (pitch, 3, 1))
                ti.copy_(torch.from_numpy(img).cuda())
            tm = torch.from_numpy(mask).cuda()
            (mb.feed_u8 if u8 else mb.feed)(ti, tm, c)
            ti.fill_(77 if u8 else -7), tm.fill_(99)
        if win is None and bands <= 4 and rng.integers(0, 6) == 0:
            lvl = int(rng.integers(0, mb.numBands() + 1))
            gl, gw = mb.level(lvl)
            ol, ow = ob.level(lvl)
            assert np.array_equal(gl, ol) and np.array_equal(gw, ow), ("level", lvl)
        if win:
            mb.set_window(*win)
        f32 = prec != 0 and bool(rng.integers(0, 2))
        d, m = mb.blend(out_f32=f32)
        if win:
            mb.set_window(0, 0)
        d, m = d.cpu().numpy(), m.cpu().numpy()
        od, om = ob.blend(f32)
        if win:
            od, om = od[:, win[0]:win[1]], om[:, win[0]:win[1]]
            d, m = d[:, :od.shape[1]], m[:, :om.shape[1]]
        path = mb.feed_path()
        assert np.array_equal(m, om), (cycle, kind)
        assert np.array_equal(d, od), (cycle, kind, n, bands, prec, path, np.argwhere(d != od)[:3])
        if not u8 and path["fused_tiles"] == n:
            want = "none" if violated else ("widened" if any_bad else "confirmed")
            assert path["narrowed"] == want, (path, want, cycle, kind)
            violated = violated or any_bad


def case_round6_calls(rng):
    """Round 6: (a) 1 - 9 tiles' fused warps collected by isx_warper_begin_batch and launched as one kernel per variant (blockIdx.z = tile; random
    sizes, cameras, CV_8UC3 / CV_16SC3 outputs, dense / pitched rows, now and then a call in the middle that cannot be collected) - every tile
    against the oracle's warp; (b) isx_warper_roi, which ranks the border on the caller's thread where the extrema provably lie there, against the
    oracle's scan of every source pixel (ROI and float extrema), the host-only self-test entry included."""
    import ctypes as C
    import torch
    kind = int(rng.integers(0, 2))
    f = float(rng.uniform(150.0, 900.0))
    wp = (G.CylindricalWarper() if kind == 0 else G.SphericalWarper()).create(f)
    if rng.integers(0, 2):
        wp.set_deferred_verify(True)
    nt = int(rng.integers(1, 10))
    jobs = []
    for i in range(nt):
        w, h = int(rng.integers(2, 420)), int(rng.integers(2, 300))
        K = np.array([[f * rng.uniform(0.8, 1.2), 0, w / 2 + rng.uniform(-5, 5)], [0, f * rng.uniform(0.8, 1.2), h / 2 + rng.uniform(-5, 5)], [0, 0, 1]], np.float32)
        R = rot(rng, float(rng.choice([0.2, 0.6, 1.2])))
        oroi, omm = O.detect_roi(kind, f, K, R, w, h)
        dw, dh = int(oroi[2]) - int(oroi[0]) + 1, int(oroi[3]) - int(oroi[1]) + 1
        if dw < 1 or dh < 1 or dw > 60000 or dh > 60000 or dw * dh > 1_500_000:
            continue
        roi, mm = wp.warpRoi((w, h), K, R, with_minmax=True)
        assert tuple(int(v) for v in roi) == tuple(int(v) for v in oroi), (roi, oroi)
        assert np.array_equal(np.asarray(mm, np.float32), omm), (mm, omm)
        # the host-only entry: the same answer wherever it answers at all
        hr, hm = np.zeros(4, np.int32), np.zeros(4, np.float32)
        fp = C.POINTER(C.c_float)
        Kc, Rc = np.ascontiguousarray(K.reshape(9)), np.ascontiguousarray(R.reshape(9))
        rc = G.load().isx_selftest_roi_host(kind, C.c_float(f), Kc.ctypes.data_as(fp), Rc.ctypes.data_as(fp), w, h, int(rng.integers(0, 2)),
                                            hr.ctypes.data_as(C.POINTER(C.c_int)), hm.ctypes.data_as(fp))
        if rc == 0:
            assert np.array_equal(hr, oroi) and np.array_equal(hm, omm), (hr, oroi, hm, omm)
        src = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        out16, pitched = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        es = 2 if out16 else 1
        pit = (dw * 3 * es + 63) // 64 * 64 if pitched else dw * 3 * es
        di = torch.full((dh * pit // es,), 77, dtype=torch.int16 if out16 else torch.uint8, device="cuda").as_strided((dh, dw, 3), (pit // es, 3, 1))
        pm = (dw + 63) // 64 * 64 if pitched else dw
        dm = torch.full((dh * pm,), 99, dtype=torch.uint8, device="cuda").as_strided((dh, dw), (pm, 1))
        smask = None
        if rng.random() < 0.15:          # a caller-supplied source mask: launched at once, not collected
            smask = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
        jobs.append((torch.from_numpy(src).cuda(), K, R, [int(v) for v in oroi], di, dm, src, out16, smask, (w, h)))
    if not jobs:
        return "skip"
    wp.begin_batch()
    for (t, K, R, roi, di, dm, src, out16, smask, _) in jobs:
        wp.warp_with_mask_planned(t, K, R, roi, di, dm, mask=None if smask is None else torch.from_numpy(smask).cuda())
    wp.end_batch()
    wp.plan_status()
    for (t, K, R, roi, di, dm, src, out16, smask, (w, h)) in jobs:
        _, oi, _ = O.warp_u8(kind, f, K, R, src, 1, 2)
        _, om, _ = O.warp_u8(kind, f, K, R, np.full((h, w), 255, np.uint8) if smask is None else smask, 0, 0)
        assert np.array_equal(di.cpu().numpy(), oi.astype(np.int16) if out16 else oi), np.argwhere(di.cpu().numpy() != oi)[:3]
        assert np.array_equal(dm.cpu().numpy(), om)


def case_long_lived(rng):
    """One warper and one blender kept for a random sequence of 5-30 operations, as a video stitcher keeps them (the parity families above
    create fresh handles per call): warps of new and repeated ROIs, multi-band cycles of 2-19 and 21-30 tiles (both sides of DEF_MAX, i.e.
    kernel-argument tile sets and the device table), band-count changes, eager / deferred / deferred-copy feeds, CV_8UC3 and CV_16SC3 tiles,
    and set_stream between torch streams (the new stream ordered behind the old one).  The precision is a property of the handle
    (isx_blender_create): each case draws one.  The case owns its handles, so its seed replays it.  Every result against the oracle."""
    import torch
    prec = int(rng.integers(0, 3))
    kind = int(rng.integers(0, 2))
    sw, sh = int(rng.integers(24, 90)), int(rng.integers(8, 40))
    f = float(rng.uniform(0.6, 2.0) * sw)
    K = np.array([[f, 0, sw / 2], [0, f, sh / 2], [0, 0, 1]], np.float32)
    src = rng.integers(0, 256, (sh, sw, 3)).astype(np.uint8)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    cur = streams[0]
    wp = (G.CylindricalWarper() if kind == 0 else G.SphericalWarper()).create(f)
    wp.set_roi_cache(bool(rng.integers(0, 2)))
    mb = G.MultiBandBlender(False, int(rng.integers(1, 6)), prec)
    cams = []
    src_dev = torch.from_numpy(src).cuda()
    for _ in range(int(rng.integers(5, 31))):
        op = rng.choice(["warp", "warp", "cycle", "cycle", "stream"])
        if op == "stream":
            nxt = streams[int(rng.integers(0, 3))]
            nxt.wait_stream(cur)
            cur = nxt
            wp.set_stream(cur)
            mb.set_stream(cur)
        elif op == "warp":
            if cams and rng.integers(0, 3) == 0:
                R = cams[int(rng.integers(0, len(cams)))]
            else:
                R = rot(rng, 0.6)
                cams.append(R)
            roi, _ = O.detect_roi(kind, f, K, R, sw, sh)
            if roi[2] < roi[0] or roi[3] < roi[1] or (roi[2] - roi[0] + 1) * (roi[3] - roi[1] + 1) > 1_000_000:
                continue
            with torch.cuda.stream(cur):
                c, wi, wm = wp.warp_with_mask(src_dev, K, R)
                wi, wm = wi.cpu().numpy(), wm.cpu().numpy()
            oc, oi, _ = O.warp_u8(kind, f, K, R, src, 1, 2)
            _, om, _ = O.warp_u8(kind, f, K, R, np.full((sh, sw), 255, np.uint8), 0, 0)
            assert tuple(c) == tuple(oc), (c, oc)
            assert np.array_equal(wi, oi) and np.array_equal(wm, om), ("warp", kind, np.argwhere(wi != oi)[:3])
        else:
            n = int(rng.integers(2, 20)) if rng.integers(0, 2) else int(rng.integers(21, 31))
            bands = int(rng.integers(0, 7))
            mode = [False, True, "copy"][int(rng.integers(0, 3))]
            s16 = bool(rng.integers(0, 2))
            corners, sizes, x = [], [], int(rng.integers(-20, 20))
            for i in range(n):
                w, h = int(rng.integers(8, 70)), int(rng.integers(6, 50))
                corners.append((x, int(rng.integers(-8, 9))))
                sizes.append((w, h))
                x += int(w * rng.uniform(0.2, 0.9))
            mb.setNumBands(bands)
            mb.set_deferred_level0(mode)
            ob = O.MultiBand(bands, prec)
            ob.prepare(corners, sizes)
            keep = []
            with torch.cuda.stream(cur):
                mb.prepare(corners, sizes)
                for (w, h), c in zip(sizes, corners):
                    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
                    mask = ((rng.random((h, w)) > rng.uniform(0, 0.4)) * 255).astype(np.uint8)
                    ob.feed(img.astype(np.int16), mask, c)
                    ti = torch.from_numpy(img.astype(np.int16) if s16 else img).cuda()
                    tm = torch.from_numpy(mask).cuda()
                    keep.append((ti, tm))
                    if s16:
                        mb.feed(ti, tm, c)
                    else:
                        mb.feed_u8(ti, tm, c)
                f32 = prec != 0 and bool(rng.integers(0, 2))
                d, m = mb.blend(out_f32=f32)
                d, m = d.cpu().numpy(), m.cpu().numpy()
            od, om = ob.blend(f32)
            assert np.array_equal(m, om), ("cycle mask", n, bands, prec, mode, s16)
            assert np.array_equal(d, od), ("cycle", n, bands, prec, mode, s16, mb.last_path(), np.argwhere(d != od)[:3])
    torch.cuda.synchronize()


# ---- the families of the entry points merged after round 6 -----------------------------------------------------------------------------
# Each is three functions: gen_X(rng) draws the inputs (a dict; case["cls"] names the shape class), model_X(case) runs the NumPy model -
# neither needs a GPU, tests/test_fuzz_generators.py runs them alone - and case_X(rng) runs the GPU entry on them and asserts.  The shape
# classes sit on the kernels' tiling constants, which are read from the kernels' sources: a constant that moves takes its classes along.

def _kernel_consts(name):
    """The `constexpr int NAME = <integer or earlier name> [* <integer or earlier name>]...;` definitions of imagestitch_amd/csrc/<name>
    (several in one declaration too); definitions of another form, such as shifts, are left out, and a name in a product that was left out
    is an error."""
    import re
    out = {}
    with open(os.path.join(ROOT, "imagestitch_amd", "csrc", name)) as f:
        text = f.read()
    for decl in re.findall(r"constexpr\s+int\s+([^;{}()]+);", text):
        for part in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(\w+(?:\s*\*\s*\w+)*)\s*", part)
            if not m:
                continue
            value = 1
            for tok in re.split(r"\s*\*\s*", m.group(2)):
                if not tok.isdigit() and tok not in out:
                    raise ValueError("%s: %s is defined through %s, which is no integer constant read before it" % (name, m.group(1), tok))
                value *= int(tok) if tok.isdigit() else out[tok]
            out[m.group(1)] = value
    return out


_VR, _GC, _GF, _SM, _BG = (_kernel_consts(n) for n in ("voronoi.hip", "graphcut.hip", "gain.hip", "seam.hip", "blocks_gain.hip"))
SEAM_GAP = 10                                                           # the gap of OpenCV's pairwise seam finders: grids are roi + 2 * gap a side
VR_WIDTHS = [_VR["VR_CHUNK"] - 1, _VR["VR_CHUNK"], _VR["VR_CHUNK"] + 1, 2 * _VR["VR_CHUNK"], 2 * _VR["VR_CHUNK"] + 1]      # of a submask
VR_HEIGHTS = [_VR["VR_SEG"] - 1, _VR["VR_SEG"], _VR["VR_SEG"] + 1, 2 * _VR["VR_SEG"], 2 * _VR["VR_SEG"] + 1]
GC_WIDTHS = [_GC["GC_TW"] - 1, _GC["GC_TW"], _GC["GC_TW"] + 1, 2 * _GC["GC_TW"], 2 * _GC["GC_TW"] + 1]                      # of a padded grid
GC_HEIGHTS = [2 * _GC["GC_TH"] - 1, 2 * _GC["GC_TH"], 2 * _GC["GC_TH"] + 1, 3 * _GC["GC_TH"]]                                # (one tile row is below roi + 20)
GF_PAIR_SIZES = [_GF["GF_PAIR_PIXELS"] - 1, _GF["GF_PAIR_PIXELS"], _GF["GF_PAIR_PIXELS"] + 1, 2 * _GF["GF_PAIR_PIXELS"], 2 * _GF["GF_PAIR_PIXELS"] + 1]
GF_DIAG_SIZES = [_GF["GF_DIAG_BYTES"] - 1, _GF["GF_DIAG_BYTES"], _GF["GF_DIAG_BYTES"] + 1]
GRAD_WIDTHS = [_SM["GRAD_TW"] - 1, _SM["GRAD_TW"], _SM["GRAD_TW"] + 1, 2 * _SM["GRAD_TW"] + 1]
GRAD_HEIGHTS = [_SM["GRAD_TH"] - 1, _SM["GRAD_TH"], _SM["GRAD_TH"] + 1, 2 * _SM["GRAD_TH"] + 1]

PLANE_ALL_PAIRS_BELOW = 1 << 17                                          # result pixels up to which case_plane_warp runs all eight warp() modes
PLANE_CLASSES = ["plain", "tiny", "odd_width", "with_T"]
GAIN_CLASSES = ["plain", "pair_item_edge", "diag_item_edge", "one_pixel_overlap", "disjoint_pair"]
VORONOI_CLASSES = ["plain", "chunk_edge", "seg_edge", "thin", "no_unique_rows"]
GRAPHCUT_CLASSES = ["plain", "tile_edge_w", "tile_edge_h", "flat_tie", "holes_heavy"]
GRAPHCUT_GRAD_CLASSES = ["tile_edge_w", "tile_edge_h", "flat_tie", "holes_heavy", "smooth", "noise", "structured"]
GCG_MAX_NODES = 4600                                                    # padded-grid nodes of a case's first pair (gen_graphcut_grad)
GCG_THIRD_TILE = (24, 16)                                               # the third tile is at most this wide and high
SEAM_GRAD_CLASSES = ["plain", "tile_edge", "one_pixel", "rect_at_border", "find"]          # the first four: seam_gradients; "find": the whole finder
BLOCKS_GAIN_CLASSES = ["plain", "several_items", "wide_row", "one_pixel_blocks", "no_pairs", "one_pixel_meeting", "apply_edges"]
BG_WIDE_ROWS = [_GF["GF_PAIR_PIXELS"] + d for d in (-1, 0, 1, 5)]          # the width of a pair of blocks whose band is one row
BG_APPLY_WIDTHS = [_BG["BA_PX"] * 64 * k + d for k in (1, 2) for d in (-1, 0, 1)]      # a workgroup of k_blocks_gain_apply: a wave of BA_PX pixels a lane wide,
BG_APPLY_HEIGHTS = [4 * _BG["BA_ROWS"] + d for d in (-1, 0, 1)]                        # its four waves BA_ROWS rows each high
BG_MAX_UNKNOWNS = 250                                                     # the dense model is O(B^2) in Python; below LU_NT and LU_PNT: one column block of
assert BG_MAX_UNKNOWNS < _BG["LU_NT"] <= _BG["LU_PNT"] and _BG["LU_RB"] > 0                # k_lu_update, one stride of k_lu_pivot (larger: the solver's own test)
WHERE = ["host", "device", "host_view", "device_view"]
_RZ = _kernel_consts("resize.hip")
RESIZE_CLASSES = ["plain", "wave_edge", "rows_edge", "half", "half_one_axis", "tiny_src", "steep", "specials"]
RZ_WAVE_WIDTHS = [_RZ["RZ_PX"] * 64 * k + d for k in (1, 2) for d in (-1, 0, 1)]          # of a destination: a wave of the resize kernels, RZ_PX pixels a lane
RZ_ROW_HEIGHTS = [4 * k + d for k in (1, 2) for d in (-1, 0, 1)] + [4 * _RZ["DR_ROWS"] * k + d for k in (1, 2) for d in (-1, 0, 1)]      # a workgroup of k_resize (4 rows) and of
RZ_MAX_SHAPE = (300, 1100)                                                # k_dilate_resize_and (4 waves of DR_ROWS rows); no mat of a case above this (rows, cols)
RZ_TYPES = [("uint8", 1), ("uint8", 3), ("float32", 1), ("float32", 3)]
RZ_ELEMENTS = [(3, 3), (1, 1), (2, 5), (20, 20), (4, 4)]
RZ_STAGE_MODES = ["no_warped", "warped", "in_place"]


def overlap_roi(tl1, tl2, sz1, sz2):
    """cv::detail::overlapRoi: (x, y, w, h) or None.  sz = (width, height)."""
    x_tl, y_tl = max(tl1[0], tl2[0]), max(tl1[1], tl2[1])
    x_br, y_br = min(tl1[0] + sz1[0], tl2[0] + sz2[0]), min(tl1[1] + sz1[1], tl2[1] + sz2[1])
    return (x_tl, y_tl, x_br - x_tl, y_br - y_tl) if x_tl < x_br and y_tl < y_br else None


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _factor_pair(rng, n):
    """(w, h) with w * h == n, any divisor pair in either order."""
    w = _pick(rng, [d for d in range(1, n + 1) if n % d == 0])
    return w, n // w


def _pair_with_overlap(rng, ow, oh):
    """Two tiles whose overlapRoi is exactly ow x oh: (corners, sizes), the tile that starts the overlap first or second."""
    a, b, c, d = (int(v) for v in rng.integers(0, 16, 4))
    x0, y0 = int(rng.integers(-40, 40)), int(rng.integers(-30, 30))
    corners, sizes = [(x0, y0), (x0 + a, y0 + b)], [(ow + a, oh + b), (ow + c, oh + d)]
    if rng.integers(0, 2):
        corners.reverse(); sizes.reverse()
    return corners, sizes


def _tile_onto(rng, corners, sizes, wr, hr):
    """One more tile of wr x hr (ranges) that overlaps one of the tiles placed so far near that tile's corner."""
    w, h = int(rng.integers(*wr)), int(rng.integers(*hr))
    k = int(rng.integers(0, len(corners)))
    corners.append((corners[k][0] + int(rng.integers(-w + 1, min(sizes[k][0], 60))), corners[k][1] + int(rng.integers(-h + 1, min(sizes[k][1], 40)))))
    sizes.append((w, h))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _place(arrays, where, seed):
    """The arrays as the GPU entry gets them: host copies, device tensors, or (the views() of the fixed-seed files) each one inside a larger
    buffer of 7s at an odd offset with a pitch that is no multiple of 16.  -> [(mat, buffer or None, (oy, ox, h, w))]"""
    out = []
    for k, a in enumerate(arrays):
        h, w = a.shape[:2]
        if not where.endswith("_view"):
            out.append((_dev(a) if where == "device" else a.copy(), None, None))
            continue
        oy, ox, pad = 1 + k % 3, 1 + (k + seed) % 5, 3 + 2 * k
        b = np.full((h + oy + 2, w + ox + pad) + a.shape[2:], 7, a.dtype)
        if where == "device_view":
            b = _dev(b)
        v = b[oy:oy + h, ox:ox + w]
        v[...] = _dev(a) if where == "device_view" else a
        out.append((v, b, (oy, ox, h, w)))
    return out


def _frame_untouched(placed):
    for k, (_, b, box) in enumerate(placed):
        if b is not None:
            frame = _host(b).copy()
            frame[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = 7
            assert (frame == 7).all(), ("wrote outside view", k)


# ---- the plane projector ------------------------------------------------------------------------------------------------------------------
def gen_plane_warp(rng):
    """The rig of _rig() in tests/test_gpu_plane_warp.py (angles up to +-0.5 rad, T zero or not) on a 2..400 x 2..300 source of 1 or 3 channels."""
    from imagestitch_amd import synth
    cls = _pick(rng, PLANE_CLASSES)
    w, h = int(rng.integers(2, 401)), int(rng.integers(2, 301))
    if cls == "tiny":
        w, h = int(rng.integers(2, 5)), int(rng.integers(2, 5))
    elif cls == "odd_width" and w % 2 == 0:
        w = w - 1 if w > 2 else 3
    with_t = cls == "with_T" or (cls != "plain" and bool(rng.integers(0, 2)))
    f = float(rng.uniform(0.9, 2.0) * max(w, h))
    K = np.array([[f, 0, w / 2 + rng.uniform(-3, 3)], [0, f * rng.uniform(0.95, 1.05), h / 2 + rng.uniform(-3, 3)], [0, 0, 1]], np.float32)
    yaw, pitch, roll = rng.uniform(-0.5, 0.5, 3)
    R = (synth._rot("y", yaw) @ synth._rot("x", pitch) @ synth._rot("z", roll)).astype(np.float32)
    T = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)], np.float32) if with_t else None
    cn = int(rng.choice([1, 3]))
    return dict(cls=cls, w=w, h=h, scale=float(f * rng.uniform(0.7, 1.3)), K=K, R=R, T=T, cn=cn,
                src=rng.integers(0, 256, (h, w, 3) if cn == 3 else (h, w)).astype(np.uint8),
                interp=int(rng.integers(0, 2)), border=int(rng.choice([0, 1, 2, 4])), where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)),
                points=[(0.0, 0.0), (float(w - 1), float(h - 1))] + [(float(rng.uniform(0, w)), float(rng.uniform(0, h))) for _ in range(3)])


def model_plane_warp(c):
    from helpers import plane_np
    m = plane_np.from_rig(O, c["scale"], c["K"], c["R"], c["T"])
    roi, mm = m.detect_roi(c["w"], c["h"])
    roi = [int(v) for v in roi]
    if roi[2] < roi[0] or roi[3] < roi[1] or (roi[2] - roi[0] + 1) * (roi[3] - roi[1] + 1) > 4_000_000:
        return "skip"
    xm, ym = m.build_maps(roi)
    pairs = [(c["interp"], c["border"])]
    if xm.size <= PLANE_ALL_PAIRS_BELOW:                               # a small result: every interpolation with every border
        pairs = [(i, b) for i in (0, 1) for b in (0, 1, 2, 4)]
    want = dict(roi=tuple(roi), mm=mm, xmap=xm, ymap=ym, warp={ib: O.remap(c["src"], xm, ym, *ib) for ib in pairs},
                points=[m.map_forward(np.float32(x), np.float32(y)) for x, y in c["points"]])
    if c["cn"] == 3:
        want["img"] = O.remap(c["src"], xm, ym, 1, 2)
        want["mask"] = O.remap(np.full((c["h"], c["w"]), 255, np.uint8), xm, ym, 0, 0)
    return want


def case_plane_warp(rng):
    """ISX_WARP_PLANE with set_translation: warpRoi, buildMaps, warp (all 2 x 4 interpolation / border pairs where the result has at most
    PLANE_ALL_PAIRS_BELOW pixels, the one pair the case drew above that), the fused warp_with_mask and warpPoint against
    tests/helpers/plane_np.py."""
    c = gen_plane_warp(rng)
    want = model_plane_warp(c)
    if want == "skip":
        return "skip"
    wp = G.PlaneWarper().create(c["scale"])
    if c["T"] is not None:
        wp.set_translation(c["T"])
    size, K, R = (c["w"], c["h"]), c["K"], c["R"]
    roi, mm = wp.warpRoi(size, K, R, with_minmax=True)
    assert tuple(roi) == want["roi"] and np.array_equal(mm, want["mm"]), (roi, want["roi"], mm, want["mm"])
    r2, gx, gy = wp.buildMaps(size, K, R, like=_dev(np.zeros(1, np.float32)) if c["where"].startswith("device") else None)
    assert tuple(r2) == want["roi"] and np.array_equal(_host(gx), want["xmap"], equal_nan=True) and np.array_equal(_host(gy), want["ymap"], equal_nan=True)
    src = _place([c["src"]], c["where"], c["view_seed"])[0][0]
    for (interp, border), w in want["warp"].items():
        corner, dst = wp.warp(src, K, R, interp, border)
        d = _host(dst)
        assert tuple(corner) == want["roi"][:2] and np.array_equal(d, w), (interp, border, np.argwhere(d != w)[:3])
    if c["cn"] == 3:
        corner, gi, gm = wp.warp_with_mask(src, K, R)
        assert tuple(corner) == want["roi"][:2] and np.array_equal(_host(gi), want["img"]) and np.array_equal(_host(gm), want["mask"])
    for (x, y), (mu, mv) in zip(c["points"], want["points"]):
        u, v = wp.warpPoint((x, y), K, R)
        assert np.array_equal(np.array([u, v]), np.array([mu, mv]), equal_nan=True), (x, y, u, mu, v, mv)


# ---- GainCompensator::feed ----------------------------------------------------------------------------------------------------------------
def gen_gain_feed(rng):
    """2..7 tiles, masks of 0 / 254 / 255.  The first two tiles carry the class: an overlap rectangle or a mask on a work-item boundary of
    gain.hip (GF_PAIR_PIXELS overlap pixels, GF_DIAG_BYTES mask bytes per item), one shared pixel, or no overlap at all; every further tile
    overlaps one placed before it."""
    cls = _pick(rng, GAIN_CLASSES)
    n = int(rng.integers(3 if cls in ("one_pixel_overlap", "disjoint_pair") else 2, 8))
    if cls == "pair_item_edge":
        corners, sizes = _pair_with_overlap(rng, *_factor_pair(rng, _pick(rng, GF_PAIR_SIZES)))
    elif cls == "diag_item_edge":
        w, h = _factor_pair(rng, _pick(rng, GF_DIAG_SIZES))
        corners, sizes = [(int(rng.integers(-40, 40)), int(rng.integers(-30, 30)))], [(w, h)]
    else:
        corners, sizes = [(int(rng.integers(-40, 40)), int(rng.integers(-30, 30)))], [(int(rng.integers(8, 160)), int(rng.integers(6, 120)))]
        if cls != "plain":
            (x0, y0), (w0, h0) = corners[0], sizes[0]
            sizes.append((int(rng.integers(8, 160)), int(rng.integers(6, 120))))
            corners.append((x0 + w0 - 1, y0 + h0 - 1) if cls == "one_pixel_overlap" else (x0 + w0 + int(rng.integers(0, 3)), y0 + int(rng.integers(-5, 6))))
    while len(sizes) < n:                                                # (large enough that most overlaps take several work items)
        _tile_onto(rng, corners, sizes, (8, 160), (6, 120))
    imgs, masks = [], []
    for w, h in sizes:
        imgs.append(rng.integers(int(rng.integers(0, 80)), 256, (h, w, 3), dtype=np.uint8))
        masks.append(rng.choice(np.array([0, 254, 255, 255, 255, 255], np.uint8), size=(h, w)))
    if cls == "one_pixel_overlap":                                     # the shared pixel counts on both sides
        masks[0][-1, -1] = masks[1][0, 0] = 255
    return dict(cls=cls, corners=corners, sizes=sizes, imgs=imgs, masks=masks, where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)))


def model_gain_feed(c):
    from test_gain_model import feed_model
    N, I, _, _, _, g = feed_model(c["corners"], c["imgs"], c["masks"])
    return dict(N=N, I=I, gains=g)


def case_gain_feed(rng):
    """isx_gain_compensator_feed against feed_model of tests/test_gain_model.py: N exactly, I bit for bit, gains to 1e-12 relative."""
    c = gen_gain_feed(rng)
    want = model_gain_feed(c)
    imgs = [p[0] for p in _place(c["imgs"], c["where"], c["view_seed"])]
    masks = [p[0] for p in _place(c["masks"], c["where"], c["view_seed"] + 1)]
    comp = G.GainCompensator().feed(c["corners"], imgs, masks)
    assert np.array_equal(comp.N, want["N"]), (c["cls"], comp.N, want["N"])
    assert np.array_equal(comp.I.view(np.uint64), want["I"].view(np.uint64)), (c["cls"], comp.I, want["I"])
    np.testing.assert_allclose(comp.gains(), want["gains"], rtol=1e-12, atol=0)


# ---- VoronoiSeamFinder --------------------------------------------------------------------------------------------------------------------
def gen_voronoi(rng):
    """2..4 tiles, per-cell holes of density 0..0.5, now and then an all-zero mask.  The first two tiles carry the class: a submask
    (roi + 20) as wide as 1 or 2 of voronoi.hip's row-pass chunks +-1, as high as 1 or 2 of its column segments +-1, a roi one cell wide
    or high, or rows of the overlap where neither tile has a cell of its own."""
    cls = _pick(rng, VORONOI_CLASSES)
    n = int(rng.integers(2, 5))
    g2 = 2 * SEAM_GAP
    if cls == "chunk_edge":
        corners, sizes = _pair_with_overlap(rng, _pick(rng, VR_WIDTHS) - g2, int(rng.integers(1, 9)))
    elif cls == "seg_edge":
        corners, sizes = _pair_with_overlap(rng, int(rng.integers(10, 80)), _pick(rng, VR_HEIGHTS) - g2)
    elif cls == "thin":
        ow, oh = (1, int(rng.integers(1, 60))) if rng.integers(0, 2) else (int(rng.integers(1, 80)), 1)
        corners, sizes = _pair_with_overlap(rng, ow, oh)
    elif cls == "no_unique_rows":                                       # one column range, tile 1 lower: the overlap's rows are collisions or nothing
        w, h, x0, y0 = int(rng.integers(20, 80)), int(rng.integers(12, 50)), int(rng.integers(-40, 40)), int(rng.integers(-30, 30))
        corners, sizes = [(x0, y0), (x0, y0 + int(rng.integers(1, h - 2)))], [(w, h), (w, h)]
    else:
        sizes = [(int(rng.integers(20, 90)), int(rng.integers(15, 70))) for _ in range(2)]
        corners = [(int(rng.integers(-30, 30)), int(rng.integers(-20, 20))) for _ in range(2)]
    while len(sizes) < n:
        _tile_onto(rng, corners, sizes, (20, 90), (15, 70))
    masks = []
    for w, h in sizes:
        m = rng.integers(1, 256, (h, w)).astype(np.uint8)             # any non-zero byte is "set"
        m[rng.random((h, w)) < rng.uniform(0, 0.5)] = 0
        masks.append(m)
    if cls == "no_unique_rows":
        x, ww = int(rng.integers(0, sizes[0][0] // 2)), int(rng.integers(1, sizes[0][0] // 2))
        for m in masks[:2]:
            m[m == 0] = 255
            m[:, x:x + ww] = 0
    if rng.integers(0, 8) == 0:
        k = int(rng.integers(0, n))
        for m in (masks[:2] if cls == "no_unique_rows" and k < 2 else masks[k:k + 1]):       # (one of that pair empty would leave the other's cells unique)
            m[...] = 0
    return dict(cls=cls, corners=corners, sizes=sizes, masks=masks, where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)))


def model_voronoi(c):
    from helpers import voronoi_np
    out = [m.copy() for m in c["masks"]]
    voronoi_np.find(c["sizes"], c["corners"], out)
    return out


def case_voronoi(rng):
    """isx_voronoi_seam_find against tests/helpers/voronoi_np.py: masks byte for byte, nothing written around a view."""
    c = gen_voronoi(rng)
    want = model_voronoi(c)
    placed = _place(c["masks"], c["where"], c["view_seed"])
    G.VoronoiSeamFinder().find(c["sizes"], c["corners"], [p[0] for p in placed])
    for k, (p, w) in enumerate(zip(placed, want)):
        got = _host(p[0])
        assert np.array_equal(got, w), (c["cls"], k, int((got != w).sum()), np.argwhere(got != w)[:3])
    _frame_untouched(placed)


# ---- GraphCutSeamFinder(COST_COLOR) -------------------------------------------------------------------------------------------------------
def gen_graphcut(rng):
    """2..3 tiles, CV_8UC3 or CV_32FC3, smooth (the layout() of tests/test_gpu_graphcut_seam.py), noise or constant images - with constant
    images every edge weighs the same, many cuts tie and only the maximal source side is right.  The first two tiles carry the class: a
    padded grid (roi + 20) as wide as 1 or 2 of graphcut.hip's BFS tiles +-1 or as high as 2 or 3 of them, constant images, or masks
    with 30 % of their cells zero.  No roi above about 130 x 100: the model's max-flow stays in milliseconds."""
    cls = _pick(rng, GRAPHCUT_CLASSES)
    n = int(rng.integers(2, 4))
    g2 = 2 * SEAM_GAP
    if cls == "tile_edge_w":
        corners, sizes = _pair_with_overlap(rng, _pick(rng, GC_WIDTHS) - g2, int(rng.integers(8, 60)))
    elif cls == "tile_edge_h":
        corners, sizes = _pair_with_overlap(rng, int(rng.integers(8, 90)), _pick(rng, GC_HEIGHTS) - g2)
    else:                                                               # the sizes and corners of the fixed-seed file's layout()
        sizes = [(int(rng.integers(40, 90)), int(rng.integers(30, 70))) for _ in range(2)]
        corners = [(int(rng.integers(-30, 30)), int(rng.integers(-20, 20))) for _ in range(2)]
    while len(sizes) < n:
        _tile_onto(rng, corners, sizes, (20, 90), (15, 70))
    kind = "constant" if cls == "flat_tie" else _pick(rng, ["smooth", "noise", "constant"])
    imgs, masks = [], []
    for w, h in sizes:
        if kind == "smooth":
            base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3))
            img = np.kron(base, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(0, 12, (h, w, 3))
        elif kind == "noise":
            img = rng.integers(0, 256, (h, w, 3))
        else:
            img = np.broadcast_to(rng.integers(0, 256, 3), (h, w, 3))
        imgs.append(np.clip(img, 0, 255).astype(np.uint8))
        m = np.full((h, w), 255, np.uint8)
        if cls == "holes_heavy":
            m[rng.random((h, w)) < 0.3] = 0
        else:
            for _ in range(int(rng.integers(0, 4))):
                y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
                m[y:y + int(rng.integers(2, 10)), x:x + int(rng.integers(2, 10))] = 0
        masks.append(m)
    if rng.integers(0, 2):
        imgs = [a.astype(np.float32) for a in imgs]
    return dict(cls=cls, kind=kind, corners=corners, sizes=sizes, imgs=imgs, masks=masks, where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)))


def model_graphcut(c):
    """-> (masks after find(), the first overlapping pair (i, j, its graph on the untouched masks) or None); "skip" without scipy."""
    try:
        import scipy.sparse.csgraph  # noqa: F401
    except ImportError:
        return "skip"
    from helpers import graphcut_np
    out = [m.copy() for m in c["masks"]]
    graphcut_np.find(c["imgs"], c["corners"], out)
    n = len(out)
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = overlap_roi(c["corners"][i], c["corners"][j], c["sizes"][i], c["sizes"][j])
            if roi is not None:
                g = graphcut_np.pair_graph(c["imgs"][i], c["imgs"][j], c["masks"][i], c["masks"][j], c["corners"][i], c["corners"][j], roi)
                return out, (i, j, g)
    return out, None


def case_graphcut(rng):
    """isx_graphcut_seam_find against tests/helpers/graphcut_np.py, masks byte for byte; isx_graphcut_seam_find_pair's certificate on the
    first overlapping pair (the masks no earlier pair has touched): a maximum flow and the maximal minimum cut of the model's graph."""
    from helpers import graphcut_np
    c = gen_graphcut(rng)
    want = model_graphcut(c)
    if want == "skip":
        return "skip"
    want, first = want
    imgs = [p[0] for p in _place(c["imgs"], c["where"], c["view_seed"])]
    placed = _place(c["masks"], c["where"], c["view_seed"] + 1)
    G.GraphCutSeamFinder().find(imgs, c["corners"], [p[0] for p in placed])
    for k, (p, w) in enumerate(zip(placed, want)):
        got = _host(p[0])
        assert np.array_equal(got, w), (c["cls"], c["kind"], k, int((got != w).sum()), np.argwhere(got != w)[:3])
    _frame_untouched(placed)
    if first is not None:
        i, j, g = first
        r = G.GraphCutSeamFinder().find_pair(imgs[i], imgs[j], c["corners"][i], c["corners"][j], c["masks"][i].copy(), c["masks"][j].copy(), certificate=True)
        assert (r["rows"], r["cols"]) == g["src"].shape, (r["rows"], r["cols"], g["src"].shape)
        graphcut_np.check_certificate(g, r["flow"], r["residuals"], r["labels"])


# ---- GraphCutSeamFinder(COST_COLOR_GRAD) --------------------------------------------------------------------------------------------------
def _gcg_image(rng, kind, pattern, k, w, h):
    """Tile k of a case: layout()'s blocky texture, noise, a constant, or image k % 2 of a structured pattern at the tile's own size."""
    if kind == "smooth":
        base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3))
        img = np.kron(base, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(0, 12, (h, w, 3))
    elif kind == "noise":
        img = rng.integers(0, 256, (h, w, 3))
    elif kind == "constant":
        img = np.broadcast_to(rng.integers(0, 256, 3), (h, w, 3))
    else:
        from graphcut_patterns import pattern_images
        img = pattern_images(pattern, h, w)[k % 2]
    return np.clip(img, 0, 255).astype(np.float32)


def gen_graphcut_grad(rng):
    """2..3 CV_32FC3 tiles for GraphCutSeamFinder(COST_COLOR_GRAD).  The first two tiles carry the class: a padded grid (roi + 20) as wide as
    1 or 2 of graphcut.hip's BFS tiles +-1 (tile_edge_w) or as high as 2 or 3 of them (tile_edge_h), constant images (flat_tie: every
    weight is 1.0f or one value, all cuts through the overlap tie; half of them the same constant twice), masks with 30 % of their cells
    zero (holes_heavy), layout()'s texture (smooth), noise, or a pattern of tools/graphcut_patterns.py at random sizes and corners
    (structured: constants, ramps, steps, checkerboards, serpentines - ties and the ends of the Q23 range).
    The model's max-flow is a Dinic on Python ints: 0.10 to 0.17 s on a padded grid of 57 x 60 = 3 420 nodes.  So the first pair's grid is
    capped at GCG_MAX_NODES = 4 600 nodes - a roi of at most 48 x 47 when square, 109 x 15 when as wide as two BFS tiles - and a third
    tile, drawn for a third of the cases, is at most 24 x 16 (two more grids of at most 44 x 36).  Measured on a CPU over the seeds
    0..209: 0.07 to 0.13 s of model time a case on average by class, 0.47 s at the worst (a tile_edge_w case of three tiles): below 0.5 s."""
    cls = _pick(rng, GRAPHCUT_GRAD_CLASSES)
    g2 = 2 * SEAM_GAP
    if cls == "tile_edge_w":
        wp = _pick(rng, GC_WIDTHS)
        ow, oh = wp - g2, int(rng.integers(1, max(2, GCG_MAX_NODES // wp - g2 + 1)))
    elif cls == "tile_edge_h":
        hp = _pick(rng, GC_HEIGHTS)
        ow, oh = int(rng.integers(1, GCG_MAX_NODES // hp - g2 + 1)), hp - g2
    else:
        ow = int(rng.integers(1, 90))
        oh = int(rng.integers(1, min(60, GCG_MAX_NODES // (ow + g2) - g2) + 1))
    corners, sizes = _pair_with_overlap(rng, ow, oh)
    if rng.integers(0, 3) == 0:
        _tile_onto(rng, corners, sizes, (4, GCG_THIRD_TILE[0] + 1), (4, GCG_THIRD_TILE[1] + 1))
    kind = {"flat_tie": "constant", "smooth": "smooth", "noise": "noise", "structured": "structured"}.get(cls) or _pick(rng, ["smooth", "noise", "constant", "structured"])
    pattern = None
    if kind == "structured":
        from graphcut_patterns import PATTERNS
        pattern = _pick(rng, list(PATTERNS))
    imgs, masks = [], []
    for k, (w, h) in enumerate(sizes):
        imgs.append(_gcg_image(rng, kind, pattern, k, w, h))
        m = np.full((h, w), 255, np.uint8)
        if cls == "holes_heavy":
            m[rng.random((h, w)) < 0.3] = 0
        else:
            for _ in range(int(rng.integers(0, 4))):
                y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
                m[y:y + int(rng.integers(2, 10)), x:x + int(rng.integers(2, 10))] = 0
        masks.append(m)
    if cls == "flat_tie" and rng.integers(0, 2):
        imgs[1][...] = imgs[0][0, 0]                                    # the same constant twice: every unpenalised weight is exactly 1.0f
    return dict(cls=cls, kind=kind, pattern=pattern, corners=corners, sizes=sizes, imgs=imgs, masks=masks, where=_pick(rng, WHERE),
                view_seed=int(rng.integers(0, 5)))


def model_graphcut_grad(c):
    """-> (masks after find(), the first overlapping pair (i, j, its Q23 graph on the untouched masks) or None); NumPy and Python ints only."""
    from helpers import graphcut_grad_np
    out = [m.copy() for m in c["masks"]]
    graphcut_grad_np.find(c["imgs"], c["corners"], out)
    n = len(out)
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = overlap_roi(c["corners"][i], c["corners"][j], c["sizes"][i], c["sizes"][j])
            if roi is not None:
                g = graphcut_grad_np.pair_graph_grad(c["imgs"][i], c["imgs"][j], c["masks"][i], c["masks"][j], c["corners"][i], c["corners"][j], roi)
                return out, (i, j, g)
    return out, None


def case_graphcut_grad(rng):
    """isx_graphcut_seam_find(COST_COLOR_GRAD) against tests/helpers/graphcut_grad_np.py, masks byte for byte; the 64-bit certificate of
    isx_graphcut_seam_find_pair64 on the first overlapping pair: a maximum flow and the maximal minimum cut of the model's Q23 graph."""
    from helpers import graphcut_np
    c = gen_graphcut_grad(rng)
    want, first = model_graphcut_grad(c)
    note = (c["cls"], c["kind"], c["pattern"], c["where"])
    imgs = [p[0] for p in _place(c["imgs"], c["where"], c["view_seed"])]
    placed = _place(c["masks"], c["where"], c["view_seed"] + 1)
    fdr = G.GraphCutSeamFinder(cost_type=G.seam.COST_COLOR_GRAD)
    fdr.find(imgs, c["corners"], [p[0] for p in placed])
    for k, (p, w) in enumerate(zip(placed, want)):
        got = _host(p[0])
        assert np.array_equal(got, w), note + (k, int((got != w).sum()), np.argwhere(got != w)[:3])
    _frame_untouched(placed)
    if first is not None:
        i, j, g = first
        r = fdr.find_pair(imgs[i], imgs[j], c["corners"][i], c["corners"][j], c["masks"][i].copy(), c["masks"][j].copy(), certificate=True)
        assert (r["rows"], r["cols"]) == g["src"].shape and r["residuals"].dtype == np.int64, note + (r["rows"], r["cols"], g["src"].shape)
        graphcut_np.check_certificate(g, r["flow"], r["residuals"], r["labels"])


# ---- DpSeamFinder(COLOR_GRAD) and isx_seam_gradients ----------------------------------------------------------------------------------------
def gen_seam_grad(rng):
    """Two halves.  About a third of the cases: seam_gradients on a rectangle of a CV_8UC3 / CV_32FC3 image - any rectangle, one as wide /
    high as 1 or 2 of seam.hip's gradient tiles +-1, one pixel, or one on the image's border (where the Sobel taps reflect).  The others
    (cls "find"): DpSeamFinder(COLOR_GRAD).find on the 2..3 tiles of tests/seam_cases.py's make_find_case, as case_find draws them."""
    half = "find" if rng.random() < 0.65 else "grad"
    u8 = bool(rng.integers(0, 2))
    if half == "find":
        from seam_cases import make_find_case
        images, corners, masks = make_find_case(int(rng.integers(0, 1 << 30)), int(rng.integers(2, 4)), u8, holes=bool(rng.integers(0, 2)),
                                                size=(int(rng.integers(20, 110)), int(rng.integers(30, 150))))
        return dict(cls="find", imgs=images, corners=corners, masks=masks, where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)))
    cls = _pick(rng, SEAM_GRAD_CLASSES[:4])
    rw, rh = int(rng.integers(1, 140)), int(rng.integers(1, 100))
    if cls == "tile_edge":
        if rng.integers(0, 2):
            rw = _pick(rng, GRAD_WIDTHS)
        else:
            rh = _pick(rng, GRAD_HEIGHTS)
    elif cls == "one_pixel":
        rw = rh = 1
    left, right, top, bottom = (int(v) for v in rng.integers(0, 12, 4))
    if cls == "rect_at_border":
        side = int(rng.integers(0, 5))                                  # one side, or (4) all four: the whole image
        left, right, top, bottom = (0 if side in (k, 4) else v for k, v in enumerate((left, right, top, bottom)))
    w, h = left + rw + right, top + rh + bottom
    if u8:
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    else:
        img = (rng.random((h, w, 3), dtype=np.float32) * np.float32(255))
    return dict(cls=cls, img=img, rect=(left, top, rw, rh), where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)))


def model_seam_grad(c):
    from helpers import dpseam_grad_np as M
    if c["cls"] == "find":
        out = [m.copy() for m in c["masks"]]
        M.DpSeamFinder(M.COLOR_GRAD).find(c["imgs"], c["corners"], out)
        return out
    gx, gy = M.gradients(c["img"])
    x, y, w, h = c["rect"]
    return np.abs(gx)[y:y + h, x:x + w], np.abs(gy)[y:y + h, x:x + w]


def case_seam_grad(rng):
    """isx_seam_gradients and isx_dp_seam_find_cost(COLOR_GRAD) against tests/helpers/dpseam_grad_np.py, bit for bit."""
    c = gen_seam_grad(rng)
    want = model_seam_grad(c)
    if c["cls"] == "find":
        imgs = [p[0] for p in _place(c["imgs"], c["where"], c["view_seed"])]
        placed = _place(c["masks"], c["where"], c["view_seed"] + 1)
        G.DpSeamFinder(G.DP_COLOR_GRAD).find(imgs, c["corners"], [p[0] for p in placed])
        for k, (p, b) in enumerate(zip(placed, want)):
            assert np.array_equal(_host(p[0]), b), (c["where"], k, np.argwhere(_host(p[0]) != b)[:3])
        _frame_untouched(placed)
        return None
    img = _place([c["img"]], c["where"], c["view_seed"])[0][0]
    gx, gy = G.seam_gradients(img, c["rect"])
    for name, a, b in (("gradx", _host(gx), want[0]), ("grady", _host(gy), want[1])):
        assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), \
            (name, c["cls"], c["rect"], np.argwhere(a != b)[:3])


# ---- BlocksGainCompensator ------------------------------------------------------------------------------------------------------------------
def _bg_counts(sizes, blw, blh):
    return sum(-(-w // blw) * -(-h // blh) for w, h in sizes)


def _bg_fit(sizes, blw, blh):
    """The block size grown (the axis with more blocks first) until the tiles hold at most BG_MAX_UNKNOWNS blocks."""
    while _bg_counts(sizes, blw, blh) > BG_MAX_UNKNOWNS:
        if max(-(-w // blw) for w, _ in sizes) >= max(-(-h // blh) for _, h in sizes):
            blw += 1 + blw // 4
        else:
            blh += 1 + blh // 4
    return blw, blh


def bg_bands(width, height, item_size):
    """The heights of the bands a record of width x height is cut into: max(1, item_size / width) rows each, the last one what is left."""
    band = max(1, item_size // width)
    return [min(band, height - y) for y in range(0, height, band)]


def bg_record_items(corners, sizes, bl_width, bl_height, diag_bytes, pair_pixels):
    """(diag, pairs): per block (width, height, band heights), and the same per pair of blocks of different images whose rectangles meet, by
    block_i, then block_j - all pairs against all, on Python integers."""
    from helpers import blocks_gain_np
    rects, owner = [], []
    for k, ((cx, cy), (w, h)) in enumerate(zip(corners, sizes)):
        for x, y, bw, bh in blocks_gain_np.block_rects(w, h, bl_width, bl_height):
            rects.append((cx + x, cy + y, bw, bh)); owner.append(k)
    diag = [(w, h, bg_bands(w, h, diag_bytes)) for _, _, w, h in rects]
    pairs = []
    for i, (xi, yi, wi, hi) in enumerate(rects):
        for j in range(i + 1, len(rects)):
            xj, yj, wj, hj = rects[j]
            w, h = min(xi + wi, xj + wj) - max(xi, xj), min(yi + hi, yj + hj) - max(yi, yj)
            if owner[i] != owner[j] and w > 0 and h > 0:
                pairs.append((w, h, bg_bands(w, h, pair_pixels)))
    return diag, pairs


def bg_forward_error_rtol(A, b, gains):
    """(rtol, measured): rtol = min(1e-9, 4 max(measured, B 2^-52 cond_1(A))) with `measured` the largest relative difference between
    np.linalg.solve (gains) and the NumPy hal::LU on the B x B system - the textbook forward-error scale of a backward-stable solve, from the
    model alone.  Where the two CPU solves agree to the last bit (measured = 0) the device, whose back substitution adds in another order, is
    still owed the rounding of its own operations."""
    from helpers import blocks_gain_np
    x, _ = blocks_gain_np.hal_lu_solve(A, b)
    measured = float(np.max(np.abs(x - gains) / np.abs(gains)))
    bound = len(b) * 2.0 ** -52 * float(np.linalg.cond(A, 1))
    return min(1e-9, 4 * max(measured, bound)), measured


def gen_blocks_gain(rng):
    """1..4 tiles under masks of 0 / 254 / 255, a block size, and one or two images to apply the maps to (of a fed size or not).  The class
    says what the case reaches: records of several work items of gain.hip, a pair of blocks whose band is one row about GF_PAIR_PIXELS
    wide, one-pixel blocks (the maps have the images' sizes), no pair of blocks that meet, one shared pixel, or an applied image on the
    edges of k_blocks_gain_apply's workgroup.  At most BG_MAX_UNKNOWNS blocks."""
    cls = _pick(rng, BLOCKS_GAIN_CLASSES + ["plain", "several_items"])      # (the two that carry the most arithmetic: twice as likely)
    x0, y0 = int(rng.integers(-40, 40)), int(rng.integers(-30, 30))
    blw, blh = int(rng.integers(6, 65)), int(rng.integers(6, 65))
    if cls == "several_items":
        blw, blh = int(rng.integers(96, 257)), int(rng.integers(96, 257))
        while True:                                                      # (large tiles that overlap widely: most draws do at once)
            sizes = [(int(rng.integers(130, 400)), int(rng.integers(130, 300))) for _ in range(int(rng.integers(2, 4)))]
            corners = [(x0 + int(rng.integers(-30, 60)) * k, y0 + int(rng.integers(-20, 40)) * k) for k in range(len(sizes))]
            diag, pairs = bg_record_items(corners, sizes, blw, blh, _GF["GF_DIAG_BYTES"], _GF["GF_PAIR_PIXELS"])
            if any(len(b) >= 2 for _, _, b in diag + pairs):
                break
    elif cls == "wide_row":
        corners, sizes = _pair_with_overlap(rng, _pick(rng, BG_WIDE_ROWS), int(rng.integers(1, 5)))
        blw, blh = max(w for w, _ in sizes) + int(rng.integers(0, 100)), int(rng.integers(1, 33))
    elif cls == "one_pixel_blocks":
        blw = blh = 1
        corners, sizes = [(x0, y0)], [(int(rng.integers(1, 11)), int(rng.integers(1, 9)))]
        for _ in range(int(rng.integers(1, 3))):
            _tile_onto(rng, corners, sizes, (1, 11), (1, 9))
    elif cls == "no_pairs":
        corners, sizes = [], []
        for k in range(int(rng.integers(1, 4))):                         # left to right, a gap of 0 (they touch and do not meet) or more
            sizes.append((int(rng.integers(8, 160)), int(rng.integers(6, 120))))
            corners.append((x0, y0 + int(rng.integers(-5, 6))))
            x0 += sizes[-1][0] + int(rng.integers(0, 3))
    elif cls == "one_pixel_meeting":
        sizes = [(int(rng.integers(8, 160)), int(rng.integers(6, 120))) for _ in range(2)]
        corners = [(x0, y0), (x0 + sizes[0][0] - 1, y0 + sizes[0][1] - 1)]
    else:
        corners, sizes = [(x0, y0)], [(int(rng.integers(8, 160)), int(rng.integers(6, 120)))]
        if cls == "apply_edges":                                         # any block shape: a map of more rows or columns than the applied image too
            blw, blh = int(rng.integers(1, 65)), int(rng.integers(1, 65))
            sizes = [(int(rng.integers(8, 80)), int(rng.integers(6, 60)))]
        for _ in range(int(rng.integers(1, 4))):
            _tile_onto(rng, corners, sizes, (8, 80) if cls == "apply_edges" else (8, 160), (6, 60) if cls == "apply_edges" else (6, 120))
    blw, blh = _bg_fit(sizes, blw, blh)
    imgs, masks = [], []
    for w, h in sizes:
        imgs.append(rng.integers(int(rng.integers(0, 80)), int(rng.integers(120, 257)), (h, w, 3), dtype=np.uint8))
        masks.append(rng.choice(np.array([0, 254, 255, 255, 255, 255], np.uint8), size=(h, w)))
    if cls == "one_pixel_meeting":                                      # the shared pixel counts on both sides
        masks[0][-1, -1] = masks[1][0, 0] = 255
    apply = []
    for k in range(int(rng.integers(1, 3))):
        index = int(rng.integers(0, len(sizes)))
        w, h = sizes[index]
        if cls == "apply_edges":
            while (w, h) == sizes[index]:
                edge = int(rng.integers(0, 3))                           # the width, the height, or both on an edge
                w = _pick(rng, BG_APPLY_WIDTHS) if edge != 1 else int(rng.integers(1, 600))
                h = _pick(rng, BG_APPLY_HEIGHTS) if edge != 0 else int(rng.integers(1, 60))
        elif (k == 1 or rng.integers(0, 2)) and w * h < (1 << 17):
            w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))
        apply.append((index, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
    return dict(cls=cls, corners=corners, sizes=sizes, imgs=imgs, masks=masks, blocks=(blw, blh), apply=apply, where=_pick(rng, WHERE),
                view_seed=int(rng.integers(0, 5)))


def model_blocks_gain(c):
    from helpers import blocks_gain_np
    m = blocks_gain_np.feed_blocks_model(c["corners"], c["imgs"], c["masks"], *c["blocks"])
    rtol, measured = bg_forward_error_rtol(m["A"], m["b"], m["gains"])
    return dict(counts=m["counts"], diag_n=m["diag_n"], pairs=m["pairs"], gains=m["gains"], rtol=rtol, measured=measured)


def case_blocks_gain(rng):
    """isx_blocks_gain_feed / _map / _apply against tests/helpers/blocks_gain_np.py: the block counts, N exactly, I bit for bit, the gains
    to bg_forward_error_rtol (from the model alone), the maps bit for bit the model's smoothing of the
    library's gains, apply bit for bit in place; nothing written around a view, nor into a fed one."""
    from helpers import blocks_gain_np
    import torch
    c = gen_blocks_gain(rng)
    want = model_blocks_gain(c)
    fed = _place(c["imgs"], c["where"], c["view_seed"]) + _place(c["masks"], c["where"], c["view_seed"] + 1)
    n = len(c["imgs"])
    comp = G.BlocksGainCompensator(*c["blocks"]).feed(c["corners"], [p[0] for p in fed[:n]], [p[0] for p in fed[n:]])
    assert comp.block_counts() == want["counts"], (c["cls"], comp.block_counts(), want["counts"])
    pairs, diag = comp.block_stats()
    assert np.array_equal(diag, want["diag_n"]), (c["cls"], diag, want["diag_n"])
    assert [(int(p["block_i"]), int(p["block_j"]), int(p["n"])) for p in pairs] == [p[:3] for p in want["pairs"]], c["cls"]
    for k, field in ((3, "i_ij"), (4, "i_ji")):
        assert np.array_equal(pairs[field].view(np.uint64), np.array([p[k] for p in want["pairs"]], np.float64).view(np.uint64)), (c["cls"], field)
    g = comp.gains()
    np.testing.assert_allclose(g, want["gains"], rtol=want["rtol"], atol=0)
    maps = comp.gain_maps()
    for got, m in zip(maps, blocks_gain_np.maps_from_gains(g, want["counts"])):
        assert got.dtype == np.float32 and got.shape == m.shape and np.array_equal(got.view(np.uint32), m.view(np.uint32)), c["cls"]
    for p, a in zip(fed, c["imgs"] + c["masks"]):
        assert np.array_equal(_host(p[0]), a), (c["cls"], "feed wrote a mat")
    _frame_untouched(fed)
    for k, (index, img) in enumerate(c["apply"]):
        placed = _place([img], c["where"], c["view_seed"] + 2 + k)
        comp.apply(index, c["corners"][index], placed[0][0])
        torch.cuda.synchronize()
        w = blocks_gain_np.apply_model(img, maps[index])
        got = _host(placed[0][0])
        assert np.array_equal(got, w), (c["cls"], index, img.shape, maps[index].shape, np.argwhere(got != w)[:3])
        _frame_untouched(placed)


# ---- cv::resize and the scaled mask stage ---------------------------------------------------------------------------------------------------
def rz_float_specials(rng, shape):
    """Finite floats only: noise with patches and single values of +-0.0, +-1e-40, +-1.4e-45, +-FLT_MAX and +-1.0 (denormals in and out,
    signed zeros, and - under the area rule - sums that overflow)."""
    kinds = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3.4028235e38, -3.4028235e38, 1.0, -1.0], np.float32)
    a = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)
    for _ in range(shape[0] * shape[1] // 6 + 1):
        y, x = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))
        a[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 5))] = kinds[int(rng.integers(0, len(kinds)))]
    single = rng.random(shape) < 0.1
    a[single] = kinds[rng.integers(0, len(kinds), shape)][single]
    a.flat[:len(kinds)] = kinds[:a.size]                               # (every kind, where the mat has room)
    return a


def rz_byte_pattern(rng, shape):
    """0 / 255 only: constant, a one-pixel checkerboard, one-pixel stripes either way, or sparse 255s"""
    y, x = np.indices(shape[:2])
    kind = int(rng.integers(0, 6))
    p = [np.zeros(shape[:2], np.int64), np.full(shape[:2], 255), ((x + y) & 1) * 255, (x & 1) * 255, (y & 1) * 255, (rng.random(shape[:2]) < 0.1) * 255][kind]
    return np.broadcast_to(p.reshape(p.shape + (1,) * (len(shape) - 2)), shape).astype(np.uint8)


def gen_resize(rng):
    """One source of a type of RZ_TYPES and a destination size, both within RZ_MAX_SHAPE; the class names what the pair reaches: a
    destination as wide as 1 or 2 waves +-1 or as high as 1 or 2 workgroups +-1 of either kernel, the area rule (both ratios exactly 2) or one
    ratio of 2 alone, a source of 1..3 rows or columns, a ratio of 6..12 in a direction drawn per axis, or special values.  A CV_8UC1 case also
    carries the mask stage on the same pair of sizes: an element, and a warped mask that is absent, given, or the output itself."""
    cls = _pick(rng, RESIZE_CLASSES)
    dtype, cn = _pick(rng, RZ_TYPES)
    sh, sw = int(rng.integers(1, 121)), int(rng.integers(1, 201))
    dh, dw = int(rng.integers(1, 151)), int(rng.integers(1, 301))
    if cls == "wave_edge":
        dw, dh = _pick(rng, RZ_WAVE_WIDTHS), int(rng.integers(1, 41))
    elif cls == "rows_edge":
        dh = _pick(rng, RZ_ROW_HEIGHTS)
    elif cls == "half":
        dh, dw = int(rng.integers(1, 81)), int(rng.integers(1, 251))
        sh, sw = 2 * dh, 2 * dw
    elif cls == "half_one_axis":
        if rng.integers(0, 2):
            sw = 2 * dw
            sh += sh == 2 * dh
        else:
            sh = 2 * dh
            sw += sw == 2 * dw
    elif cls == "tiny_src":
        axis = int(rng.integers(0, 3))                                  # rows, columns or both
        sh = int(rng.integers(1, 4)) if axis != 1 else sh
        sw = int(rng.integers(1, 4)) if axis != 0 else sw
    elif cls == "steep":
        small = int(rng.integers(1, RZ_MAX_SHAPE[0] // 12 + 1)), int(rng.integers(1, RZ_MAX_SHAPE[1] // 12 + 1))
        big = tuple(int(rng.integers(6 * n, 12 * n + 1)) for n in small)
        (sh, dh) = (small[0], big[0]) if rng.integers(0, 2) else (big[0], small[0])
        (sw, dw) = (small[1], big[1]) if rng.integers(0, 2) else (big[1], small[1])
    shape = (sh, sw, cn) if cn > 1 else (sh, sw)
    if dtype == "uint8":
        sparse = cls != "specials" and cn == 1 and bool(rng.integers(0, 2))             # a seam mask: 0 / 255 blobs with a few other values
        if cls == "specials":
            src = rz_byte_pattern(rng, shape)
        elif sparse:
            src = np.where(rng.random(shape) < 0.06, 255, 0).astype(np.uint8)
            few = rng.random(shape) < 0.02
            src[few] = rng.integers(1, 255, shape, dtype=np.uint8)[few]
        else:
            src = rng.integers(0, 256, shape, dtype=np.uint8)
    elif cls == "specials":
        src = rz_float_specials(rng, shape)
    else:                                                                # either sign, magnitudes up to 1e6: a fused multiply-add would round differently
        src = (rng.standard_normal(shape) * 10.0 ** rng.uniform(0, 6, shape)).astype(np.float32)
    stage = None
    if (dtype, cn) == ("uint8", 1):
        warped = np.where(rng.random((dh, dw)) < 0.7, 255, 0).astype(np.uint8)
        warped[rng.random((dh, dw)) < 0.1] = 0x5a
        stage = dict(element=_pick(rng, RZ_ELEMENTS), mode=_pick(rng, RZ_STAGE_MODES), warped=warped)
    return dict(cls=cls, src=src, dsize=(dw, dh), interp=int(rng.integers(0, 2)), stage=stage, where=_pick(rng, WHERE), view_seed=int(rng.integers(0, 5)))


def model_resize(c):
    from helpers import resize_np
    want = dict(out=resize_np.resize(c["src"], c["dsize"], c["interp"]), stage=None)
    if c["stage"] is not None:
        st = c["stage"]
        want["stage"] = resize_np.dilate_resize_and(c["src"], None if st["mode"] == "no_warped" else st["warped"], st["element"][0], st["element"][1], c["dsize"])
    return want


def _same_bits(got, want):
    """bit for bit, but for NaNs: those by position"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if want.dtype != np.float32:
        return np.array_equal(got, want)
    ok = ~np.isnan(want)
    return np.array_equal(np.isnan(got), ~ok) and np.array_equal(np.ascontiguousarray(got).view(np.uint32)[ok], np.ascontiguousarray(want).view(np.uint32)[ok])


def case_resize(rng):
    """isx_resize and, on CV_8UC1, isx_mask_dilate_resize_and against tests/helpers/resize_np.py, bit for bit; the inputs keep their bytes and
    nothing is written around a view."""
    c = gen_resize(rng)
    want = model_resize(c)
    src, dsize = c["src"], c["dsize"]
    dshape = (dsize[1], dsize[0]) + src.shape[2:]
    ps = _place([src], c["where"], c["view_seed"])
    pd = _place([np.zeros(dshape, src.dtype)], c["where"], c["view_seed"] + 1)
    G.resize(ps[0][0], dsize, interpolation=c["interp"], dst=pd[0][0])
    got = _host(pd[0][0])
    note = (c["cls"], str(src.dtype), src.shape, dsize, c["interp"], c["where"])
    assert _same_bits(got, want["out"]), note + (np.argwhere(got != want["out"])[:3],)
    assert _same_bits(_host(ps[0][0]), src), note + ("resize wrote its source",)
    _frame_untouched(ps + pd)
    if c["stage"] is None:
        return None
    st = c["stage"]
    (kw, kh), mode = st["element"], st["mode"]
    pw = _place([st["warped"]], c["where"], c["view_seed"] + 2)
    po = pw if mode == "in_place" else _place([np.zeros(dshape, np.uint8)], c["where"], c["view_seed"] + 3)
    if mode == "no_warped":
        G.dilate_resize_and(ps[0][0], dsize, kw, kh, out=po[0][0])
    else:
        G.dilate_resize_and(ps[0][0], pw[0][0], kw, kh, out=po[0][0])
    got = _host(po[0][0])
    note += ((kw, kh), mode)
    assert np.array_equal(got, want["stage"]), note + (int((got != want["stage"]).sum()), np.argwhere(got != want["stage"])[:3])
    assert np.array_equal(_host(ps[0][0]), src), note + ("the stage wrote its seam mask",)
    if mode != "in_place":
        assert np.array_equal(_host(pw[0][0]), st["warped"]), note + ("the stage wrote its warped mask",)
    _frame_untouched(ps + pw + (po if po is not pw else []))


# ---- the planned warp's ROI verification against tests/helpers/plan_verify_np.py ----------------------------------------------------------
PLAN_VERIFY_CLASSES = ["cyl_light", "cyl_corner_behind", "cyl_pole", "cyl_rolled", "sph_plain", "sph_north", "sph_south", "cyl_straddle",
                       "sph_straddle", "on_seam", "sph_pole_edge", "zero_bound"]
PV_SIZES = [(256, 128), (257, 129), (33, 33), (129, 46), (179, 150), (64, 48), (100, 75), (48, 64), (320, 200)]
PV_MAX_EXTREMUM = 1.0e6       # a cylindrical v beyond this (a pixel on the cylinder's axis): skipped


def _pv_rotation(yaw, pitch, roll):
    """Ry(yaw) Rx(pitch) Rz(roll) in float32 (rot() above with the angles given)"""
    a, b, c = pitch, yaw, roll
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return (Ry @ Rx @ Rz).astype(np.float32)


def _pv_draw(rng, cls):
    w, h = _pick(rng, PV_SIZES)
    wide = cls in ("cyl_pole", "cyl_corner_behind")
    f = float(np.round((rng.uniform(0.3, 0.8) if wide else rng.uniform(0.4, 2.0)) * max(w, h), 1))
    scale = float(np.float32(np.round(f * rng.uniform(0.5, 2.0), 1)))
    cx, cy = float(np.round(w / 2 + rng.uniform(-3, 3), 1)), float(np.round(h / 2 + rng.uniform(-3, 3), 1))
    kind = 0 if cls.startswith("cyl") else 1 if cls.startswith("sph") else int(rng.integers(0, 2))
    yaw, pitch, roll = rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2)
    if cls.endswith("_straddle"):
        yaw = np.pi + rng.uniform(-0.3, 0.3)
    elif cls == "sph_north":
        pitch = -np.pi / 2 + rng.uniform(-0.3, 0.3)
    elif cls == "sph_south":
        pitch = np.pi / 2 + rng.uniform(-0.3, 0.3)
    elif cls == "cyl_pole":
        # the cylinder's axis projects to (cx, cy - f / tan(pitch)) when yaw = roll = 0; the line z_ = 0 through it is then horizontal and
        # misses the image: a pole 0.3 to 1.9 px above the first row or below the last one
        py = -rng.uniform(0.3, 1.9) if rng.random() < 0.5 else h - 1 + rng.uniform(0.3, 1.9)
        yaw, roll, pitch = 0.0, 0.0, float(np.arctan(-f / (py - cy)))
    elif cls == "cyl_corner_behind":
        yaw = _pick(rng, [-1, 1]) * rng.uniform(0.9, 1.5)
    elif cls == "cyl_rolled":
        roll = _pick(rng, [-1, 1]) * rng.uniform(1.65, 2.8)
    elif cls == "on_seam":            # a pixel exactly on the back seam: yaw = pi, no roll, the principal point on a column
        yaw, roll, cx = float(np.pi), 0.0, float(np.round(cx))
    elif cls == "sph_pole_edge":      # a pole of the sphere inside the image, within 0.8 px of its first or last row (see cyl_pole)
        kind, yaw, roll = 1, float(rng.uniform(-3.0, 3.0)), 0.0
        if rng.random() < 0.5:
            pitch = float(-np.arctan(f / (h - 1 + rng.uniform(-0.8, 0.8) - cy)))              # north, beside the last row
        else:
            pitch = float(np.pi - np.arctan(f / (cy - rng.uniform(0.05, 0.8))))               # south, beside the first row
    elif cls == "zero_bound":
        yaw = pitch = roll = 0.0
        if rng.random() < 0.5:
            cx = float(np.round(rng.uniform(-0.6, 0.6), 1))
        else:
            cy = float(np.round(rng.uniform(-0.6, 0.6), 1))
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float32)
    return dict(cls=cls, kind=kind, w=w, h=h, scale=scale, K=K, R=_pv_rotation(yaw, pitch, roll), yaw=float(yaw))


def pv_is_of_class(c):
    """Is the drawn camera what its class names?  (what gen_plan_verify redraws on, and what tests/test_fuzz_generators.py checks again)"""
    from helpers import plan_verify_np as PV
    cls = c["cls"]
    scan, why = PV.scan_kind(c["kind"], c["K"], c["R"], O.camera(c["K"], c["R"])[2], c["w"], c["h"])
    north, south = PV.sph_poles(c["K"], c["R"], c["w"], c["h"])
    if cls == "cyl_light":
        return scan == "roi_border"
    if cls in ("cyl_corner_behind", "cyl_pole", "cyl_rolled"):
        return (scan, why) == ("roi_scan", {"cyl_corner_behind": "corner_behind", "cyl_pole": "cyl_pole", "cyl_rolled": "rolled"}[cls])
    if cls == "sph_plain":
        return not north and not south
    if cls in ("sph_north", "sph_south"):
        return (north, south) == (cls == "sph_north", cls == "sph_south")
    if cls.endswith("_straddle"):
        return abs(c["yaw"] - np.pi) <= 0.3 and not north and not south
    if cls == "on_seam":
        return c["yaw"] == float(np.pi) and float(c["K"][0, 2]).is_integer() and c["R"][1, 0] == 0 and not north and not south
    if cls == "sph_pole_edge":
        return c["kind"] == 1 and north != south
    return np.array_equal(c["R"], np.eye(3, dtype=np.float32))       # zero_bound


def gen_plan_verify(rng):
    """A camera of one of PLAN_VERIFY_CLASSES (redrawn until it is of its class) and a plan: the true one (shift None) or the true one with one
    bound moved by +-1 (mostly) or by up to +-40."""
    cls = _pick(rng, PLAN_VERIFY_CLASSES)
    for _ in range(200):
        c = _pv_draw(rng, cls)
        if pv_is_of_class(c):
            break
    else:
        raise AssertionError("no camera of class " + cls)
    c["shift"] = None
    if rng.random() < 0.7:
        c["shift"] = (int(rng.integers(0, 4)), int(_pick(rng, [-1, 1])) * (1 if rng.random() < 0.8 else int(rng.integers(2, 41))))
    return c


def model_plan_verify(c):
    """-> dict(roi, plan, verdict, per, extrema) or "skip" (an extremum that is not finite or beyond PV_MAX_EXTREMUM)"""
    from helpers import plan_verify_np as PV
    t = PV.truth(O, c["kind"], c["scale"], c["K"], c["R"], c["w"], c["h"])
    if not all(np.isfinite(e) and abs(e) < PV_MAX_EXTREMUM for e in t["extrema"]):
        return "skip"
    plan = list(t["roi"]) if c["shift"] is None else PV.shifted(t["roi"], *c["shift"])
    verdict, per = PV.verdict(c["kind"], c["scale"], plan, t["extrema"], t["north"], t["south"])
    return dict(roi=t["roi"], plan=plan, verdict=verdict, per=per, extrema=t["extrema"])


def case_plan_verify(rng):
    """isx_warper_queue_verify -> isx_warper_verify -> isx_warper_plan_status on a fresh handle against the three-valued model: the count is
    0 where the model says MUST_PASS, 1 where it says MUST_FLAG, either where it makes no claim."""
    import ctypes as C
    c = gen_plan_verify(rng)
    want = model_plan_verify(c)
    if want == "skip":
        return "skip"
    w = (G.CylindricalWarper() if c["kind"] == 0 else G.SphericalWarper()).create(c["scale"])
    w.queue_verify((c["w"], c["h"]), c["K"], c["R"], want["plan"])
    w.verify()
    n = C.c_int(-1)
    rc = w._lib.isx_warper_plan_status(w._h, C.byref(n))
    note = (c["cls"], c["kind"], (c["w"], c["h"]), c["scale"], c["K"].tolist(), c["R"].tolist(), c["shift"], want)
    assert rc in (0, 8) and (rc == 8) == (n.value != 0) and n.value in (0, 1), (rc, n.value) + note
    if want["verdict"] == "must_pass":
        assert n.value == 0, note
    if want["verdict"] == "must_flag":
        assert n.value == 1, note
    return None


NEW_FAMILIES = ["case_plane_warp","case_gain_feed", "case_voronoi", "case_graphcut", "case_seam_grad"]


CASES = [case_warp, case_blend, case_feather, case_prep, case_seam, case_blend_float_and_many, case_pipeline, case_find, case_warp_fused,
         case_linear_pair, case_strip, case_strip_feather, case_batch, case_s16_tiles, case_round4_calls, case_many_tiles, case_fused_feed, case_round6_calls,
         case_long_lived, case_plane_warp, case_gain_feed, case_voronoi, case_graphcut, case_seam_grad, case_blocks_gain, case_resize, case_graphcut_grad,
         case_plan_verify]


def run(budget, seed0, verbose=True, progress_path=None, only=None):
    """Round-robin over the case families for `budget` seconds; case n uses seed seed0 * 1000003 + n.  Returns the summary dict.
    only: a list of family names to run (a soak or a slice of what a change touched); None takes the comma-separated ISX_FUZZ_ONLY, or all.
    progress_path: the summary so far is written there every two minutes ("partial": true), so that a soak the GPU box's time limit cuts
    short still leaves its count behind (round 6 lost an hour-long one that way)."""
    G.load()
    t0, n, bad, skipped = time.time(), 0, 0, 0
    if only is None:
        only = [k for k in os.environ.get("ISX_FUZZ_ONLY", "").split(",") if k]
    unknown = sorted(set(only) - {f.__name__ for f in globals()["CASES"]})
    if unknown:
        raise ValueError("no such fuzz family: " + ", ".join(unknown))
    CASES = [f for f in globals()["CASES"] if not only or f.__name__ in only]
    counts = {f.__name__: 0 for f in CASES}
    fails = {f.__name__: 0 for f in CASES}
    failing_seeds = []
    stop_at_first = os.environ.get("ISX_FUZZ_STOP_AT_FIRST", "") not in ("", "0")
    def summary(partial):
        d = {"cases": n, "seconds": round(time.time() - t0, 1), "seed": seed0, "mismatches": bad, "skipped_geometries": int(skipped),
             "per_family": {k: {"cases": counts[k], "mismatches": fails[k]} for k in counts}, "failing_seeds": failing_seeds[:50]}
        if partial:
            d["partial"] = True
        return d
    last_dump = t0
    while time.time() - t0 < budget:
        if progress_path and time.time() - last_dump > 120.0:
            import json
            with open(progress_path, "w") as f:
                json.dump(summary(True), f, indent=1)
            last_dump = time.time()
        fn = CASES[n % len(CASES)]
        seed = seed0 * 1000003 + n
        try:
            r = fn(np.random.default_rng(seed))
            skipped += r == "skip"
            counts[fn.__name__] += 1
        except AssertionError:
            bad += 1; fails[fn.__name__] += 1; failing_seeds.append([fn.__name__, seed])
            if verbose:
                print("FAIL", fn.__name__, "seed", seed)
                traceback.print_exc(limit=2)
        except Exception as e:   # geometry the reference itself rejects must be rejected the same way on both sides
            try:
                code = getattr(e, "code", None)
            except Exception:
                code = None
            if verbose:
                print("EXC ", fn.__name__, "seed", seed, type(e).__name__, code, str(e)[:120])
            bad += 1; fails[fn.__name__] += 1; failing_seeds.append([fn.__name__, seed])
        n += 1
        if bad and stop_at_first:
            break
    return summary(False)


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    out = run(budget, seed0, progress_path=sys.argv[3] if len(sys.argv) > 3 else None)
    print("cases", out["cases"], {k: v["cases"] for k, v in out["per_family"].items()}, "skipped", out["skipped_geometries"],
          "failures", out["mismatches"], "in %.0f s" % out["seconds"])
    if len(sys.argv) > 3:
        import json
        import subprocess
        try:
            out["git_head"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            pass
        try:
            import torch
            out["device"] = torch.cuda.get_device_name(0)
        except Exception:
            pass
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)
    return out["mismatches"]


if __name__ == "__main__":
    sys.exit(min(main(), 100))
