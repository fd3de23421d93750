"""The plane projector (cv::detail::PlaneWarper, with translation) on the GPU against the NumPy model tests/helpers/plane_np.py: every
entry a warper handle has, bit for bit (np.array_equal, no tolerance) - random rigs with yaw / pitch / roll up to +-0.5 rad, T zero and
non-zero, 3 x 3 to 4K sources, odd widths, host / device / pitched / byte-unaligned mats, planned warps and their verification, batches,
CV_16SC3 tiles, the gain and column-range switches, a bounding box that reaches z <= 0, the pair pipeline eager and captured, threads."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import plane_np as P  # noqa: E402

from imagestitch_amd import synth  # noqa: E402
from imagestitch_amd._lib import as_mat, check, f9  # noqa: E402

pytestmark = pytest.mark.gpu

CYL, SPH, PLANE = 0, 1, 2
NEAREST, LINEAR = 0, 1
CONST, REPL, REFLECT, REFLECT101 = 0, 1, 2, 4
I16, F32 = 0, 1


def _rot(yaw, pitch, roll):
    return (synth._rot("y", yaw) @ synth._rot("x", pitch) @ synth._rot("z", roll)).astype(np.float32)


def _rig(rng, w, h, with_t, amp=0.5):
    f = float(rng.uniform(0.9, 2.0) * max(w, h))
    K = np.array([[f, 0, w / 2 + rng.uniform(-3, 3)], [0, f * rng.uniform(0.95, 1.05), h / 2 + rng.uniform(-3, 3)], [0, 0, 1]], np.float32)
    R = _rot(*rng.uniform(-amp, amp, 3))
    T = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)], np.float32) if with_t else None
    return float(f * rng.uniform(0.7, 1.3)), K, R, T


def _img(rng, h, w, cn=3, dtype=np.uint8):
    a = rng.integers(0, 256, (h, w, cn) if cn > 1 else (h, w)).astype(np.uint8)
    return a if dtype == np.uint8 else a.astype(np.float32) * np.float32(1.37)


def _warper(gpu, scale, T=None):
    w = gpu.PlaneWarper().create(scale)
    if T is not None:
        w.set_translation(T)
    return w


def _model_tile(oracle, scale, K, R, T, img, roi=None):
    """(roi, warped image LINEAR / REFLECT, warped all-255 mask NEAREST / CONSTANT) by the model."""
    m = P.from_rig(oracle, scale, K, R, T)
    _, wi, roi = m.warp(img, LINEAR, REFLECT, roi)
    _, wm, _ = m.warp(np.full(img.shape[:2], 255, np.uint8), NEAREST, CONST, roi)
    return tuple(int(v) for v in roi), wi, wm


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


SIZES = [(3, 3), (17, 9), (333, 217), (641, 359)]


@pytest.mark.parametrize("with_t", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_every_warp_entry_equals_the_model(gpu, oracle, size, with_t):
    import torch
    w, h = size
    rng = np.random.default_rng(1000 + w + int(with_t))
    for _ in range(2):
        scale, K, R, T = _rig(rng, w, h, with_t)
        m = P.from_rig(oracle, scale, K, R, T)
        warper = _warper(gpu, scale, T)
        roi, mm = warper.warpRoi((w, h), K, R, with_minmax=True)
        mroi, mmm = m.detect_roi(w, h)
        assert roi == tuple(mroi) and np.array_equal(mm, mmm), (roi, mroi)
        # buildMaps, host and device mats
        xm, ym = m.build_maps(mroi)
        r2, gx, gy = warper.buildMaps((w, h), K, R)
        assert r2 == roi and np.array_equal(gx, xm) and np.array_equal(gy, ym)
        like = torch.empty(1, device="cuda")
        dx, dy = warper.buildMapsRoi(K, R, roi, like=like)
        assert np.array_equal(dx.cpu().numpy(), xm) and np.array_equal(dy.cpu().numpy(), ym)
        # warp(): u8x3 / u8x1 / f32x3 / f32x1, the reference's two calls (tile kernels) and the generic kernel's combinations
        for cn, dtype, combos in ((3, np.uint8, [(LINEAR, REFLECT), (LINEAR, CONST), (NEAREST, REFLECT101)]),
                                  (1, np.uint8, [(NEAREST, CONST), (LINEAR, REPL)]),
                                  (3, np.float32, [(LINEAR, REFLECT)]), (1, np.float32, [(LINEAR, REFLECT), (NEAREST, CONST)])):
            src = _img(rng, h, w, cn, dtype)
            for interp, border in combos:
                want = oracle.remap(src, xm, ym, interp, border)
                for s in (src, torch.from_numpy(src).cuda()):
                    corner, dst = warper.warp(s, K, R, interp, border)
                    got = _np(dst)
                    assert corner == roi[:2] and got.dtype == want.dtype and np.array_equal(got, want), (cn, dtype, interp, border, np.argwhere(got != want)[:4])
        # the fused image + mask warp: all-255 mask and a caller's mask, CV_8UC3 and CV_16SC3 tiles
        img = _img(rng, h, w)
        wi = oracle.remap(img, xm, ym, LINEAR, REFLECT)
        wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST)
        holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
        wh = oracle.remap(holes, xm, ym, NEAREST, CONST)
        for s, hm in ((img, holes), (torch.from_numpy(img).cuda(), torch.from_numpy(holes).cuda())):
            for out16 in (False, True):
                c, gi, gm = warper.warp_with_mask(s, K, R, out16=out16)
                assert c == roi[:2] and np.array_equal(_np(gi), wi.astype(np.int16) if out16 else wi) and np.array_equal(_np(gm), wm)
                c, gi, gm = warper.warp_with_mask(s, K, R, mask=hm, out16=out16)
                assert np.array_equal(_np(gi), wi.astype(np.int16) if out16 else wi) and np.array_equal(_np(gm), wh)
        # isx_warper_warp / isx_warper_warp_with_mask with the caller's dst: the corner comes back from the call
        c, gi = warper.warp(img, K, R, LINEAR, REFLECT, dst=np.empty_like(wi))
        assert c == roi[:2] and np.array_equal(gi, wi)
        c, gi, gm = warper.warp_with_mask(img, K, R, dst_img=np.empty_like(wi), dst_mask=np.empty_like(wm))
        assert c == roi[:2] and np.array_equal(gi, wi) and np.array_equal(gm, wm)


def test_a_4k_source(gpu, oracle):
    """config-2-sized: 3840 x 2160, scale = f = 3000, yaw 0.36, with a translation."""
    import torch
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    T = np.array([0.11, -0.07, 0.05], np.float32)
    img = synth.make_tile(H, W, 1)
    roi, wi, wm = _model_tile(oracle, F, K, Rs[1], T, img)
    warper = _warper(gpu, F, T)
    c, gi, gm = warper.warp_with_mask(torch.from_numpy(img).cuda(), K, Rs[1])
    assert c == roi[:2] and np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gm.cpu().numpy(), wm)
    c, gi = warper.warp(torch.from_numpy(img).cuda(), K, Rs[1], LINEAR, REFLECT)
    assert np.array_equal(gi.cpu().numpy(), wi)


def test_pitched_and_byte_unaligned_mats(gpu, oracle):
    import torch
    rng = np.random.default_rng(77)
    w, h = 211, 67                                      # odd width: dense CV_8UC3 rows start on every byte alignment
    scale, K, R, T = _rig(rng, w, h, True)
    img = _img(rng, h, w)
    roi, wi, wm = _model_tile(oracle, scale, K, R, T, img)
    dh, dw = wm.shape
    warper = _warper(gpu, scale, T)
    for off in (1, 2, 3):
        buf = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device="cuda")
        src = buf[off:off + h * w * 3].view(h, w, 3)
        src.copy_(torch.from_numpy(img))
        assert src.data_ptr() % 4 == off
        dbuf = torch.zeros(dh * dw * 3 + 8, dtype=torch.uint8, device="cuda")
        dimg = dbuf[off:off + dh * dw * 3].view(dh, dw, 3)
        mbuf = torch.zeros(dh * dw + 8, dtype=torch.uint8, device="cuda")
        dmask = mbuf[4 - off:4 - off + dh * dw].view(dh, dw)
        c, gi, gm = warper.warp_with_mask(src, K, R, dst_img=dimg, dst_mask=dmask)
        assert c == roi[:2] and np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gm.cpu().numpy(), wm)
        assert int(dbuf[:off].sum()) == 0 and int(dbuf[off + dh * dw * 3:].sum()) == 0, "wrote outside the tile"
        c, g2 = warper.warp(src, K, R, LINEAR, REFLECT, dst=dimg.zero_())
        assert np.array_equal(g2.cpu().numpy(), wi)
    # pitched source and destinations (row pitch a multiple of 64 bytes), CV_16SC3 tile
    sp = (w * 3 + 63) // 64 * 64
    src = torch.zeros(h * sp, dtype=torch.uint8, device="cuda").as_strided((h, w, 3), (sp, 3, 1))
    src.copy_(torch.from_numpy(img))
    p16 = (dw * 6 + 63) // 64 * 64
    dimg = torch.zeros(dh * p16 // 2, dtype=torch.int16, device="cuda").as_strided((dh, dw, 3), (p16 // 2, 3, 1))
    pm = (dw + 63) // 64 * 64
    dmask = torch.zeros(dh * pm, dtype=torch.uint8, device="cuda").as_strided((dh, dw), (pm, 1))
    warper.warp_with_mask(src, K, R, dst_img=dimg, dst_mask=dmask)
    assert np.array_equal(dimg.cpu().numpy(), wi.astype(np.int16)) and np.array_equal(dmask.cpu().numpy(), wm)
    # host mats whose rows are views into a wider array
    wide = np.zeros((h, w + 5, 3), np.uint8)
    wide[:, 2:2 + w] = img
    c, gi = warper.warp(wide[:, 2:2 + w], K, R, LINEAR, REFLECT)
    assert np.array_equal(gi, wi)


def test_planned_warps_and_plan_status(gpu, oracle):
    import torch
    rng = np.random.default_rng(5)
    w, h = 400, 300
    scale, K, R, T = _rig(rng, w, h, True)
    img = _img(rng, h, w)
    roi, wi, wm = _model_tile(oracle, scale, K, R, T, img)
    warper = _warper(gpu, scale, T)
    assert warper.verify_is_light((w, h), K, R)
    src = torch.from_numpy(img).cuda()
    dimg = torch.zeros(wi.shape, dtype=torch.uint8, device="cuda")
    dmask = torch.zeros(wm.shape, dtype=torch.uint8, device="cuda")
    for deferred in (False, True):
        warper.set_deferred_verify(deferred)
        warper.warp_with_mask_planned(src, K, R, roi, dimg.zero_(), dmask.zero_())
        if deferred:
            warper.verify()
        assert warper.plan_status() == 0
        assert np.array_equal(dimg.cpu().numpy(), wi) and np.array_equal(dmask.cpu().numpy(), wm)
    warper.queue_verify((w, h), K, R, roi)
    warper.verify()
    assert warper.plan_status() == 0
    # a deliberately wrong plan (the rectangle one pixel to the right): the warp fills it as asked, the verification reports it
    wrong = (roi[0] + 1, roi[1], roi[2] + 1, roi[3])
    _, wi2, wm2 = _model_tile(oracle, scale, K, R, T, img, np.array(wrong))
    warper.warp_with_mask_planned(src, K, R, wrong, dimg, dmask)
    with pytest.raises(gpu.IsxError) as e:
        warper.plan_status()
    assert e.value.code == 8
    assert np.array_equal(dimg.cpu().numpy(), wi2) and np.array_equal(dmask.cpu().numpy(), wm2)
    # a translation the plan was not made for is a stale plan too
    w2 = _warper(gpu, scale, T)
    w2.set_translation(T + np.float32(0.01))
    w2.warp_with_mask_planned(src, K, R, roi, dimg, dmask)
    with pytest.raises(gpu.IsxError) as e:
        w2.plan_status()
    assert e.value.code == 8


@pytest.mark.parametrize("n", [2, 11])
@pytest.mark.parametrize("out16", [False, True])
def test_batches(gpu, oracle, n, out16):
    """begin_batch .. end_batch: 2 tiles, and more tiles than one launch carries (WARP_BATCH_MAX = 8)."""
    import torch
    rng = np.random.default_rng(60 + n)
    w, h = 257, 130
    scale, K, _, T = _rig(rng, w, h, True)
    warper = _warper(gpu, scale, T)
    Rs = [_rot(*rng.uniform(-0.5, 0.5, 3)) for _ in range(n)]
    imgs = [_img(rng, h, w) for _ in range(n)]
    want = [_model_tile(oracle, scale, K, Rs[i], T, imgs[i]) for i in range(n)]
    srcs = [torch.from_numpy(a).cuda() for a in imgs]
    outs = [(torch.zeros(wi.shape, dtype=torch.int16 if out16 else torch.uint8, device="cuda"), torch.zeros(wm.shape, dtype=torch.uint8, device="cuda")) for _, wi, wm in want]
    for i in range(n):                                          # (planning: the tables exist before the batch)
        assert warper.warpRoi((w, h), K, Rs[i]) == want[i][0]
    warper.begin_batch()
    for i in range(n):
        warper.warp_with_mask_planned(srcs[i], K, Rs[i], want[i][0], outs[i][0], outs[i][1])
    warper.end_batch()
    assert warper.plan_status() == 0
    for i in range(n):
        assert np.array_equal(outs[i][0].cpu().numpy(), want[i][1].astype(np.int16) if out16 else want[i][1]), i
        assert np.array_equal(outs[i][1].cpu().numpy(), want[i][2]), i


def test_gain_and_dst_columns(gpu, oracle):
    import torch
    rng = np.random.default_rng(8)
    w, h = 500, 200
    scale, K, R, T = _rig(rng, w, h, True)
    img = _img(rng, h, w)
    roi, wi, wm = _model_tile(oracle, scale, K, R, T, img)
    warper = _warper(gpu, scale, T)
    src = torch.from_numpy(img).cuda()
    for out16 in (False, True):
        warper.set_gain(1.37)
        _, gi, gm = warper.warp_with_mask(src, K, R, out16=out16)
        warper.set_gain(1.0)
        want = oracle.gain_apply(wi, 1.37)
        assert np.array_equal(gi.cpu().numpy(), want.astype(np.int16) if out16 else want) and np.array_equal(gm.cpu().numpy(), wm)
    dw = wm.shape[1]
    c0, c1 = 70, min(dw, 70 + 130)
    dimg = torch.full(wi.shape, 7, dtype=torch.uint8, device="cuda")
    dmask = torch.full(wm.shape, 7, dtype=torch.uint8, device="cuda")
    warper.set_dst_columns(c0, c1)
    warper.warp_with_mask_planned(src, K, R, roi, dimg, dmask)
    warper.set_dst_columns(0, 0)
    assert warper.plan_status() == 0
    gi, gm = dimg.cpu().numpy(), dmask.cpu().numpy()
    assert np.array_equal(gi[:, c0:c1], wi[:, c0:c1]) and np.array_equal(gm[:, c0:c1], wm[:, c0:c1])
    lo = c0 // 64 * 64                                          # computed: the 64-column blocks that hold [c0, c1), cropped at c1
    assert (gi[:, :lo] == 7).all() and (gi[:, c1:] == 7).all() and (gm[:, :lo] == 7).all() and (gm[:, c1:] == 7).all()


def test_a_bounding_box_that_reaches_behind_the_camera(gpu, oracle):
    """z <= 0 inside the rectangle: the plane projector divides all the same (no (-1, -1) sentinel) - every kernel's generic path."""
    import torch
    w, h = 64, 48
    K = np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1]], np.float32)
    R = _rot(0.5, 0.1, 0.0)
    roi = (-400, -60, 40, 60)
    rng = np.random.default_rng(4)
    img = _img(rng, h, w)
    m = P.from_rig(oracle, 60.0, K, R)
    xm, ym = m.build_maps(np.array(roi))
    assert (xm == -1).sum() == 0 and np.abs(xm[np.isfinite(xm)]).max() > 1e4          # no sentinel; the pole's neighbours are far outside
    warper = _warper(gpu, 60.0)
    gx, gy = warper.buildMapsRoi(K, R, roi)
    assert np.array_equal(gx, xm, equal_nan=True) and np.array_equal(gy, ym, equal_nan=True)
    wi = oracle.remap(img, xm, ym, LINEAR, REFLECT)
    wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST)
    src = torch.from_numpy(img).cuda()
    dst = torch.zeros(wi.shape, dtype=torch.uint8, device="cuda")
    warper.warp_roi(src, K, R, LINEAR, REFLECT, roi, dst)                                   # k_warp_tile, image only
    assert np.array_equal(dst.cpu().numpy(), wi)
    dm = torch.zeros(wm.shape, dtype=torch.uint8, device="cuda")
    warper.warp_roi(torch.full((h, w), 255, dtype=torch.uint8, device="cuda"), K, R, NEAREST, CONST, roi, dm)   # k_warp_mask_tile
    assert np.array_equal(dm.cpu().numpy(), wm)
    g = oracle.remap(img, xm, ym, LINEAR, CONST)
    warper.warp_roi(src, K, R, LINEAR, CONST, roi, dst.zero_())                             # k_warp
    assert np.array_equal(dst.cpu().numpy(), g)
    holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
    wh = oracle.remap(holes, xm, ym, NEAREST, CONST)
    _k, kp = f9(K)
    _r, rp = f9(R)
    for mask, wantm in ((None, wm), (torch.from_numpy(holes).cuda(), wh)):                  # k_warp_tile with its mask / k_warp_img_mask
        mi, mdi, mdm = as_mat(src), as_mat(dst.zero_()), as_mat(dm.zero_())
        mm = as_mat(mask) if mask is not None else None
        check(warper._lib.isx_warper_warp_with_mask_roi(warper._h, C.byref(mi), C.byref(mm) if mm is not None else None, kp, rp,
                                                        (C.c_int * 4)(*roi), C.byref(mdi), C.byref(mdm)))
        assert np.array_equal(dst.cpu().numpy(), wi) and np.array_equal(dm.cpu().numpy(), wantm)


def _oracle_pair(oracle, p, scale, bands, prec):
    ob = oracle.MultiBand(bands, prec)
    ob.prepare(p.corners, p.sizes)
    for i in p.active:
        roi, wi, wm = _model_tile(oracle, scale, p.K, p.Rs[i], None, p.imgs[i].cpu().numpy())
        assert roi == tuple(p.rois[i])
        assert np.array_equal(p.warped[i].cpu().numpy(), wi) and np.array_equal(p.wmasks[i].cpu().numpy(), wm)
        ob.feed(wi.astype(np.int16), p.seam[i].cpu().numpy(), p.corners[i])
    return ob.blend(False)


@pytest.mark.parametrize("prec", [F32, I16])
def test_pair_stitcher_plane_eager_and_captured(gpu, oracle, prec):
    import torch
    from imagestitch_amd.pipeline import PairStitcher
    W, H, F = 640, 360, 500.0
    K, Rs = synth.camera_pair(W, H, F, yaw=0.2)
    imgs = [torch.from_numpy(synth.make_tile(H, W, i)).cuda() for i in range(2)]
    p = PairStitcher(imgs, K, Rs, F, "plane", 5, prec, 0, None, "int16")
    ref = [t.clone() for t in p.step()]
    torch.cuda.synchronize()
    assert p.check_plan() == 0
    od, om = _oracle_pair(oracle, p, F, 5, prec)
    assert np.array_equal(ref[1].cpu().numpy(), om) and np.array_equal(ref[0].cpu().numpy(), od)
    p.capture()
    p.out.zero_()
    out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])
    assert p.check_plan() == 0


def test_split_stitcher_takes_the_plane_kind(gpu, oracle):
    import torch
    from imagestitch_amd.pipeline import PairStitcher, SplitStitcher
    W, H, F = 640, 360, 500.0
    K, Rs = synth.camera_pair(W, H, F, yaw=0.2)
    imgs = [torch.from_numpy(synth.make_tile(H, W, i)).cuda() for i in range(2)]
    ref = [t.clone() for t in PairStitcher(imgs, K, Rs, F, "plane", 4, F32, 0, None, "int16").step()]
    sp = SplitStitcher(imgs, K, Rs, F, "plane", 4, F32, 0, "int16", nsplit=2)
    out, m = sp.step()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])


def test_two_threads_on_two_handles(gpu, oracle):
    import torch
    rng = np.random.default_rng(21)
    w, h = 301, 177
    jobs = []
    for t in range(2):
        scale, K, R, T = _rig(rng, w, h, t == 1)
        img = _img(rng, h, w)
        jobs.append((scale, K, R, T, img, _model_tile(oracle, scale, K, R, T, img)))
    errs = []

    def run(j):
        try:
            scale, K, R, T, img, (roi, wi, wm) = jobs[j]
            st = torch.cuda.Stream()
            warper = gpu.PlaneWarper(0, st).create(scale)
            if T is not None:
                warper.set_translation(T)
            with torch.cuda.stream(st):
                src = torch.from_numpy(img).cuda()
                for _ in range(20):
                    c, gi, gm = warper.warp_with_mask(src, K, R)
                    st.synchronize()
                    assert c == roi[:2] and np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gm.cpu().numpy(), wm)
        except BaseException as e:      # noqa: BLE001
            errs.append((j, repr(e)))

    th = [threading.Thread(target=run, args=(j,)) for j in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


def test_translation_is_refused_on_the_other_kinds(gpu, oracle):
    w, h, f = 333, 217, 260.0
    K, Rs = synth.camera_pair(w, h, f, yaw=0.3)
    img = synth.make_tile(h, w, 3, noise_only=True)
    for kind, creator in ((CYL, gpu.CylindricalWarper), (SPH, gpu.SphericalWarper)):
        warper = creator().create(f)
        with pytest.raises(gpu.IsxError) as e:
            warper.set_translation((0.1, 0.0, 0.0))
        assert e.value.code == 6
        warper.set_translation((0.0, 0.0, 0.0))             # all zero is what the overloads without T pass: accepted everywhere
        corner, dst = warper.warp(img, K, Rs[0], LINEAR, REFLECT)
        oc, od, _ = oracle.warp_u8(kind, f, K, Rs[0], img, LINEAR, REFLECT)
        assert corner == oc and np.array_equal(dst, od)
    with pytest.raises(gpu.IsxError) as e:
        gpu.PlaneWarper().create(f).set_translation((0.1, float("nan"), 0.0))
    assert e.value.code == 1


def test_warp_point(gpu, oracle):
    """isx_warper_warp_point: mapForward on the host - the model for the plane kind, the oracle's mapForward for the other two."""
    rng = np.random.default_rng(31)
    for _ in range(20):
        w, h = int(rng.integers(40, 2000)), int(rng.integers(40, 1500))
        scale, K, R, T = _rig(rng, w, h, True)
        pts = [(0, 0), (w - 1, h - 1)] + [(float(rng.uniform(0, w)), float(rng.uniform(0, h))) for _ in range(6)]
        _, _, r_kinv, k_rinv = oracle.camera(K, R)
        for Tm in (None, T):
            m = P.Plane(scale).set_camera(r_kinv, k_rinv, Tm)
            warper = _warper(gpu, scale, Tm)
            for x, y in pts:
                u, v = warper.warpPoint((x, y), K, R)
                mu, mv = m.map_forward(np.float32(x), np.float32(y))
                assert u == mu and v == mv, (x, y, u, mu, v, mv)
        for kind, creator in ((CYL, gpu.CylindricalWarper), (SPH, gpu.SphericalWarper)):
            warper = creator().create(scale)
            for x, y in pts:
                u, v = warper.warpPoint((x, y), K, R)
                ou, ov = oracle.map_forward(kind, scale, r_kinv, np.float32(x), np.float32(y))
                assert u == ou and v == ov, (kind, x, y, u, ou, v, ov)
