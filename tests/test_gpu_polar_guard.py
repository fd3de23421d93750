"""The entries that serve the fisheye and stereographic kinds on mats inside guard bands (tests/helpers/guarded.py), unaligned and aligned,
host and device: they write their outputs and not a byte beside them, and leave their inputs alone.  And every entry that refuses the two
kinds returns ISX_ERR_UNSUPPORTED, names the kind, changes no state and leaves the handle usable."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402
from helpers.guarded import LAYOUTS, NOTHING, guarded, guarded_like  # noqa: E402

from imagestitch_amd._lib import as_mat, check, f9  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]


def _warper(gpu, kind, scale):
    return gpu.RotationWarper(kind, scale)


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_served_entries_write_their_outputs_only(gpu, oracle, kind, where, layout):
    w, h, f, K, R = P.rig(P.SIZES[2], "yaw0.52")              # 261 x 67: a partial 64-column block and a partial 4-row block
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    roi = warper.warpRoi((w, h), K, R)
    xm, ym = m.build_maps(roi)
    dh, dw = xm.shape
    rng = np.random.default_rng(41)
    lib, Kp, Rp, roi_c = warper._lib, f9(K), f9(R), (C.c_int * 4)(*roi)
    # buildMaps
    gx, gy = guarded((dh, dw), np.float32, where, layout, 1, "xmap"), guarded((dh, dw), np.float32, where, layout, 2, "ymap")
    mx, my = as_mat(gx.view), as_mat(gy.view)
    check(lib.isx_warper_build_maps_roi(warper._h, Kp[1], Rp[1], roi_c, C.byref(mx), C.byref(my)))
    _sync()
    gx.check(); gy.check()
    assert PC.same_bits(gx.get(), xm) and PC.same_bits(gy.get(), ym)
    # warp: the four types, one combination each
    for cn, dtype, interp, border in ((3, np.uint8, PC.LINEAR, PC.REFLECT), (1, np.uint8, PC.NEAREST, PC.CONST), (3, np.float32, PC.LINEAR | PC.TIES_EVEN, PC.REPL),
                                      (1, np.float32, PC.LINEAR, PC.REFLECT101)):
        src = PC.image(rng, h, w, cn, dtype)
        gs = guarded_like(src, where, layout, 3, "src")
        gd = guarded((dh, dw) + src.shape[2:], dtype, where, layout, 4, "dst")
        ms, md = as_mat(gs.view), as_mat(gd.view)
        check(lib.isx_warper_warp_roi(warper._h, C.byref(ms), Kp[1], Rp[1], interp, border, roi_c, C.byref(md)))
        _sync()
        gs.check(written=NOTHING); gd.check()
        assert np.array_equal(gd.get(), oracle.remap(src, xm, ym, interp & 1, border))
        corner = (C.c_int * 2)()
        gd.snapshot()
        check(lib.isx_warper_warp(warper._h, C.byref(ms), Kp[1], Rp[1], interp, border, C.byref(md), corner))
        _sync()
        gs.check(written=NOTHING); gd.check()
        assert tuple(corner) == roi[:2]
    # the fused warp: with and without a mask, CV_8UC3 and CV_16SC3, and the gain
    img = PC.image(rng, h, w)
    holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
    wi = oracle.remap(img, xm, ym, PC.LINEAR, PC.REFLECT)
    gi, gh = guarded_like(img, where, layout, 5, "img"), guarded_like(holes, where, layout, 6, "mask")
    mi, mh = as_mat(gi.view), as_mat(gh.view)
    for out16 in (False, True):
        for mask, gain in ((None, 1.0), (mh, 1.0), (None, 1.25)):
            warper.set_gain(gain)
            gdi = guarded((dh, dw, 3), np.int16 if out16 else np.uint8, where, layout, 7, "dst_img")
            gdm = guarded((dh, dw), np.uint8, where, layout, 8, "dst_mask")
            mdi, mdm = as_mat(gdi.view), as_mat(gdm.view)
            check(lib.isx_warper_warp_with_mask_roi(warper._h, C.byref(mi), C.byref(mask) if mask is not None else None, Kp[1], Rp[1], roi_c, C.byref(mdi), C.byref(mdm)))
            _sync()
            gi.check(written=NOTHING); gh.check(written=NOTHING); gdi.check(); gdm.check()
            want = PC.gained(wi, gain) if gain != 1.0 else wi
            assert np.array_equal(gdi.get(), want.astype(gdi.dtype))
            assert np.array_equal(gdm.get(), oracle.remap(holes if mask is not None else np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST))
    warper.set_gain(1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_refused_entries_leave_the_handle_as_it_was(gpu, oracle, kind):
    import torch
    w, h, f, K, R = P.rig(P.SIZES[0], "identity")
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    roi = warper.warpRoi((w, h), K, R)
    xm, ym = m.build_maps(roi)
    img = PC.image(np.random.default_rng(2), h, w)
    wi = oracle.remap(img, xm, ym, PC.LINEAR, PC.REFLECT)
    wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST)
    dimg, dmask = torch.full(wi.shape, 7, dtype=torch.uint8, device="cuda"), torch.full(wm.shape, 7, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(img).cuda()
    refused = [lambda: warper.warp_with_mask_planned(src, K, R, roi, dimg, dmask), lambda: warper.queue_verify((w, h), K, R, roi),
               lambda: warper.verify_is_light((w, h), K, R), warper.begin_batch, lambda: warper.set_dst_columns(0, 64), lambda: warper.set_dst_columns(0, 0),
               lambda: warper.set_deferred_verify(True), lambda: warper.set_translation((0.1, 0.0, 0.0))]
    for call in refused:
        with pytest.raises(gpu.IsxError) as e:
            call()
        assert e.value.code == 6 and PC.KIND_NAMES[kind] in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert int((dimg != 7).sum()) == 0 and int((dmask != 7).sum()) == 0              # the refused planned warp wrote nothing
    # what stays allowed: the zero translation, switching deferred verification off, and the calls that are no-ops with nothing pending
    warper.set_translation((0.0, 0.0, 0.0))
    warper.set_deferred_verify(False)
    warper.end_batch(); warper.verify(); warper.discard_pending(); warper.join()
    assert warper.plan_status() == 0
    # no state changed: the handle warps the whole tile, un-batched, at once
    c, gi, gm = warper.warp_with_mask(src, K, R, dst_img=dimg, dst_mask=dmask)
    torch.cuda.synchronize()
    assert c == roi[:2] and np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gm.cpu().numpy(), wm)
    with pytest.raises(gpu.IsxError) as e:
        gpu.RotationWarper(5, f)
    assert e.value.code == 1
    with pytest.raises(gpu.IsxError):
        gpu.RotationWarper("mercator", f)
