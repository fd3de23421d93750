"""k_polar_roi_scan where its extrema sit: detectResultRoi on the scan rigs of tests/polar_cases.py (tests/test_polar_scan_census.py shows, by
the model alone, that they put an extremum into every column block, wave, lane half and row band the reduction distinguishes), the ROI and
the four float extrema against tests/helpers/polar_np.py bit for bit with the ROI cache off; and the camera whose mapForward is NaN on every
source pixel, where min / max keep +-FLT_MAX."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402

from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]
ERR_INVALID = 1


def _warper(gpu, kind, scale):
    return (gpu.FisheyeWarper if kind == P.FISHEYE else gpu.StereographicWarper)().create(scale)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(PC.SCAN_RIGS))
def test_roi_of_every_scan_rig_equals_the_model(gpu, name, kind):
    w, h, f, K, R = PC.scan_rig(name, kind)
    mroi, mmm = P.from_rig(kind, f, K, R).detect_roi(w, h)
    warper = _warper(gpu, kind, f)
    warper.set_roi_cache(False)
    K2 = K.copy()
    K2[0, 2] += 3.0                                           # another camera in between: the last-answer memo never serves the second scan
    for _ in range(2):
        roi, mm = warper.warpRoi((w, h), K, R, with_minmax=True)
        assert roi == tuple(int(v) for v in mroi) and np.array_equal(mm, mmm), (name, kind, roi, mroi, mm, mmm)
        roi2, mm2 = warper.warpRoi((w, h), K2, R, with_minmax=True)
        m2roi, m2mm = P.from_rig(kind, f, K2, R).detect_roi(w, h)
        assert roi2 == tuple(int(v) for v in m2roi) and np.array_equal(mm2, m2mm), (name, kind, roi2, m2roi)


@pytest.mark.parametrize("kind", KINDS)
def test_a_camera_whose_forward_map_is_nan_everywhere(gpu, kind):
    """setCameraParams accepts PC.NAN_CAMERA (finite K and R).  The device scan, the host loop and the model agree on +-FLT_MAX and four
    INT_MIN; warp, warp_with_mask and buildMaps then fail with the degenerate-ROI error and write nothing; the handle goes on serving."""
    import torch
    K, R = PC.NAN_CAMERA
    w, h, f = 8, 6, 25.0
    m = P.from_rig(kind, f, K, R)
    mroi, mmm = m.detect_roi(w, h)
    assert [int(v) for v in mroi] == [P.INT_MIN] * 4
    warper = _warper(gpu, kind, f)
    for cache in (False, True):
        warper.set_roi_cache(cache)
        for _ in range(2):
            roi, mm = warper.warpRoi((w, h), K, R, with_minmax=True)
            assert roi == tuple(int(v) for v in mroi) and np.array_equal(mm, mmm), (roi, mm)
    warper.set_roi_cache(False)
    hroi, hmm = (C.c_int * 4)(), (C.c_float * 4)()
    _lib.check(_lib.load().isx_selftest_roi_host(kind, f, _lib.f9(K)[1], _lib.f9(R)[1], w, h, 0, hroi, hmm))
    assert tuple(hroi) == tuple(int(v) for v in mroi) and np.array_equal(np.array(list(hmm), F), mmm)
    src = PC.image(np.random.default_rng(5), h, w)
    for where in ("host", "device"):
        s = src if where == "host" else torch.from_numpy(src).cuda()
        mk = (lambda shape, dt: np.full(shape, 7, dt)) if where == "host" else (lambda shape, dt: torch.full(shape, 7, dtype=getattr(torch, np.dtype(dt).name), device="cuda"))
        d, di, dm, xm, ym = mk((1, 1, 3), np.uint8), mk((1, 1, 3), np.uint8), mk((1, 1), np.uint8), mk((1, 1), np.float32), mk((1, 1), np.float32)
        for call in (lambda: warper.warp(s, K, R, PC.LINEAR, PC.REFLECT, dst=d), lambda: warper.warp_with_mask(s, K, R, dst_img=di, dst_mask=dm),
                     lambda: _build_maps(warper, w, h, K, R, xm, ym)):
            with pytest.raises(gpu.IsxError) as e:
                call()
            assert e.value.code == ERR_INVALID and "degenerate ROI" in e.value.msg, e.value.msg
            del e
        torch.cuda.synchronize()
        for a in (d, di, dm, xm, ym):
            a = a.cpu().numpy() if hasattr(a, "cpu") else a
            assert (a == 7).all()
    w2, h2, f2, K2, R2 = P.rig(P.SIZES[0], "identity")
    assert f2 == f
    roi, mm = warper.warpRoi((w2, h2), K2, R2, with_minmax=True)
    m2roi, m2mm = P.from_rig(kind, f2, K2, R2).detect_roi(w2, h2)
    assert roi == tuple(int(v) for v in m2roi) and np.array_equal(mm, m2mm)          # the keys were re-armed behind the NaN scans


def _build_maps(warper, w, h, K, R, xm, ym):
    mx, my = _lib.as_mat(xm), _lib.as_mat(ym)
    _lib.check(warper._lib.isx_warper_build_maps(warper._h, w, h, _lib.f9(K)[1], _lib.f9(R)[1], C.byref(mx), C.byref(my), (C.c_int * 4)()))
