"""isx_resize and isx_mask_dilate_resize_and on mats inside guard bands of seeded bytes (tests/helpers/guarded.py): host and device mats, the
unaligned and the aligned layout, widths that leave a partial 4-pixel group.  The outputs are written and equal the model; not one byte
beside them, and not one byte of the inputs, changes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import guarded as G  # noqa: E402
from helpers import resize_np as R  # noqa: E402

from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
WHERE = ("host", "device")
# destination (width, height): one pixel, a partial group alone, full groups + 1, 2, 3 pixels, one group past a wave's 256 columns, rows that are
# no multiple of the 4 (resize) or 16 (mask stage) a workgroup covers
DST = [(1, 1), (3, 2), (5, 4), (66, 5), (67, 17), (257, 3), (64, 33)]
SRC = [(4, 3), (7, 5), (10, 8), (31, 9), (134, 34), (100, 2), (64, 33)]        # (width, height) per destination: up, down, the area rule, equal


def _ref(g):
    return C.byref(_lib.as_mat(g.view))


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_resize_inside_guard_bands(gpu, where, layout):
    rng = np.random.default_rng(21)
    lib = _lib.load()
    seed = 1000
    for (dw, dh), (sw, sh) in zip(DST, SRC):
        for dtype, cn in ((np.uint8, 1), (np.uint8, 3), (np.float32, 1), (np.float32, 3)):
            shape = (sh, sw, cn) if cn > 1 else (sh, sw)
            src = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else (rng.standard_normal(shape) * 1e4).astype(np.float32)
            for interp in (R.LINEAR, R.NEAREST):
                seed += 2
                gs = G.guarded_like(src, where, layout, seed, "src")
                gd = G.guarded((dh, dw, cn) if cn > 1 else (dh, dw), dtype, where, layout, seed + 1, "dst")
                _lib.check(lib.isx_resize(_ref(gs), _ref(gd), interp, 0, None))
                _sync()
                assert np.array_equal(gd.get(), R.resize(src, (dw, dh), interp)), (dw, dh, sw, sh, cn, interp)
                gd.check()
                gs.check(G.NOTHING)


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_dilate_resize_and_inside_guard_bands(gpu, where, layout):
    rng = np.random.default_rng(22)
    lib = _lib.load()
    seed = 5000
    for k, ((dw, dh), (sw, sh)) in enumerate(zip(DST, SRC)):
        seam = np.where(rng.random((sh, sw)) < 0.25, 255, 0).astype(np.uint8)
        warped = np.where(rng.random((dh, dw)) < 0.8, 255, 0).astype(np.uint8)
        kw, kh = [(3, 3), (1, 1), (20, 20), (2, 3)][k % 4]
        for with_warped in (True, False):
            seed += 3
            gs = G.guarded_like(seam, where, layout, seed, "seam_mask")
            gw = G.guarded_like(warped, where, layout, seed + 1, "warped_mask") if with_warped else None
            go = G.guarded((dh, dw), np.uint8, where, layout, seed + 2, "out")
            _lib.check(lib.isx_mask_dilate_resize_and(_ref(gs), _ref(gw) if gw is not None else None, kw, kh, _ref(go), 0, None))
            _sync()
            assert np.array_equal(go.get(), R.dilate_resize_and(seam, warped if with_warped else None, kw, kh, (dw, dh))), (dw, dh, sw, sh, kw, kh)
            go.check()
            gs.check(G.NOTHING)
            if gw is not None:
                gw.check(G.NOTHING)
        # in place: the warped mask is the output
        seed += 2
        gs = G.guarded_like(seam, where, layout, seed, "seam_mask")
        gw = G.guarded_like(warped, where, layout, seed + 1, "warped_mask")
        _lib.check(lib.isx_mask_dilate_resize_and(_ref(gs), _ref(gw), kw, kh, _ref(gw), 0, None))
        _sync()
        assert np.array_equal(gw.get(), R.dilate_resize_and(seam, warped, kw, kh))
        gw.check()
        gs.check(G.NOTHING)
