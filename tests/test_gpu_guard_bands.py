"""No entry point writes outside the mats it is given.  Every isx_mat-taking entry of include/imagestitch_hip.h runs on mats that lie
inside guard bands of seeded random bytes (tests/helpers/guarded.py): outputs and in-place mats, and the const inputs as well.  After
the call (and a device synchronise) every output equals what the oracle or the NumPy model gives - the expectations the other GPU
tests compute, no new reference -, not one byte around an output has changed, nor any byte of an input's buffer.  Both residencies
(host mats: the staging's pitched copy-back; device mats: the kernels' stores), an "odd" layout (per-pixel stores) and an "aligned"
one (dword / vector stores), at the smallest shapes where a store can go wrong: widths with a partial 4-pixel group, a partial
64-column block and one column past a 256-column grid step; 1, 3, 4, 5 and 17 rows."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import blocks_gain_np as BG  # noqa: E402
from helpers import dpseam_grad_np as M  # noqa: E402
from helpers import graphcut_grad_np as GCG  # noqa: E402
from helpers import graphcut_np as GC  # noqa: E402
from helpers import guarded as G  # noqa: E402
from helpers import plane_np as P  # noqa: E402
from helpers import voronoi_np as V  # noqa: E402
from imagestitch_amd import _lib, synth  # noqa: E402
from seam_cases import make_case, make_find_case  # noqa: E402
from test_gain_model import feed_model  # noqa: E402

pytestmark = pytest.mark.gpu

CYL, SPH, PLANE = 0, 1, 2
NEAREST, LINEAR = 0, 1
CONST, REFLECT = 0, 2
I16, F32, F16 = 0, 1, 2
WHERE = ("host", "device")
LAYOUTS = G.LAYOUTS
# (width, height): a partial 4-pixel group, a partial 64-column block, one column past a 256-column grid step; 4 rows per thread, odd bands
SHAPES = [(1, 1), (2, 3), (3, 17), (5, 4), (63, 5), (64, 3), (65, 17), (67, 4), (257, 5)]
SHAPES3 = [(5, 4), (67, 17), (257, 3)]                         # the three partial-unit classes, for the costlier entries
# (kind, source w, source h, focal) -> the size of detectResultRoi's rectangle under rig() (searched on the CPU oracle; asserted below)
CAMERAS = {(CYL, 4, 3, 90.0): (5, 4), (CYL, 67, 17, 90.0): (64, 17), (CYL, 69, 4, 90.0): (65, 5), (CYL, 2, 1, 40.0): (2, 1),
           (SPH, 2, 17, 40.0): (3, 17), (SPH, 71, 16, 90.0): (67, 17), (SPH, 66, 16, 90.0): (63, 17), (SPH, 1, 1, 40.0): (1, 1),
           (PLANE, 4, 4, 40.0): None, (PLANE, 66, 16, 90.0): None, (PLANE, 2, 17, 40.0): None,
           (CYL, 268, 3, 380.0): (257, 8), (SPH, 266, 2, 420.0): (257, 7), (PLANE, 258, 3, 400.0): None}   # past a 256-column grid step
_seed = [0]


@pytest.fixture(autouse=True)
def own_seeds(request):
    """The fill seeds of a case come from its own name and parameters and a counter that starts here: the bytes a case sees do not
    depend on which cases ran before it (a failure in the whole suite shows again under -k)."""
    _seed[0] = zlib.crc32(request.node.name.encode()) << 16


def seed():
    _seed[0] += 1
    return _seed[0]


def sync():
    import torch
    torch.cuda.synchronize()


def gin(a, where, layout, name=None):
    return G.guarded_like(a, where, layout, seed(), name)


def gout(shape, dtype, where, layout, name=None):
    return G.guarded(shape, dtype, where, layout, seed(), name)


def mat(g):
    return _lib.as_mat(g.view if isinstance(g, G.Guarded) else g)


def ref(g):
    return C.byref(mat(g)) if g is not None else None


def unchanged(*inputs):
    for g in inputs:
        if g is not None:
            g.check(G.NOTHING)


def equal(g, want, what=None):
    got = g.get()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), (what, np.argwhere(got != want)[:4])


def rig(w, h, f):
    K, Rs = synth.camera_pair(w, h, f, yaw=0.1, pitch=0.05, roll=0.02)
    return K, Rs[0]


def maps(oracle, kind, f, K, R, w, h, roi=None):
    """(roi, xmap, ymap) by the oracle (the plane projector: by its NumPy model), over detectResultRoi's rectangle or the caller's."""
    if kind == PLANE:
        m = P.from_rig(oracle, f, K, R, None)
        if roi is None:
            roi, _ = m.detect_roi(w, h)
        xm, ym = m.build_maps(roi)
    else:
        if roi is None:
            roi, _ = oracle.detect_roi(kind, f, K, R, w, h)
        _, _, _, kr = oracle.camera(K, R)
        xm, ym = oracle.build_maps(kind, f, kr, np.asarray(roi, np.int32))
    return tuple(int(v) for v in roi), xm, ym


def make_warper(gpu, kind, f):
    return {CYL: gpu.CylindricalWarper, SPH: gpu.SphericalWarper, PLANE: gpu.PlaneWarper}[kind]().create(f)


def camera_cases(oracle, kinds=(CYL, SPH, PLANE)):
    for (kind, w, h, f), size in CAMERAS.items():
        if kind not in kinds:
            continue
        K, R = rig(w, h, f)
        roi, xm, ym = maps(oracle, kind, f, K, R, w, h)
        if size is not None:
            assert (xm.shape[1], xm.shape[0]) == size, (kind, w, h, f, xm.shape)
        assert xm.shape[1] > 256 or w < 256, (kind, w, h, f, xm.shape)
        yield kind, w, h, f, K, R, roi, xm, ym


def img_u8(rng, h, w, cn=3):
    return rng.integers(0, 256, (h, w, cn) if cn > 1 else (h, w), dtype=np.uint8)


# ---- warper ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_warper_warp(gpu, oracle, where, layout):
    """isx_warper_warp: the three projectors, CV_8UC3 / CV_8UC1 / CV_32FC3 / CV_32FC1."""
    rng = np.random.default_rng(1)
    widths = set()
    for kind, w, h, f, K, R, roi, xm, ym in camera_cases(oracle):
        warper = make_warper(gpu, kind, f)
        widths.add(xm.shape[1])
        for cn, dtype, interp, border in ((3, np.uint8, LINEAR, REFLECT), (1, np.uint8, NEAREST, CONST), (3, np.float32, LINEAR, REFLECT),
                                          (1, np.float32, LINEAR, CONST)):
            src = img_u8(rng, h, w, cn)
            src = src if dtype == np.uint8 else src.astype(np.float32) * np.float32(1.37)
            want = oracle.remap(src, xm, ym, interp, border)
            s, d = gin(src, where, layout, "src"), gout(want.shape, dtype, where, layout, "dst")
            corner, _ = warper.warp(s.view, K, R, interp, border, dst=d.view)
            sync()
            assert corner == roi[:2]
            equal(d, want, (kind, w, h, cn, dtype))
            d.check()
            unchanged(s)
    assert {5, 64, 65, 2, 3, 67, 63, 1, 257} <= widths


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_warper_rectangles_of_the_callers(gpu, oracle, where, layout):
    """isx_warper_warp_roi, isx_warper_warp_with_mask_roi and isx_warper_build_maps_roi over rectangles of exactly the wanted sizes
    (the entries do not check that a rectangle is detectResultRoi's), and isx_warper_build_maps over detectResultRoi's.  The fused
    call runs without a source mask (k_warp_tile: blocks of 64 columns) and with the caller's (k_warp_img_mask: 4 pixels per thread,
    a grid step of 256 columns - at 257 its second block in x stores one column), CV_8UC3 and CV_16SC3."""
    rng = np.random.default_rng(2)
    lib = _lib.load()
    for kind in (CYL, SPH, PLANE):
        w, h, f = 71, 16, 90.0
        K, R = rig(w, h, f)
        full, _, _ = maps(oracle, kind, f, K, R, w, h)
        warper = make_warper(gpu, kind, f)
        img = img_u8(rng, h, w)
        holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
        _k, kp = _lib.f9(K)
        _r, rp = _lib.f9(R)
        for dw, dh in SHAPES:
            roi = (full[0] - 3, full[1] - 1, full[0] - 3 + dw - 1, full[1] - 1 + dh - 1)
            _, xm, ym = maps(oracle, kind, f, K, R, w, h, roi)
            croi = (C.c_int * 4)(*roi)
            gx, gy = gout((dh, dw), np.float32, where, layout, "xmap"), gout((dh, dw), np.float32, where, layout, "ymap")
            _lib.check(lib.isx_warper_build_maps_roi(warper._h, kp, rp, croi, ref(gx), ref(gy)))
            sync()
            equal(gx, xm), equal(gy, ym)
            gx.check(), gy.check()
            s, sm, d = gin(img, where, layout, "src"), gin(holes, where, layout, "src_mask"), gout((dh, dw, 3), np.uint8, where, layout, "dst")
            warper.warp_roi(s.view, K, R, LINEAR, REFLECT, roi, d.view)
            sync()
            wi = oracle.remap(img, xm, ym, LINEAR, REFLECT)
            equal(d, wi, ("warp_roi", kind, dw, dh))
            d.check()
            unchanged(s)
            wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST)
            wh = oracle.remap(holes, xm, ym, NEAREST, CONST)
            for out16, mask in ((False, None), (True, None), (False, sm), (True, sm)):
                di = gout((dh, dw, 3), np.int16 if out16 else np.uint8, where, layout, "dst_img")
                dm = gout((dh, dw), np.uint8, where, layout, "dst_mask")
                _lib.check(lib.isx_warper_warp_with_mask_roi(warper._h, ref(s), ref(mask), kp, rp, croi, ref(di), ref(dm)))
                sync()
                equal(di, wi.astype(np.int16) if out16 else wi, ("with_mask_roi", kind, dw, dh, out16, mask is not None))
                equal(dm, wh if mask else wm, ("with_mask_roi mask", kind, dw, dh, out16, mask is not None))
                di.check(), dm.check()
                unchanged(s, sm)
        # isx_warper_build_maps: detectResultRoi's rectangle
        _, xm, ym = maps(oracle, kind, f, K, R, w, h)
        gx, gy = gout(xm.shape, np.float32, where, layout, "xmap"), gout(xm.shape, np.float32, where, layout, "ymap")
        r2 = (C.c_int * 4)()
        _lib.check(lib.isx_warper_build_maps(warper._h, w, h, kp, rp, ref(gx), ref(gy), r2))
        sync()
        assert tuple(r2) == full
        equal(gx, xm), equal(gy, ym)
        gx.check(), gy.check()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("out16", [False, True])
def test_warper_warp_with_mask_and_planned(gpu, oracle, where, layout, out16):
    """isx_warper_warp_with_mask (k_warp_tile; with a caller's mask k_warp_img_mask) and isx_warper_warp_with_mask_planned, CV_8UC3 and
    CV_16SC3 tiles, with isx_warper_set_gain folded in; rectangles of 1 to 67 columns and of 257 (the plane's: more than 256)."""
    rng = np.random.default_rng(3)
    for kind, w, h, f, K, R, roi, xm, ym in camera_cases(oracle):
        warper = make_warper(gpu, kind, f)
        img = img_u8(rng, h, w)
        holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
        wi = oracle.remap(img, xm, ym, LINEAR, REFLECT)
        wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST)
        wh = oracle.remap(holes, xm, ym, NEAREST, CONST)
        dt = np.int16 if out16 else np.uint8
        s, sm = gin(img, where, layout, "src_img"), gin(holes, where, layout, "src_mask")
        for mask, gain, planned in ((None, 1.0, False), (sm, 1.0, False), (None, 1.0, True), (sm, 1.0, True), (None, 1.37, False), (None, 0.6, True)):
            di, dm = gout(wi.shape, dt, where, layout, "dst_img"), gout(wm.shape, np.uint8, where, layout, "dst_mask")
            warper.set_gain(gain)
            if planned:
                warper.warp_with_mask_planned(s.view, K, R, roi, di.view, dm.view, mask=mask.view if mask else None)
            else:
                corner, _, _ = warper.warp_with_mask(s.view, K, R, mask=mask.view if mask else None, out16=out16, dst_img=di.view, dst_mask=dm.view)
                assert corner == roi[:2]
            warper.set_gain(1.0)
            sync()
            want = wi if gain == 1.0 else oracle.gain_apply(wi, gain)
            equal(di, want.astype(dt), (kind, w, h, out16, mask is not None, gain, planned))
            equal(dm, wh if mask else wm)
            di.check(), dm.check()
            unchanged(s, sm)
        assert warper.plan_status() == 0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_warper_batch_of_two_tiles(gpu, oracle, layout):
    """isx_warper_begin_batch .. isx_warper_end_batch: two device tiles of different sizes in one launch, and then with a tile of host
    mats between them - that one cannot be collected: it is launched at once, behind the tile collected so far, and comes back through
    the staging buffers; the device tile after it waits for isx_warper_end_batch."""
    rng = np.random.default_rng(4)
    for kind in (CYL, SPH):
        cases = [c for c in camera_cases(oracle, (kind,))]
        for tiles, res in (((cases[0], cases[1]), ("device", "device")), ((cases[2], cases[3]), ("device", "device")),
                           ((cases[0], cases[2], cases[1]), ("device", "host", "device")), ((cases[2], cases[4], cases[3]), ("device", "host", "device"))):
            f = 90.0                                                 # one handle: its scale is the batch's
            warper = make_warper(gpu, kind, f)
            jobs = []
            for k, ((_, w, h, _, K, R, _, _, _), r) in enumerate(zip(tiles, res)):
                roi, xm, ym = maps(oracle, kind, f, K, R, w, h)
                img = img_u8(rng, h, w)
                out16 = k == 1
                wi = oracle.remap(img, xm, ym, LINEAR, REFLECT)
                wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST)
                jobs.append((gin(img, r, layout, "src"), K, R, roi, gout(wi.shape, np.int16 if out16 else np.uint8, r, layout, "dst_img"),
                             gout(wm.shape, np.uint8, r, layout, "dst_mask"), wi.astype(np.int16) if out16 else wi, wm))
            warper.begin_batch()
            for s, K, R, roi, di, dm, _, _ in jobs:
                warper.warp_with_mask_planned(s.view, K, R, roi, di.view, dm.view)
            sync()
            flushed = res.index("host") + 1 if "host" in res else 0  # the host tile sent itself and what was collected before it off
            for k, (s, _, _, _, di, dm, wi, wm) in enumerate(jobs):
                if k < flushed:
                    equal(di, wi, ("before end_batch", k)), equal(dm, wm)
                    di.check(), dm.check()
                    unchanged(s)
                else:                                                # collected, not launched
                    unchanged(s, di, dm)
            warper.end_batch()
            sync()
            for s, _, _, _, di, dm, wi, wm in jobs:
                equal(di, wi), equal(dm, wm)
                di.check(), dm.check()
                unchanged(s)
            assert warper.plan_status() == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("out16", [False, True])
def test_warper_dst_columns(gpu, oracle, where, layout, out16):
    """isx_warper_set_dst_columns: the columns [col0 rounded down to a block of 64, col1) are computed, the rest of the mats is left
    as it is - ranges that end inside a 64-column block, at its edge, past the tile."""
    rng = np.random.default_rng(5)
    lib = _lib.load()
    w, h, f = 71, 16, 90.0
    K, R = rig(w, h, f)
    _k, kp = _lib.f9(K)
    _r, rp = _lib.f9(R)
    img = img_u8(rng, h, w)
    for kind in (CYL, SPH, PLANE):
        full, _, _ = maps(oracle, kind, f, K, R, w, h)
        warper = make_warper(gpu, kind, f)
        s = gin(img, where, layout, "src")
        for (dw, dh), ranges in (((257, 5), [(0, 1), (70, 100), (64, 128), (130, 257), (200, 300)]), ((67, 17), [(3, 5), (60, 66), (65, 67)]),
                                 ((130, 4), [(128, 129), (1, 130)])):
            roi = (full[0] - 2, full[1], full[0] - 2 + dw - 1, full[1] + dh - 1)
            _, xm, ym = maps(oracle, kind, f, K, R, w, h, roi)
            wi = oracle.remap(img, xm, ym, LINEAR, REFLECT)
            wi = wi.astype(np.int16) if out16 else wi
            wm = oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST)
            for c0, c1 in ranges:
                di, dm = gout(wi.shape, wi.dtype, where, layout, "dst_img"), gout(wm.shape, np.uint8, where, layout, "dst_mask")
                warper.set_dst_columns(c0, c1)
                _lib.check(lib.isx_warper_warp_with_mask_roi(warper._h, ref(s), None, kp, rp, (C.c_int * 4)(*roi), ref(di), ref(dm)))
                warper.set_dst_columns(0, 0)
                sync()
                lo, hi = c0 // 64 * 64, min(c1, dw)
                assert np.array_equal(di.get()[:, lo:hi], wi[:, lo:hi]) and np.array_equal(dm.get()[:, lo:hi], wm[:, lo:hi]), (kind, dw, dh, c0, c1)
                di.check(written=(lo, hi)), dm.check(written=(lo, hi))
                unchanged(s)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_remap(gpu, oracle, where, layout):
    """isx_remap: src, xmap and ymap are inputs; CV_8UC1 / CV_8UC3 / CV_32FC1 / CV_32FC3."""
    rng = np.random.default_rng(6)
    for (dw, dh), (cn, dtype, interp, border) in zip(SHAPES, [(3, np.uint8, 1, 2), (1, np.uint8, 0, 0), (3, np.float32, 1, 2), (1, np.float32, 1, 4)] * 3):
        src = (rng.random((13, 19, cn) if cn > 1 else (13, 19)) * 255).astype(dtype)
        xm = (rng.random((dh, dw)) * 25 - 3).astype(np.float32)
        ym = (rng.random((dh, dw)) * 18 - 3).astype(np.float32)
        want = oracle.remap(src, xm, ym, interp, border)
        s, gx, gy = gin(src, where, layout, "src"), gin(xm, where, layout, "xmap"), gin(ym, where, layout, "ymap")
        d = gout(want.shape, dtype, where, layout, "dst")
        _lib.check(_lib.load().isx_remap(ref(s), ref(gx), ref(gy), interp, border, ref(d), 0, None))
        sync()
        equal(d, want, (dw, dh, cn, dtype))
        d.check()
        unchanged(s, gx, gy)


# ---- blender -----------------------------------------------------------------------------------------------------------------------------
# (corners, sizes (w, h), bands): results of 67 x 21, 131 x 37 and 5 x 5 - a partial column group and an odd height at every level
BLENDS = {"two_bands": ([(0, 0), (30, 2)], [(37, 19), (37, 19)], 2), "five_bands": ([(0, 0), (64, 4)], [(70, 33), (67, 33)], 5),
          "tiny": ([(0, 0), (2, 1)], [(3, 4), (3, 4)], 2)}
_blend_cache = {}


def blend_case(name):
    """The tiles of a BLENDS entry: per tile (CV_8UC3 image, seam mask, warped mask, fed mask = dilate 3 x 3 (seam) & warped)."""
    if name not in _blend_cache:
        from oracle import capi as O
        corners, sizes, bands = BLENDS[name]
        rng = np.random.default_rng(len(name))
        tiles = []
        for w, h in sizes:
            img = img_u8(rng, h, w)
            seam = (rng.random((h, w)) > 0.3).astype(np.uint8) * 255
            warped = (rng.random((h, w)) > 0.1).astype(np.uint8) * 255
            tiles.append((img, seam, warped, O.dilate_rect(seam, 3, 3) & warped))
        _blend_cache[name] = (corners, sizes, bands, tiles, {})
    return _blend_cache[name]


def blend_want(name, kind, prec=I16, f32=False):
    from oracle import capi as O
    corners, sizes, bands, tiles, memo = blend_case(name)
    key = (kind, prec, f32)
    if key not in memo:
        ob = {"mb": lambda: O.MultiBand(bands, prec), "feather": lambda: O.Feather(0.1), "no": O.NoBlend}[kind]()
        ob.prepare(corners, sizes)
        for (img, _, _, fed), c in zip(tiles, corners):
            ob.feed(img.astype(np.int16), fed, c)
        memo[key] = ob.blend(f32) if kind == "mb" else ob.blend()
    return memo[key]


FEEDS = {"two_bands": "feed", "five_bands": "feed_u8", "tiny": "feed_dilated"}


def feed_guarded(b, name, where, layout, how=None):
    """Feeds the tiles of a BLENDS entry as guarded inputs; returns the guarded mats (to be checked after blend())."""
    corners, _, _, tiles, _ = blend_case(name)
    ins = []
    for (img, seam, warped, fed), c in zip(tiles, corners):
        how_ = how or FEEDS[name]
        if how_ == "feed_dilated":
            gi, gs, gw = gin(img, where, layout, "img"), gin(seam, where, layout, "seam_mask"), gin(warped, where, layout, "warped_mask")
            b.feed_dilated(gi.view, gs.view, gw.view, 3, 3, c)
            ins += [gi, gs, gw]
        else:
            gi = gin(img.astype(np.int16) if how_ == "feed" else img, where, layout, "img")
            gm = gin(fed, where, layout, "mask")
            getattr(b, how_)(gi.view, gm.view, c)
            ins += [gi, gm]
    return ins


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("prec", [I16, F32, F16])
def test_multiband_blend(gpu, oracle, prec, deferred, where, layout):
    """isx_blender_blend of a multi-band blender, eager and deferred cycle: dst (CV_16SC3, CV_32FC3 in the float precisions, CV_8UC3)
    and dst_mask; the tiles and masks fed through isx_blender_feed / _feed_u8 / _feed_dilated are inputs, checked after blend()."""
    for name in BLENDS:
        corners, sizes, bands, _, _ = blend_case(name)
        outs = [("int16", False)] + ([("float32", True)] if prec != I16 else []) + [("uint8", False)]
        for dt, f32 in outs:
            od, om = blend_want(name, "mb", prec, f32)
            if dt == "uint8":
                od = np.clip(od, 0, 255).astype(np.uint8)            # result.convertTo(CV_8U), as tests/test_gpu_blend.py
            b = gpu.MultiBandBlender(False, bands, prec)
            b.set_deferred_level0(deferred)
            b.prepare(corners, sizes)
            ins = feed_guarded(b, name, where, layout)
            assert b.result_size() == (od.shape[1], od.shape[0])
            d, dm = gout(od.shape, dt, where, layout, "dst"), gout(om.shape, np.uint8, where, layout, "dst_mask")
            b.blend(d.view, dm.view)
            sync()
            assert b.last_path()["cycle"] == ("deferred" if deferred else "eager")
            equal(d, od, (name, prec, deferred, dt)), equal(dm, om)
            d.check(), dm.check()
            unchanged(*ins)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", ["feather", "no"])
def test_feather_and_no_blend(gpu, oracle, kind, where, layout):
    """isx_blender_blend of the FeatherBlender and of Blender::NO, eager and with private copies (deferred mode 2)."""
    for name in BLENDS:
        corners, sizes, _, _, _ = blend_case(name)
        od, om = blend_want(name, kind)
        for mode in (False, "copy"):
            b = gpu.FeatherBlender(False, 0.1) if kind == "feather" else gpu.NoBlender()
            b.set_deferred_level0(mode)
            b.prepare(corners, sizes)
            ins = feed_guarded(b, name, where, layout)
            d, dm = gout(od.shape, np.int16, where, layout, "dst"), gout(om.shape, np.uint8, where, layout, "dst_mask")
            b.blend(d.view, dm.view)
            sync()
            equal(d, od, (name, kind, mode)), equal(dm, om)
            d.check(), dm.check()
            unchanged(*ins)


def windows(gpu_blender, oracle_blender, seed_, where, layout):
    """isx_blender_set_window on the deferred cycle of gpu_blender(): every window's columns against the oracle's whole blend."""
    rng = np.random.default_rng(seed_)
    corners, sizes = [(0, 0), (131, 1)], [(170, 17), (170, 16)]
    tiles = [(img_u8(rng, h, w), (rng.random((h, w)) > 0.2).astype(np.uint8) * 255) for w, h in sizes]
    ob = oracle_blender
    ob.prepare(corners, sizes)
    for (img, m), c in zip(tiles, corners):
        ob.feed(img.astype(np.int16), m, c)
    od, om = ob.blend()
    fw = od.shape[1]
    assert fw == 301 and od.shape[0] == 17
    for x0, x1 in ((0, 128), (128, 256), (256, 384), (128, 384)):
        b = gpu_blender()
        b.set_deferred_level0(True)
        b.set_window(x0, x1)
        b.prepare(corners, sizes)
        ins = []
        for (img, m), c in zip(tiles, corners):
            gi, gm = gin(img, where, layout, "img"), gin(m, where, layout, "mask")
            b.feed_u8(gi.view, gm.view, c)
            ins += [gi, gm]
        d, dm = gout((17, x1 - x0, 3), np.int16, where, layout, "dst"), gout((17, x1 - x0), np.uint8, where, layout, "dst_mask")
        b.blend(d.view, dm.view)
        sync()
        n = min(x1, fw) - x0
        assert np.array_equal(d.get()[:, :n], od[:, x0:x0 + n]) and np.array_equal(dm.get()[:, :n], om[:, x0:x0 + n]), (x0, x1)
        d.check(written=(0, n)), dm.check(written=(0, n))
        unchanged(*ins)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("prec", [I16, F32])
def test_blender_window(gpu, oracle, prec, where, layout):
    """isx_blender_set_window: the mats are the window's width; only the columns that lie inside the result are written."""
    windows(lambda: gpu.MultiBandBlender(False, 3, prec), oracle.MultiBand(3, prec), 8, where, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_feather_blender_window(gpu, oracle, where, layout):
    """... and of a deferred FeatherBlender."""
    windows(lambda: gpu.FeatherBlender(False, 0.1), oracle.Feather(0.1), 9, where, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("prec", [I16, F32, F16])
def test_blend_batch_of_two_sizes(gpu, oracle, prec, where, layout):
    """isx_blender_blend_batch over two blenders of different sizes (deferred cycles of one precision and band count share a chain)."""
    from imagestitch_amd.blender import blend_batch
    names = ("two_bands", "tiny")
    bs, ds, dms, ins, want = [], [], [], [], []
    for name in names:
        corners, sizes, bands, _, _ = blend_case(name)
        b = gpu.MultiBandBlender(False, bands, prec)
        b.set_deferred_level0(True)
        b.prepare(corners, sizes)
        ins += feed_guarded(b, name, where, layout, how="feed_u8")
        od, om = blend_want(name, "mb", prec, False)
        bs.append(b), want.append((od, om))
        ds.append(gout(od.shape, np.int16, where, layout, "dst")), dms.append(gout(om.shape, np.uint8, where, layout, "dst_mask"))
    blend_batch(bs, [d.view for d in ds], [m.view for m in dms])
    sync()
    for d, dm, (od, om) in zip(ds, dms, want):
        equal(d, od, prec), equal(dm, om)
        d.check(), dm.check()
    unchanged(*ins)


# ---- the small calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_mask_dilate_and(gpu, oracle, where, layout):
    rng = np.random.default_rng(9)
    for (w, h), (kw, kh), with_other in zip(SHAPES, [(3, 3), (20, 20), (5, 1), (1, 7), (33, 33)] * 2, [True, False] * 5):
        mask = (rng.random((h, w)) > 0.8).astype(np.uint8) * 255
        other = (rng.random((h, w)) > 0.2).astype(np.uint8) * 255
        want = oracle.dilate_rect(mask, kw, kh) & (other if with_other else 255)
        gm, go = gin(mask, where, layout, "mask"), gin(other, where, layout, "other") if with_other else None
        d = gout((h, w), np.uint8, where, layout, "out")
        _lib.check(_lib.load().isx_mask_dilate_and(ref(gm), ref(go), kw, kh, ref(d), 0, None))
        sync()
        equal(d, want.astype(np.uint8), (w, h, kw, kh))
        d.check()
        unchanged(gm, go)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_gain_apply_in_place(gpu, oracle, where, layout):
    rng = np.random.default_rng(10)
    for (w, h), cn, gain in zip(SHAPES, [3, 1, 3] * 3, [1.37, 0.61, 2.5] * 3):
        img = img_u8(rng, h, w, cn)
        g = gin(img, where, layout, "image")
        gpu.gain_apply(g.view, gain)
        sync()
        equal(g, oracle.gain_apply(img, gain), (w, h, cn))
        g.check()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_convert_to_every_pair(gpu, oracle, where, layout):
    """isx_convert_to: every pair of the CV_8U / CV_16S / CV_32F depths that isx_mat types exist for (3 channels: all six; 1 channel:
    CV_8UC1 <-> CV_32FC1)."""
    rng = np.random.default_rng(11)
    pairs = [(np.uint8, np.int16, 3), (np.uint8, np.float32, 3), (np.int16, np.uint8, 3), (np.int16, np.float32, 3), (np.float32, np.uint8, 3),
             (np.float32, np.int16, 3), (np.uint8, np.float32, 1), (np.float32, np.uint8, 1)]
    for sd, dd, cn in pairs:
        for w, h in SHAPES3 + [(1, 1), (63, 5)]:
            shape = (h, w, cn) if cn > 1 else (h, w)
            if sd == np.float32:
                src = ((rng.random(shape) - 0.5) * (70000 if dd == np.int16 else 600)).astype(np.float32)
                src.reshape(-1)[0] = 2.5                          # a tie
                want = oracle.convert_f32(src, dd)
            elif sd == np.int16:
                src = rng.integers(-32768, 32768, shape).astype(np.int16)
                want = np.clip(src, 0, 255).astype(np.uint8) if dd == np.uint8 else src.astype(np.float32)
            else:
                src = rng.integers(0, 256, shape, dtype=np.uint8)
                want = src.astype(dd)
            s, d = gin(src, where, layout, "src"), gout(shape, dd, where, layout, "dst")
            gpu.convert_to(s.view, dd, dst=d.view)
            sync()
            equal(d, want, (sd, dd, cn, w, h))
            d.check()
            unchanged(s)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("u8", [False, True])
def test_seam_gradients(gpu, u8, where, layout):
    rng = np.random.default_rng(12 + u8)
    H, W = 23, 300
    img = img_u8(rng, H, W) if u8 else (rng.random((H, W, 3)) * 255).astype(np.float32)
    gx_all, gy_all = M.gradients(img)
    s = gin(img, where, layout, "image")
    for k, (w, h) in enumerate(SHAPES):
        x, y = (0, 0) if k % 3 == 0 else ((W - w, H - h) if k % 3 == 1 else (7, 2))
        ox, oy = gout((h, w), np.float32, where, layout, "abs_gradx"), gout((h, w), np.float32, where, layout, "abs_grady")
        gpu.seam_gradients(s.view, (x, y, w, h), out=(ox.view, oy.view))
        sync()
        equal(ox, np.ascontiguousarray(np.abs(gx_all)[y:y + h, x:x + w]), (x, y, w, h))
        equal(oy, np.ascontiguousarray(np.abs(gy_all)[y:y + h, x:x + w]), (x, y, w, h))
        ox.check(), oy.check()
    unchanged(s)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_seam_estimate(gpu, oracle, where, layout):
    """isx_seam_estimate and isx_seam_estimate_cost write no mat: the two images and the label image are inputs."""
    lib = _lib.load()
    for seed_, u8, horizontal in ((0, False, False), (1, True, True), (2, False, True)):
        c = make_case(seed_, size1=(33, 67), size2=(35, 65), tl1=(-9, 2), tl2=(25, -3), u8=u8, horizontal=horizontal)
        args = (c["img1"], c["img2"], c["tl1"], c["tl2"], c["union_tl"], c["labels"], c["label"], c["roi"], c["p1"], c["p2"])
        g1, g2, gl = gin(c["img1"], where, layout, "image1"), gin(c["img2"], where, layout, "image2"), gin(c["labels"], where, layout, "labels")
        want, wh = oracle.seam_estimate(*args)
        cap = c["roi"][2] + c["roi"][3] + 2
        out, n, horiz = np.zeros((cap, 2), np.int32), C.c_int(0), C.c_int(0)
        _lib.check(lib.isx_seam_estimate(ref(g1), ref(g2), c["tl1"][0], c["tl1"][1], c["tl2"][0], c["tl2"][1], c["union_tl"][0], c["union_tl"][1], ref(gl),
                                         c["label"], (C.c_int * 4)(*c["roi"]), c["p1"][0], c["p1"][1], c["p2"][0], c["p2"][1],
                                         out.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n), C.byref(horiz), 0, None))
        sync()
        assert bool(horiz.value) == wh and np.array_equal(out[:n.value], want) and len(want) > 0
        unchanged(g1, g2, gl)
        for cf, model_cf in ((gpu.DP_COLOR, M.COLOR), (gpu.DP_COLOR_GRAD, M.COLOR_GRAD)):
            mw, mh = M.seam_estimate(*args, model_cf)
            got, gh = gpu.seam_estimate(g1.view, g2.view, *args[2:5], gl.view, *args[6:], cost_func=cf)
            sync()
            assert gh == mh and np.array_equal(got, mw), cf
            unchanged(g1, g2, gl)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_blend_pair_linear(gpu, oracle, where, layout):
    rng = np.random.default_rng(13)
    for (h1, w1, h2, w2, dx, dy) in ((17, 67, 19, 65, 40, 3), (5, 63, 4, 64, 30, -1), (33, 130, 33, 131, 126, 0)):
        img1 = (rng.random((h1, w1, 3)) * 255).astype(np.float32)
        img2 = (rng.random((h2, w2, 3)) * 255).astype(np.float32)
        img1[:3, -9:] = 3.0
        img2[-2:, :7] = 2.0
        tl1, tl2 = (10, 20), (10 + dx, 20 + dy)
        rc, opano, oseam = oracle.blend_pair_linear(img1, img2, tl1, tl2)
        assert rc == 0
        g1, g2 = gin(img1, where, layout, "images1"), gin(img2, where, layout, "images2")
        d = gout(opano.shape, np.float32, where, layout, "pano")
        seam_x = np.zeros(opano.shape[0], np.int32)
        _lib.check(_lib.load().isx_blend_pair_linear(ref(g1), ref(g2), tl1[0], tl1[1], tl2[0], tl2[1], ref(d), seam_x.ctypes.data_as(_lib._IP), 0, None))
        sync()
        assert np.array_equal(seam_x, oseam)
        equal(d, opano, (h1, w1, h2, w2))
        d.check()
        unchanged(g1, g2)


# ---- the finders and the gain feed ---------------------------------------------------------------------------------------------------
def small_layout(n, seed_):
    """n overlapping tiles whose sizes come from the shape classes (a partial 64-column block, a partial group, odd heights)."""
    rng = np.random.default_rng(seed_)
    sizes = [(67, 17), (65, 21), (63, 19), (70, 5)][:n]
    corners = [(0, 0), (31, -3), (-20, 6), (10, 9)][:n]
    imgs, masks = [], []
    for w, h in sizes:
        base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3))
        img = np.kron(base, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(0, 12, (h, w, 3))
        imgs.append(np.clip(img, 0, 255).astype(np.uint8))
        m = np.full((h, w), 255, np.uint8)
        y, x = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 4))
        m[y:y + 3, x:x + 4] = 0
        masks.append(m)
    return corners, imgs, masks


def run_finder(call, images, masks, want, where, layout, mixed=False):
    """call(images or None, masks) on guarded mats; the masks are in place and compared whole, the images are inputs."""
    res = [("device" if k == 1 else "host") if mixed else where for k in range(len(masks))]
    gi = [gin(a, r, layout, "image%d" % k) for k, (a, r) in enumerate(zip(images, res))] if images is not None else []
    gm = [gin(m, r, layout, "mask%d" % k) for k, (m, r) in enumerate(zip(masks, res))]
    call([g.view for g in gi], [g.view for g in gm])
    sync()
    for k, (g, w) in enumerate(zip(gm, want)):
        equal(g, w, k)
        g.check()
    unchanged(*gi)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE + ("mixed",))
@pytest.mark.parametrize("cost", ["color", "color_grad"])
def test_dp_seam_find(gpu, cost, where, layout):
    """isx_dp_seam_find_cost (COLOR and COLOR_GRAD) and isx_dp_seam_find."""
    lib = _lib.load()
    for n, u8, size in ((2, True, (33, 67)), (3, False, (21, 65))):
        images, corners, masks = make_find_case(50 + n, n, u8, holes=True, size=size)
        want = [m.copy() for m in masks]
        M.DpSeamFinder(M.COLOR if cost == "color" else M.COLOR_GRAD).find(images, corners, want)
        assert any((a != b).any() for a, b in zip(want, masks))
        cf = gpu.DP_COLOR if cost == "color" else gpu.DP_COLOR_GRAD
        run_finder(lambda gi, gm: gpu.DpSeamFinder(cf).find(gi, corners, gm), images, masks, want, where, layout, where == "mixed")
        if cost == "color":
            def old(gi, gm):
                cnt, mi, c, mm, ptr = _lib.tile_args(gi, corners, gm, None)
                _lib.check(lib.isx_dp_seam_find(cnt, mi, c, mm, 0, ptr))
            run_finder(old, images, masks, want, where, layout, where == "mixed")


_GRAD_WANT = {}


def _grad_want(n, seed_):
    """The COST_COLOR_GRAD model's masks of small_layout(n, seed_): solved once for all the parametrised cases, never edited."""
    if (n, seed_) not in _GRAD_WANT:
        corners, imgs, masks = small_layout(n, seed_)
        _GRAD_WANT[(n, seed_)] = GCG.find(imgs, corners, [m.copy() for m in masks])
    return _GRAD_WANT[(n, seed_)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE + ("mixed",))
def test_graphcut_seam_find(gpu, where, layout):
    """isx_graphcut_seam_find and isx_graphcut_seam_find_pair; the model's masks as tests/test_gpu_graphcut_seam.py takes them (scipy)."""
    import scipy  # noqa: F401  (helpers/graphcut_np.py needs it: an explicit dependency of this test, not a skip)
    for n, seed_, f32 in ((2, 1, False), (3, 2, True)):
        corners, imgs, masks = small_layout(n, seed_)
        want = [m.copy() for m in masks]
        GC.find(imgs, corners, want)
        assert any((a != b).any() for a, b in zip(want, masks))
        src = [a.astype(np.float32) for a in imgs] if f32 else imgs
        run_finder(lambda gi, gm: gpu.GraphCutSeamFinder().find(gi, corners, gm), src, masks, want, where, layout, where == "mixed")
    corners, imgs, masks = small_layout(2, 1)
    want = [m.copy() for m in masks]
    GC.find(imgs, corners, want)
    run_finder(lambda gi, gm: gpu.GraphCutSeamFinder().find_pair(gi[0], gi[1], corners[0], corners[1], gm[0], gm[1]), imgs, masks, want, where, layout,
               where == "mixed")
    # COST_COLOR_GRAD (CV_32FC3: three row pointers per tile in the build kernel) through find(), and isx_graphcut_seam_find_pair64 with its
    # certificate, which is checked against the model's Q23 graph
    for n, seed_ in ((2, 1), (3, 2)):
        corners, imgs, masks = small_layout(n, seed_)
        want = _grad_want(n, seed_)
        assert any((a != b).any() for a, b in zip(want, masks))
        run_finder(lambda gi, gm: gpu.GraphCutSeamFinder(cost_type=GCG.COST_COLOR_GRAD).find(gi, corners, gm), [a.astype(np.float32) for a in imgs], masks,
                   want, where, layout, where == "mixed")
    corners, imgs, masks = small_layout(2, 1)
    want = _grad_want(2, 1)
    sizes = [(a.shape[1], a.shape[0]) for a in imgs]
    graph = GCG.pair_graph(imgs[0], imgs[1], masks[0], masks[1], corners[0], corners[1], GC.overlap_roi(corners[0], corners[1], sizes[0], sizes[1]))

    def pair64(gi, gm):
        r = gpu.GraphCutSeamFinder(cost_type=GCG.COST_COLOR_GRAD).find_pair(gi[0], gi[1], corners[0], corners[1], gm[0], gm[1], certificate=True)
        assert r["residuals"].dtype == np.int64
        GC.check_certificate(graph, r["flow"], r["residuals"], r["labels"])
    run_finder(pair64, [a.astype(np.float32) for a in imgs], masks, want, where, layout, where == "mixed")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE + ("mixed",))
def test_voronoi_seam_find(gpu, where, layout):
    for n, seed_ in ((2, 1), (3, 2), (4, 3)):
        corners, _, masks = small_layout(n, seed_)
        sizes = [(m.shape[1], m.shape[0]) for m in masks]
        want = [m.copy() for m in masks]
        V.find(sizes, corners, want)
        assert any((a != b).any() for a, b in zip(want, masks))
        run_finder(lambda gi, gm: gpu.VoronoiSeamFinder().find(sizes, corners, gm), None, masks, want, where, layout, where == "mixed")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE + ("mixed",))
def test_gain_compensator_feed_takes_inputs_only(gpu, where, layout):
    for n, seed_ in ((2, 1), (4, 3)):
        corners, imgs, masks = small_layout(n, seed_)
        for m in masks:
            m[::3, ::5] = 254                                        # not 255: outside the overlap count
        N, I, _, _, _, g = feed_model(corners, imgs, masks)
        res = [("device" if k == 1 else "host") if where == "mixed" else where for k in range(n)]
        gi = [gin(a, r, layout, "image%d" % k) for k, (a, r) in enumerate(zip(imgs, res))]
        gm = [gin(m, r, layout, "mask%d" % k) for k, (m, r) in enumerate(zip(masks, res))]
        comp = gpu.GainCompensator().feed(corners, [x.view for x in gi], [x.view for x in gm])
        sync()
        assert np.array_equal(comp.N, N) and np.array_equal(comp.I.view(np.uint64), I.view(np.uint64))
        np.testing.assert_allclose(comp.gains(), g, rtol=1e-12, atol=0)
        unchanged(*gi, *gm)


# ---- BlocksGainCompensator ---------------------------------------------------------------------------------------------------------------
_blocks_gain = {}


def blocks_gain_case():
    """The two tiles of the finder rows (67 x 17 and 65 x 21) in blocks of 32 x 8: 3 x 3 blocks each; the model, and a rtol of the gains by the
    forward-error rule of tests/blocks_gain_cases.py.  Computed once per module."""
    if "case" not in _blocks_gain:
        from blocks_gain_cases import forward_error_rtol      # (tools/fuzz_parity.py's bg_forward_error_rtol)
        corners, imgs, masks = small_layout(2, 1)
        for m in masks:
            m[::3, ::5] = 254                                        # not 255: outside the counts
        model = BG.feed_blocks_model(corners, imgs, masks, 32, 8)
        assert model["counts"] == [(3, 3), (3, 3)] and len(model["pairs"]) > 4
        _blocks_gain["case"] = (corners, imgs, masks, model, forward_error_rtol(model["A"], model["b"], model["gains"])[0])
    return _blocks_gain["case"]


def blocks_gain_fed(gpu):
    """One handle fed with blocks_gain_case(), for the rows that only read it."""
    if "fed" not in _blocks_gain:
        corners, imgs, masks, _, _ = blocks_gain_case()
        comp = gpu.BlocksGainCompensator(32, 8).feed(corners, imgs, masks)
        _blocks_gain["fed"] = (comp, comp.gain_maps())
    return _blocks_gain["fed"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE + ("mixed",))
def test_blocks_gain_feed_takes_inputs_only(gpu, where, layout):
    """isx_blocks_gain_feed: the images and the masks are inputs."""
    corners, imgs, masks, model, rtol = blocks_gain_case()
    res = [("device" if k == 1 else "host") if where == "mixed" else where for k in range(2)]
    gi = [gin(a, r, layout, "image%d" % k) for k, (a, r) in enumerate(zip(imgs, res))]
    gm = [gin(m, r, layout, "mask%d" % k) for k, (m, r) in enumerate(zip(masks, res))]
    comp = gpu.BlocksGainCompensator(32, 8).feed(corners, [x.view for x in gi], [x.view for x in gm])
    sync()
    pairs, diag = comp.block_stats()
    assert comp.block_counts() == model["counts"] and np.array_equal(diag, model["diag_n"])
    assert [(int(p["block_i"]), int(p["block_j"]), int(p["n"])) for p in pairs] == [p[:3] for p in model["pairs"]]
    assert np.array_equal(pairs["i_ij"].view(np.uint64), np.array([p[3] for p in model["pairs"]]).view(np.uint64))
    assert np.array_equal(pairs["i_ji"].view(np.uint64), np.array([p[4] for p in model["pairs"]]).view(np.uint64))
    np.testing.assert_allclose(comp.gains(), model["gains"], rtol=rtol, atol=0)
    unchanged(*gi, *gm)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_blocks_gain_apply_in_place(gpu, where, layout):
    """isx_blocks_gain_apply: the 3 x 3 maps resized to every shape; the image's bytes are the model's and not one byte beside them."""
    comp, gmaps = blocks_gain_fed(gpu)
    rng = np.random.default_rng(15)
    for k, (w, h) in enumerate(SHAPES):
        img = img_u8(rng, h, w)
        g = gin(img, where, layout, "image")
        comp.apply(k % 2, (0, 0), g.view)
        sync()
        equal(g, BG.apply_model(img, gmaps[k % 2]), (w, h))
        g.check()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_blocks_gain_map(gpu, where, layout):
    """isx_blocks_gain_map: the smoothed map into the caller's CV_32FC1 mat."""
    comp, _ = blocks_gain_fed(gpu)
    counts = comp.block_counts()
    for i, want in enumerate(BG.maps_from_gains(comp.gains(), counts)):
        d = gout(want.shape, np.float32, where, layout, "map")
        _lib.check(_lib.load().isx_blocks_gain_map(comp._h, i, ref(d), None))
        sync()
        equal(d, want, i)
        d.check()


# ---- image files ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", WHERE)
def test_image_files(gpu, where, layout, tmp_path):
    """isx_bmp_write / isx_jpeg_write read their mat, isx_bmp_read / isx_jpeg_read fill the caller's: a .bmp comes back as written; a
    .jpg comes back as the package's own imread gives it into an ordinary array (the decoder's parity has tests/test_imgio.py)."""
    import imagestitch_amd as I
    lib = _lib.load()
    rng = np.random.default_rng(14)
    for w, h in SHAPES3 + [(1, 1), (63, 5)]:
        img = np.kron(img_u8(rng, h // 4 + 1, w // 4 + 1), np.ones((4, 4, 1), np.uint8))[:h, :w]
        for ext in ("bmp", "jpg"):
            path = str(tmp_path / ("t_%d_%d.%s" % (w, h, ext))).encode()
            s = gin(img, where, layout, "img")
            _lib.check(lib.isx_bmp_write(path, ref(s)) if ext == "bmp" else lib.isx_jpeg_write(path, ref(s), 90))
            sync()
            unchanged(s)
            want = img if ext == "bmp" else np.asarray(I.imread(path.decode()))
            d = gout((h, w, 3), np.uint8, where, layout, "out")
            _lib.check(lib.isx_bmp_read(path, ref(d)) if ext == "bmp" else lib.isx_jpeg_read(path, ref(d)))
            sync()
            equal(d, want, (w, h, ext))
            d.check()


# ---- the helper itself, on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_stray_device_store_is_found(gpu, layout):
    """tests/test_guarded_helper.py on a device buffer: stores made with torch just outside the view, and inside it outside `written`."""
    for dtype, cn in ((np.uint8, 3), (np.int16, 3), (np.float32, 1)):
        h, w = 5, 67
        probe = gout((h, w, cn) if cn > 1 else (h, w), dtype, "device", layout)
        m = mat(probe)
        assert m.data == probe.buf.data_ptr() + probe.offset and m.step == probe.pitch and m.device == 0
        assert (m.data % 256 == 0 and m.step % 64 == 0) if layout == "aligned" else (m.data % (4 if dtype == np.uint8 else 16) != 0)
        row0 = probe.first + G.ROWS_ABOVE * probe.pitch
        for i, region in ((probe.nbytes - 1, "below"), (row0 + probe.lead + probe.row_bytes, "pad"), (row0 + probe.pitch + probe.lead - 1, "lead"),
                          (row0 - probe.pitch + probe.lead, "above"), (row0 + h * probe.pitch + probe.lead, "below")):
            g = gout(probe.shape, dtype, "device", layout)
            g.check(), g.check(G.NOTHING)
            g.buf[i] ^= 0x5A
            with pytest.raises(G.GuardError) as e:
                g.check()
            assert e.value.region == region
        g = gout(probe.shape, dtype, "device", layout)
        g.view[:, 3:5] += 1
        g.check(), g.check((3, 5))
        for written in (G.NOTHING, (3, 4), (4, 5)):
            with pytest.raises(G.GuardError) as e:
                g.check(written)
            assert e.value.region == "view"
