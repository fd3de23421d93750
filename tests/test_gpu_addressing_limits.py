"""Every threshold between a fast kernel (32-bit byte offsets from 24-bit multiplies), the generic size_t kernel and ISX_ERR_UNSUPPORTED, from
both sides: a row pitch of 2^24 bytes, a source span step * rows of 2^31, a destination span of 2^32, 32767 pixels a side (DESIGN.md
"Addressing limits" lists the predicates and the case that straddles each).  One operand of a call lies in a large-pitch guarded mat
(tests/helpers/guarded_wide.py: a wrong offset lands inside the test's own allocation and is found there), every other mat in an
ordinary one (tests/helpers/guarded.py).  Every case compares with the oracle byte for byte, checks that outputs have only their view
written and inputs not one byte, and asserts which path ran: the launch names of isx_profile_entry for the warper,
isx_blender_last_path / _feed_path / _level1_format for the blender.  Shapes are the smallest that reach a path: tiles 24-70 pixels
wide, 8-24 rows on the wide layouts, 255 / 256 / 257 and 511 / 512 rows on the tall ones."""
import ctypes as C
import gc
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_guard_bands as GB  # noqa: E402  (its rig, maps, models and seeds)
from helpers import guarded as G  # noqa: E402
from helpers import guarded_wide as W  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

CYL = 0
NEAREST, LINEAR = 0, 1
CONST, REFLECT = 0, 2
I16, F32, F16 = 0, 1, 2
UNSUPPORTED = 6
P24 = 1 << 24
BELOW = P24 - 64                                            # "tall32" at 256 / 257 rows
# (kind, source w, source h, focal) -> detectResultRoi's (w, h) under GB.rig(): searched on the CPU oracle, asserted in cam()
SMALL = (CYL, 67, 17, 90.0)
CAMERAS = {SMALL: (64, 17), (CYL, 67, 17, 70.0): (62, 17), (CYL, 24, 255, 80.0): (28, 256), (CYL, 24, 255, 70.0): (28, 257),
           (CYL, 24, 256, 105.0): (28, 256), (CYL, 24, 505, 117.5): (34, 511), (CYL, 24, 505, 110.0): (33, 512)}
S255_D256, S255_D257, S256_D256, D511, D512 = (CYL, 24, 255, 80.0), (CYL, 24, 255, 70.0), (CYL, 24, 256, 105.0), (CYL, 24, 505, 117.5), (CYL, 24, 505, 110.0)
seed, sync, equal, unchanged = GB.seed, GB.sync, GB.equal, GB.unchanged


def mat(g):
    return _lib.as_mat(g.view if isinstance(g, (G.Guarded, W.WideGuarded)) else g)


def ref(g):
    return C.byref(mat(g)) if g is not None else None


@pytest.fixture(autouse=True)
def own_seeds(request):
    GB._seed[0] = zlib.crc32(request.node.name.encode()) << 16


@pytest.fixture(scope="module", autouse=True)
def release_the_large_buffers():
    yield
    import torch
    torch.cuda.empty_cache()


def big(shape, dtype, spec, name, content=None):
    """A device mat per spec = (layout, pitch or None); spec None: an ordinary guarded one.  A tall layout skips only when the device
    has less free memory than the mat needs plus 2 GiB."""
    if spec is None:
        g = G.guarded(shape, dtype, "device", "aligned" if seed() % 2 else "odd", seed(), name)
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
        g = W.wide_guarded(shape, dtype, layout, seed(), name, pitch)
        if layout.startswith("wide"):
            assert 8 <= shape[0] <= 24 and g.nbytes <= 420 << 20, (layout, shape, g.nbytes)      # 8-24 rows, about 400 MiB at most
        m = mat(g)
        assert m.step == g.pitch and m.rows == shape[0] and m.data == g.view.data_ptr()
    return g.set(content) if content is not None else g


class launches:
    """with launches() as l: ...; l.names = the launch names of the calls inside (isx_profile_entry)."""

    def __enter__(self):
        lib = _lib.load()
        lib.isx_profile_enable(1); lib.isx_profile_filter(None); lib.isx_profile_sample(1); lib.isx_profile_reset()
        self.names = None
        return self

    def __exit__(self, *exc):
        try:
            self.names = set(_lib.profile_entries()) if exc[0] is None else set()
        finally:
            _lib.load().isx_profile_enable(0)
        return False


def refused(call):
    with pytest.raises(_lib.IsxError) as e:
        call()
    assert e.value.code == UNSUPPORTED, e.value
    del e       # the info holds the traceback, which holds this frame and the caller's: dropped here, they keep no blender alive until a collection


# ---- warper --------------------------------------------------------------------------------------------------------------------------
_cams = {}


def cam(oracle, key):
    """Rig, ROI and the oracle's warps of one CAMERAS entry (computed once): a CV_8UC3 image LINEAR / REFLECT, a CV_8UC1 image NEAREST /
    CONSTANT, the all-255 mask."""
    if key not in _cams:
        kind, w, h, f = key
        K, R = GB.rig(w, h, f)
        roi, xm, ym = GB.maps(oracle, kind, f, K, R, w, h)
        assert (xm.shape[1], xm.shape[0]) == CAMERAS[key], (key, xm.shape)          # the side of 256 / 257 / 512 rows the case is named for
        rng = np.random.default_rng(len(_cams) + 40)
        img, grey = GB.img_u8(rng, h, w), GB.img_u8(rng, h, w, 1)
        _cams[key] = dict(K=K, R=R, roi=roi, f=f, img=img, grey=grey, wi=oracle.remap(img, xm, ym, LINEAR, REFLECT),
                          wg=oracle.remap(grey, xm, ym, NEAREST, CONST), wm=oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, NEAREST, CONST))
    return _cams[key]


# operand, (layout, pitch), camera, on the fast side
WARP_CASES = {
    "src_pitch_below": ("src", ("wide_below", None), SMALL, True), "src_pitch_2p24": ("src", ("wide", None), SMALL, False),
    "src_pitch_2p24_64": ("src", ("wide", P24 + 64), SMALL, False),
    "src_span_255": ("src", ("tall31", None), S255_D256, True), "src_span_256": ("src", ("tall31", None), S256_D256, False),
    "dst_pitch_below": ("dst", ("wide_below", None), SMALL, True), "dst_pitch_2p24": ("dst", ("wide", None), SMALL, False),
    "dst_pitch_2p24_64": ("dst", ("wide", P24 + 64), SMALL, False),
    "dst_span_256": ("dst", ("tall32", BELOW), S255_D256, True), "dst_span_257": ("dst", ("tall32", BELOW), S255_D257, False),
    "dst_span_511": ("dst", ("tall32", None), D511, True), "dst_span_512": ("dst", ("tall32", None), D512, False),
}


@pytest.mark.parametrize("case", list(WARP_CASES))
@pytest.mark.parametrize("what", ["img", "mask"])
def test_warp_tile_kernel_below_each_limit_generic_kernel_past_it(gpu, oracle, what, case):
    """isx_warper_warp, the two calls the reference makes per tile (CV_8UC3 LINEAR / REFLECT, CV_8UC1 NEAREST / CONSTANT): k_warp_tile /
    k_warp_mask_tile while the source's and the destination's pitch and span are below their limits, the generic k_warp from the limit on
    (the `!small` leg) - the oracle's bytes on either side."""
    operand, spec, key, fast = WARP_CASES[case]
    c = cam(oracle, key)
    src, want, interp, border = (c["img"], c["wi"], LINEAR, REFLECT) if what == "img" else (c["grey"], c["wg"], NEAREST, CONST)
    s = big(src.shape, np.uint8, spec if operand == "src" else None, "src", src)
    d = big(want.shape, np.uint8, spec if operand == "dst" else None, "dst")
    warper = GB.make_warper(gpu, key[0], c["f"])
    with launches() as l:
        corner, _ = warper.warp(s.view, c["K"], c["R"], interp, border, dst=d.view)
    assert corner == c["roi"][:2]
    tile = "warp_tile_img" if what == "img" else "warp_tile_mask"
    assert l.names & {"warp_tile_img", "warp_tile_mask", "warp", "warp_tile"} == {tile if fast else "warp"}, l.names
    equal(d, want, case)
    d.check()
    unchanged(s)


@pytest.mark.parametrize("w,h", [(32768, 2), (2, 32768)])
def test_warp_source_of_32768_pixels_a_side(gpu, oracle, w, h):
    """cols, rows <= 32767 is the tile kernels' limit (short source coordinates): one pixel past it isx_warper_warp takes k_warp."""
    f = 40.0
    K, R = GB.rig(w, h, f)
    roi, xm, ym = GB.maps(oracle, CYL, f, K, R, w, h)
    rng = np.random.default_rng(w)
    warper = GB.make_warper(gpu, CYL, f)
    for src, interp, border in ((GB.img_u8(rng, h, w), LINEAR, REFLECT), (GB.img_u8(rng, h, w, 1), NEAREST, CONST)):
        want = oracle.remap(src, xm, ym, interp, border)
        s, d = big(src.shape, np.uint8, None, "src", src), big(want.shape, np.uint8, None, "dst")
        with launches() as l:
            corner, _ = warper.warp(s.view, K, R, interp, border, dst=d.view)
        assert corner == roi[:2] and l.names & {"warp_tile_img", "warp_tile_mask", "warp"} == {"warp"}, l.names
        equal(d, want, (w, h, interp))
        d.check()
        unchanged(s)
    # one pixel less: the tile kernels
    src = GB.img_u8(rng, h - (h > w), w - (w > h))
    hh, ww = src.shape[:2]
    K, R = GB.rig(ww, hh, f)
    roi, xm, ym = GB.maps(oracle, CYL, f, K, R, ww, hh)
    want = oracle.remap(src, xm, ym, LINEAR, REFLECT)
    s, d = big(src.shape, np.uint8, None, "src", src), big(want.shape, np.uint8, None, "dst")
    with launches() as l:
        warper.warp(s.view, K, R, LINEAR, REFLECT, dst=d.view)
    assert l.names & {"warp_tile_img", "warp"} == {"warp_tile_img"}, l.names
    equal(d, want, (ww, hh))
    d.check()
    unchanged(s)


def test_remap_refuses_a_source_of_32768_columns(gpu, oracle):
    """isx_remap keeps cv::remap's short coordinates: 32768 columns are ISX_ERR_UNSUPPORTED and dst stays as it is; 32767 are remapped."""
    rng = np.random.default_rng(7)
    xm = (rng.random((4, 5)) * 32900 - 100).astype(np.float32)
    ym = (rng.random((4, 5)) * 4 - 1).astype(np.float32)
    for cols, ok in ((32768, False), (32767, True)):
        src = GB.img_u8(rng, 2, cols, 1)
        s, gx, gy = big(src.shape, np.uint8, None, "src", src), big(xm.shape, np.float32, None, "xmap", xm), big(ym.shape, np.float32, None, "ymap", ym)
        d = big((4, 5), np.uint8, None, "dst")

        def call():
            _lib.check(_lib.load().isx_remap(ref(s), ref(gx), ref(gy), NEAREST, CONST, ref(d), 0, None))
        if ok:
            call()
            sync()
            equal(d, oracle.remap(src, xm, ym, NEAREST, CONST))
            d.check()
        else:
            refused(call)
            sync()
            unchanged(d)
        unchanged(s, gx, gy)


# operand -> ((layout, pitch), camera) on the slow side, the same on the fast side
FUSED_CASES = {
    "src_pitch": ("src", ("wide", None), SMALL, ("wide_below", None), SMALL),
    "src_pitch_64": ("src", ("wide", P24 + 64), SMALL, ("wide_below", None), SMALL),
    "src_span": ("src", ("tall31", None), S256_D256, ("tall31", None), S255_D256),
    "dst_img_pitch": ("dimg", ("wide", None), SMALL, ("wide_below", None), SMALL),
    "dst_img_span": ("dimg", ("tall32", BELOW), S255_D257, ("tall32", BELOW), S255_D256),
    "dst_img_span_2p32": ("dimg", ("tall32", None), D512, ("tall32", None), D511),
    "dst_mask_pitch": ("dmask", ("wide", None), SMALL, ("wide_below", None), SMALL),
    "dst_mask_span": ("dmask", ("tall32", BELOW), S255_D257, ("tall32", BELOW), S255_D256),      # no guard covered this one
    "dst_mask_span_2p32": ("dmask", ("tall32", None), D512, ("tall32", None), D511),              # ... step * rows == 2^32 exactly
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
@pytest.mark.parametrize("out16", [False, True])
def test_warp_with_mask_refuses_past_each_limit(gpu, oracle, out16, case):
    """isx_warper_warp_with_mask and _planned, CV_8UC3 and CV_16SC3 tiles: k_warp_tile has no generic sibling, so each operand in turn on
    the slow side of its limit - source pitch and span, the image's and the MASK's pitch and span - is ISX_ERR_UNSUPPORTED with not one
    byte written; the same call with the operand on the fast side gives the oracle's tile and mask.  The destination mask's span was
    not checked: its rows past 4 GiB were stored on early rows (k_warp_tile: d.mask + (__umul24(dy, d.mask_step) + dx0))."""
    operand, slow, slow_cam, fast, fast_cam = FUSED_CASES[case]
    dt = np.int16 if out16 else np.uint8
    for spec, key, ok in ((slow, slow_cam, False), (fast, fast_cam, True)):
        c = cam(oracle, key)
        s = big(c["img"].shape, np.uint8, spec if operand == "src" else None, "src", c["img"])
        di = big(c["wi"].shape, dt, spec if operand == "dimg" else None, "dst_img")
        dm = big(c["wm"].shape, np.uint8, spec if operand == "dmask" else None, "dst_mask")
        warper = GB.make_warper(gpu, key[0], c["f"])
        for planned in (False, True):
            def call():
                if planned:
                    warper.warp_with_mask_planned(s.view, c["K"], c["R"], c["roi"], di.view, dm.view)
                else:
                    assert warper.warp_with_mask(s.view, c["K"], c["R"], out16=out16, dst_img=di.view, dst_mask=dm.view)[0] == c["roi"][:2]
            with launches() as l:
                if ok:
                    call()
                else:
                    refused(call)
            if ok:
                assert "warp_tile" in l.names, l.names
                equal(di, c["wi"].astype(dt), (case, planned)), equal(dm, c["wm"], (case, planned))
                di.check(), dm.check()
                unchanged(s)
                di.set(np.zeros(di.shape, dt)), dm.set(np.zeros(dm.shape, np.uint8))          # the second entry writes them again
            else:
                assert not l.names & {"warp_tile", "warp_img_mask"}, l.names
                unchanged(s, di, dm)
        assert warper.plan_status() == 0
        del s, di, dm                                                # one tall mat at a time


@pytest.mark.parametrize("operand", ["dimg", "dmask"])
@pytest.mark.parametrize("out16", [False, True])
def test_warp_with_a_source_mask_at_the_destination_span(gpu, oracle, out16, operand):
    """The same with the caller's source mask: k_warp_img_mask (its dword stores at __umul24(dy, step) offsets) writes dst_img, then
    dst_mask, of 256 rows of 2^24 - 64 bytes - the last row starts 16 KiB below 2^32 - and is refused at 257 rows."""
    dt = np.int16 if out16 else np.uint8
    for key, ok in ((S255_D257, False), (S255_D256, True)):
        c = cam(oracle, key)
        h, w = c["img"].shape[:2]
        holes = (np.random.default_rng(h).integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
        _, xm, ym = GB.maps(oracle, key[0], c["f"], c["K"], c["R"], w, h)
        wh = oracle.remap(holes, xm, ym, NEAREST, CONST)
        s, sm = big(c["img"].shape, np.uint8, None, "src", c["img"]), big(holes.shape, np.uint8, None, "src_mask", holes)
        di = big(c["wi"].shape, dt, ("tall32", BELOW) if operand == "dimg" else None, "dst_img")
        dm = big(wh.shape, np.uint8, ("tall32", BELOW) if operand == "dmask" else None, "dst_mask")
        warper = GB.make_warper(gpu, key[0], c["f"])

        def call():
            warper.warp_with_mask(s.view, c["K"], c["R"], mask=sm.view, out16=out16, dst_img=di.view, dst_mask=dm.view)
        with launches() as l:
            if ok:
                call()
            else:
                refused(call)
        if ok:
            assert "warp_img_mask" in l.names and "warp_tile" not in l.names, l.names
            equal(di, c["wi"].astype(dt), operand), equal(dm, wh, operand)
            di.check(), dm.check()
            unchanged(s, sm)
        else:
            assert not l.names & {"warp_tile", "warp_img_mask"}, l.names
            unchanged(s, sm, di, dm)
        del di, dm


@pytest.mark.parametrize("out16", [False, True])
def test_warp_batch_does_not_collect_the_refused_tile(gpu, oracle, out16):
    """isx_warper_begin_batch .. _end_batch: a tile whose destination mask spans 4 GiB is refused when it is issued and never collected;
    the refusal ends the batch, which launches the tile collected before it - that one equals the oracle; a new batch of the two tiles
    with the mask below the limit gives both."""
    dt = np.int16 if out16 else np.uint8
    a, b = cam(oracle, (CYL, 67, 17, 70.0)), cam(oracle, S255_D257)
    assert a["f"] == b["f"]                                          # one handle: its scale is the batch's
    warper = GB.make_warper(gpu, CYL, a["f"])
    sa, sb = big(a["img"].shape, np.uint8, None, "src0", a["img"]), big(b["img"].shape, np.uint8, None, "src1", b["img"])
    da, ma = big(a["wi"].shape, dt, None, "dst_img0"), big(a["wm"].shape, np.uint8, None, "dst_mask0")
    db, mb = big(b["wi"].shape, dt, None, "dst_img1"), big(b["wm"].shape, np.uint8, ("tall32", BELOW), "dst_mask1")
    warper.begin_batch()
    warper.warp_with_mask_planned(sa.view, a["K"], a["R"], a["roi"], da.view, ma.view)
    sync()
    unchanged(sa, da, ma)                                             # collected, not launched
    refused(lambda: warper.warp_with_mask_planned(sb.view, b["K"], b["R"], b["roi"], db.view, mb.view))
    sync()
    equal(da, a["wi"].astype(dt)), equal(ma, a["wm"])
    da.check(), ma.check()
    unchanged(sa, sb, db, mb)
    warper.end_batch()
    sync()
    unchanged(sb, db, mb)
    del mb
    mb = big(b["wm"].shape, np.uint8, None, "dst_mask1")
    da.set(np.zeros(da.shape, dt)), ma.set(np.zeros(ma.shape, np.uint8))
    warper.begin_batch()
    warper.warp_with_mask_planned(sa.view, a["K"], a["R"], a["roi"], da.view, ma.view)
    warper.warp_with_mask_planned(sb.view, b["K"], b["R"], b["roi"], db.view, mb.view)
    warper.end_batch()
    sync()
    for s, d, m, c in ((sa, da, ma, a), (sb, db, mb, b)):
        equal(d, c["wi"].astype(dt)), equal(m, c["wm"])
        d.check(), m.check()
        unchanged(s)
    assert warper.plan_status() == 0


# ---- blender -------------------------------------------------------------------------------------------------------------------------
# name -> (corners, sizes (w, h), bands)
GEOMETRIES = {"r8": ([(0, 0), (26, 0)], [(40, 8)] * 2, 2), "r16": ([(0, 0), (26, 0)], [(40, 16)] * 2, 2), "r255": ([(0, 0), (26, 0)], [(40, 255)] * 2, 2), "r256": ([(0, 0), (26, 0)], [(40, 256)] * 2, 2),
              "r257": ([(0, 0), (26, 0)], [(40, 257)] * 2, 2), "r258": ([(0, 0), (26, 0)], [(40, 258)] * 2, 2), "r511": ([(0, 0), (26, 0)], [(40, 511)] * 2, 2), "r512": ([(0, 0), (26, 0)], [(40, 512)] * 2, 2),
              "w256": ([(0, 0), (60, 0), (120, 0)], [(70, 256)] * 3, 2), "w257": ([(0, 0), (60, 0), (120, 0)], [(70, 257)] * 3, 2)}
KINDS = {"i16": I16, "f32": F32, "f16": F16, "feather": None, "no": None}
_geo = {}


def geometry(name):
    if name not in _geo:
        corners, sizes, bands = GEOMETRIES[name]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        tiles = [(GB.img_u8(rng, h, w), (rng.random((h, w)) > 0.15).astype(np.uint8) * 255) for w, h in sizes]
        _geo[name] = (corners, sizes, bands, tiles, {})
    return _geo[name]


def blend_want(oracle, name, kind, f32=False):
    corners, sizes, bands, tiles, memo = geometry(name)
    if (kind, f32) not in memo:
        ob = oracle.Feather(0.1) if kind == "feather" else (oracle.NoBlend() if kind == "no" else oracle.MultiBand(bands, KINDS[kind]))
        ob.prepare(corners, sizes)
        for (img, m), c in zip(tiles, corners):
            ob.feed(img.astype(np.int16), m, c)
        memo[(kind, f32)] = ob.blend(f32) if kind in ("i16", "f32", "f16") else ob.blend()
    return memo[(kind, f32)]


def make_blender(gpu, name, kind, mode):
    bands = GEOMETRIES[name][2]
    b = gpu.FeatherBlender(False, 0.1) if kind == "feather" else (gpu.NoBlender() if kind == "no" else gpu.MultiBandBlender(False, bands, KINDS[kind]))
    if mode:
        b.set_deferred_level0(mode)
    return b


def feed_all(b, name, s16=False, special=None):
    """prepare() and the feeds of a geometry from ordinary guarded device mats; special = (operand, spec): tile 0's image or mask lies in
    that large-pitch layout.  Returns the guarded inputs."""
    corners, sizes, _, tiles, _ = geometry(name)
    b.prepare(corners, sizes)
    ins = []
    for k, ((img, m), c) in enumerate(zip(tiles, corners)):
        a = img.astype(np.int16) if s16 else img
        gi = big(a.shape, a.dtype, special[1] if special and k == 0 and special[0] == "img" else None, "img%d" % k, a)
        gm = big(m.shape, np.uint8, special[1] if special and k == 0 and special[0] == "mask" else None, "mask%d" % k, m)
        (b.feed if s16 else b.feed_u8)(gi.view, gm.view, c)
        ins += [gi, gm]
    return ins


# operand, (layout, pitch), geometry, on the fast side
PLACEMENTS = [("img", ("wide", None), "r16", False), ("mask", ("wide", P24 + 64), "r16", False), ("img", ("tall31", None), "r256", False),
              ("mask", ("tall31", None), "r256", False), ("img", ("wide_below", None), "r16", True), ("mask", ("wide_below", None), "r16", True),
              ("img", ("tall31", None), "r255", True), ("mask", ("tall31", None), "r255", True)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ["i16", "f32", "f16"])
def test_feed_of_a_tile_past_and_below_the_source_limits(gpu, oracle, kind, mode):
    """isx_blender_feed (CV_16SC3) / _feed_u8 (CV_8UC3) of device tiles, eager, deferred (mode 1) and with private copies (mode 2): the
    tile's image, then its mask, at a pitch of 2^24 and at step * rows = 2^31 - there Src0::iend stays 0 and every kernel reads the tile
    through load_src0's size_t branch: mode 2 feeds that tile without the fused pass, mode 1 ends in k_collapse_gather - and 64 bytes /
    one row below: the fused feed, k_collapse_roll.  The oracle's bytes everywhere."""
    for i, (operand, spec, name, fast) in enumerate(PLACEMENTS):
        s16 = (i + mode + KINDS[kind]) % 2 == 1
        od, om = blend_want(oracle, name, kind)
        b = make_blender(gpu, name, kind, mode)
        ins = feed_all(b, name, s16, (operand, spec))
        d, dm = big(od.shape, np.int16, None, "dst"), big(om.shape, np.uint8, None, "dst_mask")
        b.blend(d.view, dm.view)
        sync()
        path, fed = b.last_path(), b.feed_path()
        what = (kind, mode, operand, spec, s16, path, fed)
        assert path["cycle"] == ("deferred" if mode else "eager"), what
        if mode == 1:
            assert path["last_step"] == ("collapse_roll" if fast else "collapse_gather"), what
            if kind == "f32" and not s16:
                assert b.level1_format() == ("planar_q8" if fast else "records"), what
        if mode == 2:
            assert fed["fused_tiles"] == (2 if fast else 1), what          # tile 1 is an ordinary mat: fused either way
            assert path["last_step"] == "collapse_roll", what             # (slow side: tile 0's private copy is dense, iend is set for it)
        else:
            assert fed["fused_tiles"] == 0, what
        equal(d, od, what), equal(dm, om, what)
        d.check(), dm.check()
        unchanged(*ins)
        del ins


@pytest.mark.parametrize("kind,mode", [("feather", 0), ("feather", 1), ("feather", 2), ("no", 0)])
def test_feather_and_no_feed_of_a_tile_past_the_source_limits(gpu, oracle, kind, mode):
    """FeatherBlender (eager: k_feather_acc reads the tile in feed(); deferred: k_feather_gather reads the caller's tile in blend(); mode 2:
    its private copy) and Blender::NO (k_no_feed): the tile's image, then its mask, at a pitch of 2^24 / 2^24 + 64 and at step * rows =
    2^31.  These kernels have one form, with size_t rows: the oracle's bytes, the inputs untouched."""
    first = {("feather", 0): "feather_acc", ("feather", 1): "feather_gather", ("feather", 2): "feather_gather", ("no", 0): "no_feed"}[(kind, mode)]
    for i, (operand, spec, name, fast) in enumerate(PLACEMENTS):
        if fast:
            continue
        od, om = blend_want(oracle, name, kind)
        b = make_blender(gpu, name, kind, mode)
        with launches() as l:
            ins = feed_all(b, name, i % 2 == 1, (operand, spec))
            d, dm = big(od.shape, np.int16, None, "dst"), big(om.shape, np.uint8, None, "dst_mask")
            b.blend(d.view, dm.view)
        assert first in l.names and (mode == 0 or "feather_acc" not in l.names), (kind, mode, l.names)
        equal(d, od, (kind, mode, operand, spec)), equal(dm, om, (kind, mode, operand, spec))
        d.check(), dm.check()
        unchanged(*ins)
        del ins


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_blend_batch_with_a_tile_past_the_limit(gpu, oracle, kind):
    """isx_blender_blend_batch of two deferred blenders: one tile of the first at a pitch of 2^24 turns the whole chain's last step into
    k_collapse_gather; 64 bytes below, the batch ends in k_collapse_roll."""
    from imagestitch_amd.blender import blend_batch
    od, om = blend_want(oracle, "r16", kind)
    for spec, last in ((("wide", None), "collapse_gather"), (("wide_below", None), "collapse_roll")):
        bs, ins, outs = [], [], []
        for k in range(2):
            b = make_blender(gpu, "r16", kind, 1)
            ins += feed_all(b, "r16", False, ("img", spec) if k == 0 else None)
            bs.append(b)
            outs.append((big(od.shape, np.int16, None, "dst"), big(om.shape, np.uint8, None, "dst_mask")))
        blend_batch(bs, [d.view for d, _ in outs], [m.view for _, m in outs])
        sync()
        for b, (d, dm) in zip(bs, outs):
            assert b.last_path() == {"cycle": "deferred_batched", "last_step": last}, (spec, b.last_path())
            equal(d, od, spec), equal(dm, om, spec)
            d.check(), dm.check()
        unchanged(*ins)
        del ins


def test_a_widened_cycle_keeps_32_bit_offsets_for_its_wide_copies(gpu, oracle):
    """Mode 2, CV_16SC3 tiles of which one holds a value that is no byte: the narrowed copies are widened (isx_blender_feed_path: 2) and
    narrow_resolve() computes Src0::iend for the wide copies again - they are dense, so the last step stays k_collapse_roll."""
    corners, sizes, bands, tiles, _ = geometry("r16")
    imgs = [t[0].astype(np.int16) for t in tiles]
    imgs[0][5, 7] = (300, -4, 255)
    ob = oracle.MultiBand(bands, F32)
    ob.prepare(corners, sizes)
    for im, (_, m), c in zip(imgs, tiles, corners):
        ob.feed(im, m, c)
    od, om = ob.blend(False)
    b = gpu.MultiBandBlender(False, bands, F32)
    b.set_deferred_level0(2)
    b.prepare(corners, sizes)
    ins = []
    for k, (im, (_, m), c) in enumerate(zip(imgs, tiles, corners)):
        gi, gm = big(im.shape, np.int16, ("wide_below", None) if k == 0 else None, "img%d" % k, im), big(m.shape, np.uint8, None, "mask%d" % k, m)
        b.feed(gi.view, gm.view, c)
        ins += [gi, gm]
    d, dm = big(od.shape, np.int16, None, "dst"), big(om.shape, np.uint8, None, "dst_mask")
    b.blend(d.view, dm.view)
    sync()
    assert b.feed_path() == {"fused_tiles": 2, "narrowed": "widened"} and b.last_path()["last_step"] == "collapse_roll", (b.feed_path(), b.last_path())
    equal(d, od), equal(dm, om)
    d.check(), dm.check()
    unchanged(*ins)


def _outputs(od, om, dt, operand, spec):
    return big(od.shape, dt, spec if operand == "dst" else None, "dst"), big(om.shape, np.uint8, spec if operand == "dst_mask" else None, "dst_mask")


# geometry -> the (operand, (layout, pitch)) that one fed blender refuses in turn
REFUSALS = {"r16": [("dst", ("wide", None)), ("dst", ("wide", P24 + 64)), ("dst_mask", ("wide", None))],
            "r257": [("dst", ("tall32", BELOW)), ("dst_mask", ("tall32", BELOW))],
            "r258": [("dst_mask", ("tall32", BELOW))],                # the first row count whose last row starts past 2^32
            "r512": [("dst_mask", ("tall32", None))]}


@pytest.mark.parametrize("kind", list(KINDS))
def test_blend_refuses_a_destination_past_its_limits(gpu, oracle, kind):
    """isx_blender_blend, multi-band in the three precisions (deferred: k_collapse_roll stores the result), Feather and NO: dst and
    dst_mask at a pitch of 2^24, dst and - beside a dense dst - dst_mask at step * rows >= 2^32 (257 and 258 rows of 2^24 - 64 bytes;
    512 rows of 2^23: exactly 2^32) are ISX_ERR_UNSUPPORTED with nothing written, and the blender is as it was: blend() into ordinary
    mats gives the oracle's result.  The mask's span was not checked (o.mask[__umul24(y, o.mask_step) + x] and the last step's
    (unsigned)y * (unsigned)mask_step wrap from row 257 of such a mask on).  256 rows of 2^24 - 64 bytes, 16 KiB below the limit, and
    511 rows of 2^23 are blended."""
    mode = 1 if kind in ("i16", "f32", "f16") else 0
    dt = np.float32 if kind == "f32" else np.int16
    for name, specs in REFUSALS.items():
        od, om = blend_want(oracle, name, kind, dt == np.float32)
        b = make_blender(gpu, name, kind, mode)
        ins = feed_all(b, name)
        for operand, spec in specs:
            d, dm = _outputs(od, om, dt, operand, spec)
            refused(lambda: b.blend(d.view, dm.view))
            sync()
            unchanged(d, dm, *ins)
            del d, dm
        d, dm = _outputs(od, om, dt, None, None)
        b.blend(d.view, dm.view)
        sync()
        equal(d, od, (kind, name)), equal(dm, om, (kind, name))
        d.check(), dm.check()
        unchanged(*ins)
    for name, operand, spec in (("r256", "dst", ("tall32", BELOW)), ("r256", "dst_mask", ("tall32", BELOW)), ("r511", "dst_mask", ("tall32", None))):
        od, om = blend_want(oracle, name, kind, dt == np.float32)
        b = make_blender(gpu, name, kind, mode)
        ins = feed_all(b, name)
        d, dm = _outputs(od, om, dt, operand, spec)
        b.blend(d.view, dm.view)
        sync()
        if mode:
            assert b.last_path() == {"cycle": "deferred", "last_step": "collapse_roll"}, b.last_path()
        equal(d, od, (kind, name, operand)), equal(dm, om, (kind, name, operand))
        d.check(), dm.check()
        unchanged(*ins)
        del d, dm


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_blend_window_at_the_destination_limits(gpu, oracle, kind):
    """... and with a column window (isx_blender_set_window): the mats hold the columns [128, 256) of a result 190 wide."""
    dt = np.float32 if kind == "f32" else np.int16
    x0, x1 = 128, 256
    for name, operand, spec, ok in (("w257", "dst", ("tall32", BELOW), False), ("w257", "dst_mask", ("tall32", BELOW), False),
                                    ("w256", "dst", ("tall32", BELOW), True), ("w256", "dst_mask", ("tall32", BELOW), True)):
        od, om = blend_want(oracle, name, kind, dt == np.float32)
        fh, fw = om.shape
        assert fw == 190 and fh == GEOMETRIES[name][1][0][1]
        b = make_blender(gpu, name, kind, 1)
        b.set_window(x0, x1)
        ins = feed_all(b, name)
        outs = [_outputs(np.empty((fh, x1 - x0, 3)), np.empty((fh, x1 - x0)), dt, operand, spec)] if not ok else []
        for d, dm in outs:
            refused(lambda: b.blend(d.view, dm.view))
            sync()
            unchanged(d, dm, *ins)
        del outs
        d, dm = _outputs(np.empty((fh, x1 - x0, 3)), np.empty((fh, x1 - x0)), dt, operand if ok else None, spec)
        b.blend(d.view, dm.view)
        sync()
        n = fw - x0
        assert np.array_equal(d.get()[:, :n], od[:, x0:]) and np.array_equal(dm.get()[:, :n], om[:, x0:]), (kind, name, operand)
        d.check(written=(0, n)), dm.check(written=(0, n))
        unchanged(*ins)
        del d, dm


@pytest.mark.parametrize("kind", list(KINDS))
def test_prepare_refuses_a_roi_past_the_record_index(gpu, kind):
    """isx_blender_prepare_roi: 2^24 pixels a side and 2^31 pixels are ISX_ERR_UNSUPPORTED before anything is allocated."""
    import torch
    b = make_blender(gpu, "r16", kind, 0)
    gc.collect()                                                     # a blender of an earlier case (1.2 GiB prepared) that only a dead cycle holds goes now, not between the two readings
    sync()
    kept, free = b.retained_bytes(), torch.cuda.mem_get_info()[0]
    rois = [(0, 0, 65536, 32768)] + ([(0, 0, 1 << 24, 1)] if kind not in ("no",) else [])      # (Blender::NO keeps one level: only the pixel count)
    for roi in rois:
        refused(lambda: b.prepare(roi))
    sync()
    assert b.retained_bytes() == kept and abs(torch.cuda.mem_get_info()[0] - free) < (64 << 20)
    if kind != "no":
        b.prepare((0, 0, (1 << 24) - 32, 1))                          # one block of 32 below: prepared (16 bytes a record: 1.2 GiB at most)


# ---- every other entry, once on "wide" ---------------------------------------------------------------------------------------------
def wide(shape, dtype, name, content=None, plus64=False):
    """A device mat of 8-16 rows at a pitch of 2^24 (or 2^24 + 64) bytes."""
    assert 8 <= shape[0] <= 16, shape
    return big(shape, dtype, ("wide", P24 + 64 if plus64 else None), name, content)


def layout16(n, seed_):
    """n overlapping tiles of 12-16 rows (the tiles of test_gpu_guard_bands.small_layout, lower): corners, CV_8UC3 images, masks with a hole."""
    rng = np.random.default_rng(seed_)
    sizes, corners = [(67, 16), (65, 14), (63, 12)][:n], [(0, 0), (31, -3), (-20, 4)][:n]
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


def _finder(call, images, masks, want):
    gi = [wide(a.shape, a.dtype, "image%d" % k, a) for k, a in enumerate(images)] if images is not None else []
    gm = [wide(m.shape, np.uint8, "mask%d" % k, m, plus64=k == 1) for k, m in enumerate(masks)]
    call([g.view for g in gi], [g.view for g in gm])
    sync()
    for k, (g, w) in enumerate(zip(gm, want)):
        equal(g, w, k)
        g.check()
    unchanged(*gi)


def _dilate_and(gpu, oracle):
    rng = np.random.default_rng(9)
    for (w, h), (kw, kh), with_other in (((67, 12), (3, 3), True), ((65, 9), (20, 20), False)):
        mask = (rng.random((h, w)) > 0.8).astype(np.uint8) * 255
        other = (rng.random((h, w)) > 0.2).astype(np.uint8) * 255
        gm, go = wide(mask.shape, np.uint8, "mask", mask), wide(other.shape, np.uint8, "other", other, True) if with_other else None
        d = wide((h, w), np.uint8, "out")
        _lib.check(_lib.load().isx_mask_dilate_and(ref(gm), ref(go), kw, kh, ref(d), 0, None))
        sync()
        equal(d, (oracle.dilate_rect(mask, kw, kh) & (other if with_other else 255)).astype(np.uint8), (w, h))
        d.check()
        unchanged(gm, go)


def _gain_apply(gpu, oracle):
    rng = np.random.default_rng(10)
    for cn, gain in ((3, 1.37), (1, 0.61)):
        img = GB.img_u8(rng, 12, 67, cn)
        g = wide(img.shape, np.uint8, "image", img, cn == 1)
        gpu.gain_apply(g.view, gain)
        sync()
        equal(g, oracle.gain_apply(img, gain), cn)
        g.check()


def _convert_to(gpu, oracle):
    rng = np.random.default_rng(11)
    for sd, dd, cn in ((np.uint8, np.int16, 3), (np.int16, np.float32, 3), (np.float32, np.uint8, 3), (np.float32, np.int16, 3), (np.uint8, np.float32, 1)):
        shape = (9, 65, cn) if cn > 1 else (9, 65)
        if sd == np.float32:
            src = ((rng.random(shape) - 0.5) * (70000 if dd == np.int16 else 600)).astype(np.float32)
            want = oracle.convert_f32(src, dd)
        elif sd == np.int16:
            src = rng.integers(-32768, 32768, shape).astype(np.int16)
            want = src.astype(np.float32)
        else:
            src = rng.integers(0, 256, shape, dtype=np.uint8)
            want = src.astype(dd)
        s, d = wide(shape, sd, "src", src), wide(shape, dd, "dst", None, True)
        gpu.convert_to(s.view, dd, dst=d.view)
        sync()
        equal(d, want, (sd, dd, cn))
        d.check()
        unchanged(s)


def _seam_gradients(gpu, oracle):
    rng = np.random.default_rng(12)
    for u8 in (True, False):
        img = GB.img_u8(rng, 16, 70) if u8 else (rng.random((16, 70, 3)) * 255).astype(np.float32)
        gx_all, gy_all = GB.M.gradients(img)
        s = wide(img.shape, img.dtype, "image", img)
        x, y, w, h = 7, 2, 40, 9
        ox, oy = wide((h, w), np.float32, "abs_gradx"), wide((h, w), np.float32, "abs_grady", None, True)
        gpu.seam_gradients(s.view, (x, y, w, h), out=(ox.view, oy.view))
        sync()
        equal(ox, np.ascontiguousarray(np.abs(gx_all)[y:y + h, x:x + w])), equal(oy, np.ascontiguousarray(np.abs(gy_all)[y:y + h, x:x + w]))
        ox.check(), oy.check()
        unchanged(s)


def _seam_estimate(gpu, oracle):
    for seed_, u8, horizontal in ((0, False, False), (1, True, True)):
        c = GB.make_case(seed_, size1=(14, 67), size2=(16, 65), tl1=(-9, 1), tl2=(25, -1), u8=u8, horizontal=horizontal)
        args = (c["img1"], c["img2"], c["tl1"], c["tl2"], c["union_tl"], c["labels"], c["label"], c["roi"], c["p1"], c["p2"])
        assert c["labels"].shape[0] <= 24
        g1, g2 = wide(c["img1"].shape, c["img1"].dtype, "image1", c["img1"]), wide(c["img2"].shape, c["img2"].dtype, "image2", c["img2"], True)
        gl = big(c["labels"].shape, c["labels"].dtype, ("wide", None), "labels", c["labels"])
        for cf, model_cf in ((gpu.DP_COLOR, GB.M.COLOR), (gpu.DP_COLOR_GRAD, GB.M.COLOR_GRAD)):
            mw, mh = GB.M.seam_estimate(*args, model_cf)
            got, gh = gpu.seam_estimate(g1.view, g2.view, *args[2:5], gl.view, *args[6:], cost_func=cf)
            sync()
            assert gh == mh and np.array_equal(got, mw) and len(mw) > 0, cf
            unchanged(g1, g2, gl)


def _dp_seam_find(gpu, oracle):
    for n, u8 in ((2, True), (3, False)):
        images, corners, masks = GB.make_find_case(53, n, u8, holes=True, size=(11, 67))          # tiles of 15, 16 and 11 rows
        for cost, cf in ((GB.M.COLOR, gpu.DP_COLOR), (GB.M.COLOR_GRAD, gpu.DP_COLOR_GRAD)):
            want = [m.copy() for m in masks]
            GB.M.DpSeamFinder(cost).find(images, corners, want)
            assert any((a != b).any() for a, b in zip(want, masks))
            _finder(lambda gi, gm: gpu.DpSeamFinder(cf).find(gi, corners, gm), images, masks, want)


def _graphcut_seam_find(gpu, oracle):
    import scipy  # noqa: F401  (helpers/graphcut_np.py needs it)
    for n, f32 in ((2, False), (3, True)):
        corners, imgs, masks = layout16(n, n)
        want = [m.copy() for m in masks]
        GB.GC.find(imgs, corners, want)
        assert any((a != b).any() for a, b in zip(want, masks))
        _finder(lambda gi, gm: gpu.GraphCutSeamFinder().find(gi, corners, gm), [a.astype(np.float32) for a in imgs] if f32 else imgs, masks, want)
    for n in (2, 3):                                                 # COST_COLOR_GRAD: the Sobel's three row pointers per tile, every mat at the wide pitch
        corners, imgs, masks = layout16(n, n)
        want = GB.GCG.find(imgs, corners, [m.copy() for m in masks])
        assert any((a != b).any() for a, b in zip(want, masks))
        _finder(lambda gi, gm: gpu.GraphCutSeamFinder(cost_type=GB.GCG.COST_COLOR_GRAD).find(gi, corners, gm), [a.astype(np.float32) for a in imgs], masks, want)


def _voronoi_seam_find(gpu, oracle):
    corners, _, masks = layout16(3, 2)
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    want = [m.copy() for m in masks]
    GB.V.find(sizes, corners, want)
    assert any((a != b).any() for a, b in zip(want, masks))
    _finder(lambda gi, gm: gpu.VoronoiSeamFinder().find(sizes, corners, gm), None, masks, want)


def _gain_compensator_feed(gpu, oracle):
    corners, imgs, masks = layout16(3, 3)
    for m in masks:
        m[::3, ::5] = 254
    N, I, _, _, _, g = GB.feed_model(corners, imgs, masks)
    gi = [wide(a.shape, np.uint8, "image%d" % k, a) for k, a in enumerate(imgs)]
    gm = [wide(m.shape, np.uint8, "mask%d" % k, m, k == 1) for k, m in enumerate(masks)]
    comp = gpu.GainCompensator().feed(corners, [x.view for x in gi], [x.view for x in gm])
    sync()
    assert np.array_equal(comp.N, N) and np.array_equal(comp.I.view(np.uint64), I.view(np.uint64))
    np.testing.assert_allclose(comp.gains(), g, rtol=1e-12, atol=0)
    unchanged(*gi, *gm)


def _blocks_gain(gpu, oracle):
    """isx_blocks_gain_feed, _apply and _map: blocks of 32 x 2, so that the maps have 8 and 7 rows."""
    from blocks_gain_cases import forward_error_rtol
    corners, imgs, masks = layout16(2, 1)
    for m in masks:
        m[::3, ::5] = 254
    model = GB.BG.feed_blocks_model(corners, imgs, masks, 32, 2)
    assert model["counts"] == [(3, 8), (3, 7)], model["counts"]
    rtol = forward_error_rtol(model["A"], model["b"], model["gains"])[0]
    gi = [wide(a.shape, np.uint8, "image%d" % k, a) for k, a in enumerate(imgs)]
    gm = [wide(m.shape, np.uint8, "mask%d" % k, m, k == 1) for k, m in enumerate(masks)]
    comp = gpu.BlocksGainCompensator(32, 2).feed(corners, [x.view for x in gi], [x.view for x in gm])
    sync()
    pairs, diag = comp.block_stats()
    assert comp.block_counts() == model["counts"] and np.array_equal(diag, model["diag_n"])
    assert [(int(p["block_i"]), int(p["block_j"]), int(p["n"])) for p in pairs] == [p[:3] for p in model["pairs"]]
    np.testing.assert_allclose(comp.gains(), model["gains"], rtol=rtol, atol=0)
    unchanged(*gi, *gm)
    gmaps = comp.gain_maps()
    img = GB.img_u8(np.random.default_rng(15), 12, 67)
    g = wide(img.shape, np.uint8, "image", img)
    comp.apply(0, (0, 0), g.view)
    sync()
    equal(g, GB.BG.apply_model(img, gmaps[0]))
    g.check()
    want = GB.BG.maps_from_gains(comp.gains(), comp.block_counts())[0]
    d = wide(want.shape, np.float32, "map")
    _lib.check(_lib.load().isx_blocks_gain_map(comp._h, 0, ref(d), None))
    sync()
    equal(d, want)
    d.check()


def _blend_pair_linear(gpu, oracle):
    rng = np.random.default_rng(13)
    img1, img2 = (rng.random((16, 67, 3)) * 255).astype(np.float32), (rng.random((16, 65, 3)) * 255).astype(np.float32)
    img1[:3, -9:] = 3.0
    img2[-2:, :7] = 2.0
    tl1, tl2 = (10, 20), (50, 20)
    rc, opano, oseam = oracle.blend_pair_linear(img1, img2, tl1, tl2)
    assert rc == 0 and opano.shape[0] == 16
    g1, g2 = wide(img1.shape, np.float32, "images1", img1), wide(img2.shape, np.float32, "images2", img2, True)
    d = wide(opano.shape, np.float32, "pano")
    seam_x = np.zeros(opano.shape[0], np.int32)
    _lib.check(_lib.load().isx_blend_pair_linear(ref(g1), ref(g2), tl1[0], tl1[1], tl2[0], tl2[1], ref(d), seam_x.ctypes.data_as(_lib._IP), 0, None))
    sync()
    assert np.array_equal(seam_x, oseam)
    equal(d, opano)
    d.check()
    unchanged(g1, g2)


WIDE_ENTRIES = {"dilate_and": _dilate_and, "gain_apply": _gain_apply, "convert_to": _convert_to, "seam_gradients": _seam_gradients,
                "seam_estimate": _seam_estimate, "dp_seam_find": _dp_seam_find, "graphcut_seam_find": _graphcut_seam_find,
                "voronoi_seam_find": _voronoi_seam_find, "gain_compensator_feed": _gain_compensator_feed, "blocks_gain_feed_apply_map": _blocks_gain,
                "blend_pair_linear": _blend_pair_linear}


@pytest.mark.parametrize("entry", list(WIDE_ENTRIES))
def test_every_other_entry_on_a_pitch_of_2p24(gpu, oracle, entry):
    """The entries whose kernels index with size_t, pinned: every device mat of the call has 8-16 rows (asserted where it is built) at a
    pitch of 2^24 or 2^24 + 64 bytes; the expectations are those of tests/test_gpu_guard_bands.py (oracle and NumPy models), the guard
    checks too - inputs untouched, outputs written inside their view only."""
    WIDE_ENTRIES[entry](gpu, oracle)


def test_resize_entries_on_a_pitch_of_2p24(gpu):
    """isx_resize and isx_mask_dilate_resize_and (the model of tests/test_gpu_resize_guard.py) with every mat at 2^24 or 2^24 + 64 bytes a
    row."""
    from helpers import resize_np as RZ
    lib = _lib.load()
    rng = np.random.default_rng(21)
    src = GB.img_u8(rng, 16, 67)
    for (dw, dh), interp in (((40, 9), RZ.LINEAR), ((70, 12), RZ.NEAREST)):
        s, d = big(src.shape, np.uint8, ("wide", None), "src", src), big((dh, dw, 3), np.uint8, ("wide", P24 + 64), "dst")
        _lib.check(lib.isx_resize(ref(s), ref(d), interp, 0, None))
        sync()
        equal(d, RZ.resize(src, (dw, dh), interp), (dw, dh, interp))
        d.check()
        unchanged(s)
    seam = np.where(rng.random((9, 31)) < 0.25, 255, 0).astype(np.uint8)
    warped = np.where(rng.random((16, 67)) < 0.8, 255, 0).astype(np.uint8)
    gs, gw = big(seam.shape, np.uint8, ("wide", None), "seam_mask", seam), big(warped.shape, np.uint8, ("wide", P24 + 64), "warped_mask", warped)
    go = big(warped.shape, np.uint8, ("wide", None), "out")
    _lib.check(lib.isx_mask_dilate_resize_and(ref(gs), ref(gw), 3, 3, ref(go), 0, None))
    sync()
    equal(go, RZ.dilate_resize_and(seam, warped, 3, 3, (67, 16)))
    go.check()
    unchanged(gs, gw)


# ---- one host mat ------------------------------------------------------------------------------------------------------------------------
def host_wide(array, seed_):
    """A host mat of 2^24 + 64 bytes a row inside one seeded NumPy buffer (the staging's hipMemcpy2DAsync takes that pitch): the view,
    the buffer and its snapshot."""
    a = np.asarray(array)
    pitch, lead = P24 + 64, 4096
    row = a.shape[1] * (a.shape[2] if a.ndim == 3 else 1) * a.itemsize
    buf = np.random.default_rng(seed_).integers(0, 256, lead + (a.shape[0] - 1) * pitch + row + lead, dtype=np.uint8)
    view = np.ndarray(a.shape, a.dtype, buffer=buf, offset=lead, strides=(pitch,) + a.strides[1:])
    view[...] = a
    return view, buf, buf.copy()


def test_a_host_mat_of_2p24_64_bytes_a_row(gpu, oracle):
    """isx_warper_warp and isx_blender_feed_u8 of a HOST mat whose rows are 2^24 + 64 bytes apart (8 rows): staged with that pitch,
    the oracle's bytes, the caller's buffer untouched."""
    w, h, f = 67, 8, 90.0
    K, R = GB.rig(w, h, f)
    roi, xm, ym = GB.maps(oracle, CYL, f, K, R, w, h)
    src = GB.img_u8(np.random.default_rng(3), h, w)
    want = oracle.remap(src, xm, ym, LINEAR, REFLECT)
    view, buf, snap = host_wide(src, seed())
    assert view.shape[0] == 8 and _lib.as_mat(view).step == P24 + 64
    d = G.guarded(want.shape, np.uint8, "host", "odd", seed(), "dst")
    corner, _ = GB.make_warper(gpu, CYL, f).warp(view, K, R, LINEAR, REFLECT, dst=d.view)
    sync()
    assert corner == roi[:2]
    equal(d, want)
    d.check()
    assert np.array_equal(buf, snap)
    del buf, snap
    corners, sizes, bands, tiles, _ = geometry("r8")
    od, om = blend_want(oracle, "r8", "i16")
    for mode in (0, 2):
        b = make_blender(gpu, "r8", "i16", mode)
        b.prepare(corners, sizes)
        view, buf, snap = host_wide(tiles[0][0], seed())
        assert view.shape[0] == 8 and _lib.as_mat(view).step == P24 + 64
        b.feed_u8(view, tiles[0][1], corners[0])
        b.feed_u8(tiles[1][0], tiles[1][1], corners[1])
        dd, dm = b.blend(np.empty(od.shape, np.int16), np.empty(om.shape, np.uint8))
        sync()
        assert np.array_equal(dd, od) and np.array_equal(dm, om) and np.array_equal(buf, snap), mode
        del buf, snap


# ---- the helper itself -------------------------------------------------------------------------------------------------------------------
def test_a_stray_store_in_a_large_pitch_mat_is_found(gpu):
    """tests/helpers/guarded_wide.py on the device: a store before the view, in a gap, after the view and - the mask store this file is
    about - one that wrapped at 2^32 onto an early row; `written` limits the view as in guarded.py."""
    g = W.wide_guarded((12, 40, 3), np.uint8, "wide", seed())
    g.check(), g.check(G.NOTHING)
    for i, region in ((g.offset - 1, "above"), (g.offset + g.row_bytes, "pad"), (g.offset + g.pitch - 1, "lead"), (g.offset + 11 * g.pitch + g.row_bytes, "below"),
                      (0, "above"), (g.nbytes - 1, "below"), (g.offset + 3 * g.pitch + 5, "view")):
        g.buf[i] ^= 0x5A
        with pytest.raises(G.GuardError) as e:
            g.check(G.NOTHING)
        assert e.value.region == region, (i, e.value.region)
        g.buf[i] ^= 0x5A
        g.check(G.NOTHING)
    g.view[:, 3:5] += 1
    g.check(), g.check((3, 5))
    for written in (G.NOTHING, (3, 4), (4, 5)):
        with pytest.raises(G.GuardError) as e:
            g.check(written)
        assert e.value.region == "view"
    del g
    t = big((258, 28), np.uint8, ("tall32", BELOW), "mask")
    t.check(G.NOTHING)
    assert 256 * t.pitch + t.row_bytes < 1 << 32 <= 257 * t.pitch      # 257 rows still end below 2^32; row 257 starts past it
    wrapped = (257 * t.pitch + 5) % (1 << 32)                        # where a 32-bit offset puts byte 5 of row 257
    assert wrapped // t.pitch == 0 and wrapped % t.pitch >= t.row_bytes
    t.buf[t.offset + wrapped] ^= 0x5A
    with pytest.raises(G.GuardError) as e:
        t.check()
    assert e.value.region == "pad" and e.value.row == 0
