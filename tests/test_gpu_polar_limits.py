"""The fisheye and stereographic entries at the addressing limits tests/test_gpu_addressing_limits.py holds the other kinds to (the
polar section, "Limits").  k_polar_warp and k_polar_build_maps index with size_t and keep cv::remap's short source coordinates: warp_roi and
build_maps_roi are served at a row pitch of 2^24 bytes, on a source of 32768 pixels a side (coordinates clamp at 32767) and on a source
past 2 GiB.  The fused entry applies warp_with_mask's refusals before it looks at the kind: ISX_ERR_UNSUPPORTED from a pitch of 2^24 and
from 32768 pixels a side, with nothing written.  A window 65536 wide or high (br - tl, as cv::Rect measures it) is ISX_ERR_INVALID for every entry, 65535 are served.
One operand of a call lies in a large-pitch guarded mat (tests/helpers/guarded_wide.py), every other mat in an ordinary guarded one; every
served case equals oracle.remap over the MODEL's maps (tests/helpers/polar_np.py) byte for byte, outputs have only their view written and
inputs not one byte, and the launch names say which kernel ran."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
import test_gpu_addressing_limits as AL  # noqa: E402  (big(), launches, refused, mat / ref; its seeds are test_gpu_guard_bands')
import test_gpu_guard_bands as GB  # noqa: E402
from helpers import polar_np as P  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]
P24 = 1 << 24
INVALID, UNSUPPORTED = 1, 6
big, launches, refused, ref, sync, equal, unchanged = AL.big, AL.launches, AL.refused, AL.ref, AL.sync, AL.equal, AL.unchanged
POLAR_LAUNCHES = {"polar_warp", "polar_build_maps", "polar_warp_img_mask"}


@pytest.fixture(autouse=True)
def own_seeds(request):
    GB._seed[0] = zlib.crc32(request.node.name.encode()) << 16


@pytest.fixture(scope="module", autouse=True)
def release_the_large_buffers():
    yield
    import torch
    torch.cuda.empty_cache()


def _warper(gpu, kind, scale):
    return (gpu.FisheyeWarper if kind == P.FISHEYE else gpu.StereographicWarper)().create(scale)


def _shape(win):
    return (win[3] - win[1] + 1, win[2] - win[0] + 1)


def _warp_roi(warper, s, K, R, interp, border, win, d):
    _lib.check(warper._lib.isx_warper_warp_roi(warper._h, ref(s), _lib.f9(K)[1], _lib.f9(R)[1], interp, border, (C.c_int * 4)(*[int(v) for v in win]), ref(d)))


def _fused_roi(warper, s, K, R, win, di, dm):
    _lib.check(warper._lib.isx_warper_warp_with_mask_roi(warper._h, ref(s), None, _lib.f9(K)[1], _lib.f9(R)[1], (C.c_int * 4)(*[int(v) for v in win]), ref(di), ref(dm)))


def window_over(m, xs, ys, most=(64, 24)):
    """The destination rectangle that holds mapForward of the source points xs x ys (neither projection is close to the identity), cut to
    `most` (w, h) around its centre."""
    gx, gy = np.meshgrid(np.asarray(xs, F), np.asarray(ys, F))
    u, v = m.map_forward(gx, gy)
    assert np.isfinite(u).all() and np.isfinite(v).all()
    x0, y0, x1, y1 = int(np.floor(u.min())), int(np.floor(v.min())), int(np.ceil(u.max())), int(np.ceil(v.max()))
    if x1 - x0 + 1 > most[0]:
        x0 = (x0 + x1) // 2 - most[0] // 2
        x1 = x0 + most[0] - 1
    if y1 - y0 + 1 > most[1]:
        y0 = (y0 + y1) // 2 - most[1] // 2
        y1 = y0 + most[1] - 1
    return (x0, y0, x1, y1)


def _maps_roi(warper, K, R, win, gx, gy):
    _lib.check(warper._lib.isx_warper_build_maps_roi(warper._h, _lib.f9(K)[1], _lib.f9(R)[1], (C.c_int * 4)(*[int(v) for v in win]), ref(gx), ref(gy)))


# ---- a row pitch of 2^24 bytes ------------------------------------------------------------------------------------------------------------------
_small = {}


def small(oracle, kind):
    """A 41 x 13 source (13 rows: a wide layout takes 8-24) and a 47 x 10 window of its ROI, with the model's maps and the expected tiles (once)."""
    if kind not in _small:
        w, h, f = 41, 13, 25.0
        K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F)
        R = P.ROTATIONS["yaw0.52"].astype(F)
        m = P.from_rig(kind, f, K, R)
        roi = [int(v) for v in m.detect_roi(w, h)[0]]
        assert roi[2] - roi[0] >= 20 and roi[3] - roi[1] >= 10, roi
        win = (roi[0], roi[1] + 1, min(roi[2], roi[0] + 46), roi[1] + 10)
        xm, ym = m.build_maps(win)
        img = PC.image(np.random.default_rng(60 + kind), h, w)
        _small[kind] = dict(f=f, K=K, R=R, win=win, xm=xm, ym=ym, img=img, wi=oracle.remap(img, xm, ym, PC.LINEAR, PC.REFLECT),
                            wm=oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST))
        assert (_small[kind]["wm"] == 255).any() and _shape(win)[0] == 10
    return _small[kind]


WIDE = {"pitch_2p24": ("wide", None), "pitch_2p24_64": ("wide", P24 + 64)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("operand", ["src", "dst"])
@pytest.mark.parametrize("pitch", list(WIDE))
def test_warp_roi_is_served_at_a_pitch_of_2p24(gpu, oracle, pitch, operand, kind):
    c = small(oracle, kind)
    s = big(c["img"].shape, np.uint8, WIDE[pitch] if operand == "src" else None, "src", c["img"])
    d = big(c["wi"].shape, np.uint8, WIDE[pitch] if operand == "dst" else None, "dst")
    with launches() as l:
        _warp_roi(_warper(gpu, kind, c["f"]), s, c["K"], c["R"], PC.LINEAR, PC.REFLECT, c["win"], d)
    assert l.names & (POLAR_LAUNCHES | {"warp", "warp_tile_img"}) == {"polar_warp"}, l.names
    equal(d, c["wi"], (pitch, operand))
    d.check()
    unchanged(s)


@pytest.mark.parametrize("kind", KINDS)
def test_build_maps_roi_is_served_at_a_pitch_of_2p24(gpu, oracle, kind):
    c = small(oracle, kind)
    for xspec, yspec in ((WIDE["pitch_2p24"], None), (None, WIDE["pitch_2p24_64"])):
        gx, gy = big(c["xm"].shape, F, xspec, "xmap"), big(c["ym"].shape, F, yspec, "ymap")
        with launches() as l:
            _maps_roi(_warper(gpu, kind, c["f"]), c["K"], c["R"], c["win"], gx, gy)
        assert l.names & POLAR_LAUNCHES == {"polar_build_maps"}, l.names
        sync()
        assert PC.same_bits(gx.get(), c["xm"]) and PC.same_bits(gy.get(), c["ym"]), (xspec, yspec)
        gx.check(), gy.check()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("operand", ["src", "dimg", "dmask"])
def test_fused_roi_refuses_a_pitch_of_2p24(gpu, oracle, operand, out16, kind):
    """warp_with_mask's refusals come before the polar branch: each operand in turn at a pitch of 2^24 is ISX_ERR_UNSUPPORTED with not one
    byte written; one pitch below (2^24 - 64, 2^24 - 4 for the mask) the same call gives the model's tile and mask."""
    c = small(oracle, kind)
    dt = np.int16 if out16 else np.uint8
    warper = _warper(gpu, kind, c["f"])
    for spec, ok in ((("wide", None), False), (("wide_below", None), True)):
        s = big(c["img"].shape, np.uint8, spec if operand == "src" else None, "src", c["img"])
        di = big(c["wi"].shape, dt, spec if operand == "dimg" else None, "dst_img")
        dm = big(c["wm"].shape, np.uint8, spec if operand == "dmask" else None, "dst_mask")
        with launches() as l:
            if ok:
                _fused_roi(warper, s, c["K"], c["R"], c["win"], di, dm)
            else:
                refused(lambda: _fused_roi(warper, s, c["K"], c["R"], c["win"], di, dm))
        sync()
        if ok:
            assert l.names & POLAR_LAUNCHES == {"polar_warp_img_mask"}, l.names
            equal(di, c["wi"].astype(dt), operand), equal(dm, c["wm"], operand)
            di.check(), dm.check()
        else:
            assert not l.names & POLAR_LAUNCHES, l.names
            unchanged(di, dm)
        unchanged(s)


# ---- a source of 32768 pixels a side ---------------------------------------------------------------------------------------------------------
def long_source(kind, w, h):
    """A camera whose principal point lies 7.5 pixels before the far end of the long side, and the window that holds the images of the
    source points from 30 before that end to 30 past it: the model's maps cross 32767 along the long side."""
    f = 40.0
    K = np.array([[f, 0, w - 7.5 if w > h else 1.0], [0, f, h - 7.5 if h > w else 1.0], [0, 0, 1]], F)
    R = np.eye(3, dtype=F)
    m = P.from_rig(kind, f, K, R)
    far, near = max(w, h) - 1 + np.arange(-30, 31), np.arange(-1, 3)
    win = window_over(m, far if w > h else near, near if w > h else far)
    xm, ym = m.build_maps(win)
    return f, K, R, win, xm, ym


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", [(32768, 2), (2, 32768)])
def test_source_of_32768_pixels_a_side(gpu, oracle, w, h, kind):
    """warp_roi has no side limit for these kinds: the coordinates clamp to a short as cv::remap's do (oracle.remap over the model's maps,
    which reach past 32767).  The fused entry refuses 32768 a side and serves 32767."""
    f, K, R, win, xm, ym = long_source(kind, w, h)
    along = xm if w > h else ym
    assert along.max() > 32770 and along.min() < 32760 and not ((xm == -1) & (ym == -1)).any(), (along.min(), along.max())
    rng = np.random.default_rng(w + kind)
    warper = _warper(gpu, kind, f)
    for src, interp, border in ((GB.img_u8(rng, h, w), PC.LINEAR, PC.REFLECT), (GB.img_u8(rng, h, w, 1), PC.NEAREST, PC.CONST), (GB.img_u8(rng, h, w, 1), PC.LINEAR, PC.CONST)):
        want = oracle.remap(src, xm, ym, interp, border)
        s, d = big(src.shape, np.uint8, None, "src", src), big(want.shape, np.uint8, None, "dst")
        with launches() as l:
            _warp_roi(warper, s, K, R, interp, border, win, d)
        assert l.names & POLAR_LAUNCHES == {"polar_warp"}, l.names
        equal(d, want, (w, h, interp, border))
        d.check()
        unchanged(s)
    for cut, ok in ((0, False), (1, True)):                  # the fused entry: 32768 refused, 32767 served (the same camera and window)
        src = GB.img_u8(rng, h - cut * (h > w), w - cut * (w > h))
        wi = oracle.remap(src, xm, ym, PC.LINEAR, PC.REFLECT)
        wm = oracle.remap(np.full(src.shape[:2], 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST)
        s, di, dm = big(src.shape, np.uint8, None, "src", src), big(wi.shape, np.uint8, None, "dst_img"), big(wm.shape, np.uint8, None, "dst_mask")
        if ok:
            _fused_roi(warper, s, K, R, win, di, dm)
            sync()
            equal(di, wi, (w, h, "fused")), equal(dm, wm, (w, h, "fused mask"))
            assert (wm == 255).any() and (wm == 0).any()
            di.check(), dm.check()
        else:
            refused(lambda: _fused_roi(warper, s, K, R, win, di, dm))
            sync()
            unchanged(di, dm)
        unchanged(s)


# ---- a source past 2 GiB --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_warp_roi_reads_a_source_past_2_gib(gpu, oracle, kind):
    """129 rows at a pitch of 2^24: the last row starts 2^31 bytes behind the first.  warp_roi serves it (size_t offsets) and the bottom of
    the warped tile, which reads that row, equals the model.  (Skips only where the device has less free memory than the 4 GiB mat + 2 GiB.)"""
    w, h, f = 24, 129, 80.0
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F)
    R = P.ROTATIONS["identity"].astype(F)
    m = P.from_rig(kind, f, K, R)
    roi = [int(v) for v in m.detect_roi(w, h)[0]]
    assert roi[2] - roi[0] < 65536 and roi[3] - roi[1] < 65536
    win = window_over(m, np.arange(w), np.arange(h - 12, h))                  # where the last 12 source rows land
    xm, ym = m.build_maps(win)
    inside = (xm > 0) & (xm < w - 1) & (ym > 0) & (ym < h - 1)
    assert ym[inside].max() > 127 + 1 / 32 and inside.sum() > 50, (ym[inside].max(), inside.sum())          # bilinear taps in row 128
    src = PC.image(np.random.default_rng(90 + kind), h, w)
    want = oracle.remap(src, xm, ym, PC.LINEAR, PC.REFLECT)
    s = big(src.shape, np.uint8, ("tall31", P24), "src", src)
    assert (h - 1) * s.pitch == 1 << 31
    d = big(want.shape, np.uint8, None, "dst")
    with launches() as l:
        _warp_roi(_warper(gpu, kind, f), s, K, R, PC.LINEAR, PC.REFLECT, win, d)
    assert l.names & POLAR_LAUNCHES == {"polar_warp"}, l.names
    equal(d, want)
    d.check()
    unchanged(s)


# ---- the window --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_window_of_65536_is_invalid_and_65535_is_served(gpu, oracle, kind):
    """check_roi_sane measures a window as cv::Rect(tl, br) does, width = br.x - tl.x (the tile has one column more, W:150): a caller's window
    65536 wide or high is ISX_ERR_INVALID for every entry and nothing is written; 65535 wide, one row, is served - a tile of 65536 columns."""
    import torch
    w, h, f, K, R = P.rig(P.SIZES[0], "identity")
    m = P.from_rig(kind, f, K, R)
    warper = _warper(gpu, kind, f)
    src = PC.image(np.random.default_rng(3 + kind), h, w)
    dsrc = torch.from_numpy(src).cuda()
    for win in ((-30000, 4, 35536, 4), (4, -30000, 4, 35536)):
        shp = _shape(win)
        assert max(shp) == 65537 and max(win[2] - win[0], win[3] - win[1]) == 65536
        d, dm, gx, gy = (torch.full(shp + (3,), 7, dtype=torch.uint8, device="cuda"), torch.full(shp, 7, dtype=torch.uint8, device="cuda"),
                         torch.full(shp, 7, dtype=torch.float32, device="cuda"), torch.full(shp, 7, dtype=torch.float32, device="cuda"))
        for call in (lambda: _warp_roi(warper, dsrc, K, R, PC.LINEAR, PC.REFLECT, win, d), lambda: _fused_roi(warper, dsrc, K, R, win, d, dm),
                     lambda: _maps_roi(warper, K, R, win, gx, gy)):
            with pytest.raises(_lib.IsxError) as e:
                call()
            assert e.value.code == INVALID and "degenerate ROI" in e.value.msg, e.value.msg
            del e
        sync()
        assert all(bool((t == 7).all()) for t in (d, dm, gx, gy))
    win = (-30000, 4, 35535, 4)
    xm, ym = m.build_maps(win)
    assert xm.shape == (1, 65536) and win[2] - win[0] == 65535
    d, gx, gy = big((1, 65536, 3), np.uint8, None, "dst"), big((1, 65536), F, None, "xmap"), big((1, 65536), F, None, "ymap")
    s = big(src.shape, np.uint8, None, "src", src)
    _warp_roi(warper, s, K, R, PC.LINEAR, PC.REFLECT, win, d)
    _maps_roi(warper, K, R, win, gx, gy)
    sync()
    equal(d, oracle.remap(src, xm, ym, PC.LINEAR, PC.REFLECT))
    assert PC.same_bits(gx.get(), xm) and PC.same_bits(gy.get(), ym)
    d.check(), gx.check(), gy.check()
    unchanged(s)
