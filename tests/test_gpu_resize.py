"""isx_resize and isx_mask_dilate_resize_and on the GPU against the NumPy model (tests/helpers/resize_np.py), np.array_equal throughout: the
four types x both interpolations on host and device mats over the size pairs that reach every branch of the kernels, pitched views that
start at an odd byte, a captured resize -> dilate_resize_and chain, the error codes, and the fused mask stage against the model and against
the three calls it replaces.

Sizes are rows x cols.  The area rule of INTER_LINEAR applies where the SOURCE is twice the destination in both directions; the specification's
table lists its pairs in the upscaling direction (37 x 53 -> 74 x 106, 37 x 106 -> 74 x 106; the mask stage's 23 x 31 -> 46 x 62), which the
general path takes, so each is run in both directions here: the downscaling one is what reaches the rule (and the one-direction-only exception)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import resize_np as R  # noqa: E402

from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7

# (source rows, cols) -> (destination rows, cols)
PAIRS = [((37, 53), (74, 106)),        # the specification's "both ratios 2", as it lists it: an upscale by two, the general path
         ((74, 106), (37, 53)),        # ... and the direction the area rule applies in
         ((37, 106), (74, 106)),       # twice in one direction only, as listed
         ((74, 106), (37, 106)),       # ... and downscaling: half the rows only, not the rule
         ((74, 106), (74, 53)),        # half the columns only
         ((31, 45), (101, 131)),       # non-integer upscale, a partial 4-pixel group, a partial block of columns
         ((101, 131), (31, 45)),       # plain downscale
         ((1, 1), (5, 7)), ((1, 9), (3, 4)),      # one-pixel sources
         ((29, 43), (29, 43)),         # equal sizes
         ((3, 300), (5, 1100))]        # a row longer than one block's span of columns (256)
TYPES = [(np.uint8, 1), (np.uint8, 3), (np.float32, 1), (np.float32, 3)]


def _src(dtype, cn, shape, seed):
    rng = np.random.default_rng(seed)
    full = shape + ((cn,) if cn > 1 else ())
    if dtype == np.uint8:
        return rng.integers(0, 256, full, dtype=np.uint8)
    # negative values and magnitudes up to 1e6: a fused multiply-add would round differently
    return (rng.standard_normal(full) * 10.0 ** rng.uniform(0, 6, full)).astype(np.float32)


_MODEL = {}


def _want(dtype, cn, s, d, interp):
    """the model's answer, computed once per case and left unchanged"""
    key = (np.dtype(dtype).name, cn, s, d, interp)
    if key not in _MODEL:
        src = _src(dtype, cn, s, 1000 * s[0] + 100 * s[1] + 10 * d[0] + d[1] + cn)
        out = R.resize(src, (d[1], d[0]), interp)
        src.setflags(write=False); out.setflags(write=False)
        _MODEL[key] = (src, out)
    return _MODEL[key]


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("s,d", PAIRS, ids=["%dx%d-%dx%d" % (s + d) for s, d in PAIRS])
def test_resize_matches_the_model(gpu, s, d, where):
    import torch
    for dtype, cn in TYPES:
        for interp in (R.LINEAR, R.NEAREST):
            src, want = _want(dtype, cn, s, d, interp)
            a = torch.from_numpy(src.copy()).cuda() if where == "device" else src.copy()
            got = gpu.resize(a, (d[1], d[0]), interpolation=interp)
            if where == "device":
                torch.cuda.synchronize()
            g = _np(got)
            assert g.dtype == want.dtype and g.shape == want.shape
            assert np.array_equal(g, want), (np.dtype(dtype).name, cn, interp, int((g != want).sum()))
            assert np.array_equal(_np(a), src)


def test_known_answers_and_factors(gpu):
    assert gpu.resize(np.array([[0, 255]], np.uint8), (4, 1)).tolist() == [[0, 64, 191, 255]]
    assert gpu.resize(np.array([[1, 2], [3, 5]], np.uint8), (1, 1)).tolist() == [[3]]
    src = _src(np.uint8, 3, (35, 45), 5)
    got = gpu.resize(src, fx=0.5, fy=0.5)              # 22.5 -> 22 columns, 17.5 -> 18 rows: ties to even
    assert got.shape == (18, 22, 3) and np.array_equal(got, R.resize(src, (22, 18)))
    with pytest.raises(gpu.IsxError) as e:
        gpu.resize(src, fx=0.01, fy=0.01)
    assert e.value.code == ERR_SIZE


def _raw_mat(buf_ptr, offset, shape, dtype, cn, pitch, device):
    t = {("uint8", 1): _lib.ISX_8UC1, ("uint8", 3): _lib.ISX_8UC3, ("float32", 1): _lib.ISX_32FC1, ("float32", 3): _lib.ISX_32FC3}[(np.dtype(dtype).name, cn)]
    return _lib.IsxMat(buf_ptr + offset, shape[0], shape[1], t, pitch, device)


@pytest.mark.parametrize("where", ["device", "host"])
def test_pitched_views_starting_at_an_odd_byte(gpu, where):
    """source and destination rows at odd addresses with odd pitches (for CV_32F: floats that are not even 4-byte aligned), inside buffers of
    seeded bytes: the result equals the model and no byte around the destination's rows changes"""
    import torch
    lib = _lib.load()
    s, d = (31, 45), (101, 131)
    for dtype, cn in TYPES:
        es = np.dtype(dtype).itemsize * cn
        for interp in (R.LINEAR, R.NEAREST):
            src, want = _want(dtype, cn, s, d, interp)
            sp, dp = s[1] * es + 7, d[1] * es + 13                     # odd pitches
            if sp % 2 == 0:
                sp += 1
            if dp % 2 == 0:
                dp += 1
            so, do = 33, 77                                            # odd offsets into 256-byte aligned buffers
            sbuf = np.random.default_rng(1).integers(0, 256, so + s[0] * sp + 64, dtype=np.uint8)
            dbuf = np.random.default_rng(2).integers(0, 256, do + d[0] * dp + 64, dtype=np.uint8)
            rows = np.lib.stride_tricks.as_strided(sbuf[so:], (s[0], s[1] * es), (sp, 1))
            rows[...] = src.reshape(s[0], -1).view(np.uint8)
            before = dbuf.copy()
            if where == "device":
                ts, td = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf).cuda()
                assert ts.data_ptr() % 256 == 0 and td.data_ptr() % 256 == 0
                ms, md = _raw_mat(ts.data_ptr(), so, s, dtype, cn, sp, 0), _raw_mat(td.data_ptr(), do, d, dtype, cn, dp, 0)
            else:
                ms, md = _raw_mat(sbuf.ctypes.data, so, s, dtype, cn, sp, -1), _raw_mat(dbuf.ctypes.data, do, d, dtype, cn, dp, -1)
            _lib.check(lib.isx_resize(C.byref(ms), C.byref(md), interp, 0, None))
            if where == "device":
                torch.cuda.synchronize()
                dbuf = td.cpu().numpy()
                assert np.array_equal(ts.cpu().numpy(), sbuf)
            got = np.lib.stride_tricks.as_strided(dbuf[do:], (d[0], d[1] * es), (dp, 1))
            assert np.array_equal(got, want.reshape(d[0], -1).view(np.uint8)), (np.dtype(dtype).name, cn, interp)
            keep = np.ones(dbuf.size, bool)
            for y in range(d[0]):
                keep[do + y * dp:do + y * dp + d[1] * es] = False
            assert np.array_equal(dbuf[keep], before[keep]), (np.dtype(dtype).name, cn, interp)


def test_error_codes(gpu):
    lib = _lib.load()
    u1, u3, f1 = np.zeros((8, 9), np.uint8), np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9), np.float32)
    i16, i32 = np.zeros((8, 9, 3), np.int16), np.zeros((8, 9), np.int32)

    def rc(a, b, interp=R.LINEAR):
        ma, mb = _lib.as_mat(a), _lib.as_mat(b)
        return lib.isx_resize(C.byref(ma), C.byref(mb), interp, 0, None)
    assert rc(u1, np.zeros((4, 5), np.uint8)) == 0
    assert rc(u1, np.zeros((4, 5, 3), np.uint8)) == ERR_TYPE and rc(u1, np.zeros((4, 5), np.float32)) == ERR_TYPE and rc(u3, u1.copy()) == ERR_TYPE
    assert rc(i16, i16.copy()) == ERR_UNSUPPORTED and rc(i32, i32.copy()) == ERR_UNSUPPORTED
    for interp in (2, 3, 4, 5, -1, R.LINEAR | 0x100):           # CUBIC, AREA, LANCZOS4, LINEAR_EXACT, nonsense, the warper's ties-even flag
        assert rc(f1, f1.copy(), interp) == ERR_UNSUPPORTED, interp
    for rows, cols in ((0, 9), (8, 0), (0, 0), (-1, 9)):
        e = _lib.as_mat(u1)
        e.rows, e.cols = rows, cols
        full = _lib.as_mat(u1.copy())
        assert lib.isx_resize(C.byref(e), C.byref(full), R.LINEAR, 0, None) == ERR_SIZE
        assert lib.isx_resize(C.byref(full), C.byref(e), R.LINEAR, 0, None) == ERR_SIZE
        assert lib.isx_mask_dilate_resize_and(C.byref(e), None, 3, 3, C.byref(full), 0, None) == ERR_SIZE
        assert lib.isx_mask_dilate_resize_and(C.byref(full), None, 3, 3, C.byref(e), 0, None) == ERR_SIZE
    assert lib.isx_resize(None, C.byref(_lib.as_mat(u1)), R.LINEAR, 0, None) == ERR_INVALID

    def rd(seam, warped, out, kw=3, kh=3):
        ms, mo = _lib.as_mat(seam), _lib.as_mat(out)
        mw = _lib.as_mat(warped) if warped is not None else None
        return lib.isx_mask_dilate_resize_and(C.byref(ms), C.byref(mw) if mw is not None else None, kw, kh, C.byref(mo), 0, None)
    out = np.zeros((20, 30), np.uint8)
    assert rd(u1, None, out) == 0 and rd(u1, out.copy(), out) == 0
    assert rd(u1, np.zeros((20, 31), np.uint8), out) == ERR_SIZE and rd(u1, np.zeros((20, 30), np.float32), out) == ERR_SIZE
    assert rd(f1, None, out) == ERR_TYPE and rd(u1, None, np.zeros((20, 30), np.float32)) == ERR_TYPE and rd(u3, None, out) == ERR_TYPE
    for kw, kh in ((0, 3), (3, 0), (4097, 3), (3, 4097), (-1, -1)):          # isx_mask_dilate_and's element limit
        assert rd(u1, None, out, kw, kh) == ERR_INVALID
    with pytest.raises(gpu.IsxError) as e:
        gpu.dilate_resize_and(u1, out, other=out)
    assert e.value.code == ERR_INVALID


# ---- isx_mask_dilate_resize_and --------------------------------------------------------------------------------------------------------------

def _seam_mask(h, w, seed):
    """random 0 / 255 blobs, some touching every border"""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    for _ in range(5):
        y, x = int(rng.integers(2, h - 4)), int(rng.integers(2, w - 4))
        m[y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 6))] = 255
    m[0, 3:6] = 255; m[h - 1, w - 7:w - 4] = 255; m[8:11, 0] = 255; m[4:6, w - 1] = 255       # one blob on each border
    m[h - 1, 0] = 255                                                                          # and a corner
    m[rng.random((h, w)) < 0.03] = 255
    return m


MASK_SIZES = [((23, 31), (91, 127)), ((23, 31), (46, 62)), ((23, 31), (23, 31)),
              ((46, 62), (23, 31))]                   # the small mask twice the output: the area rule inside the fused kernel
ELEMENTS = [(3, 3), (1, 1), (20, 20), (2, 5)]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("s,d", MASK_SIZES, ids=["%dx%d-%dx%d" % (s + d) for s, d in MASK_SIZES])
def test_dilate_resize_and_matches_the_model_and_the_three_calls(gpu, s, d, where):
    import torch
    seam = _seam_mask(s[0], s[1], 100 + s[0])
    rng = np.random.default_rng(d[0])
    warped = np.where(rng.random(d) < 0.7, 255, 0).astype(np.uint8)
    warped[rng.random(d) < 0.05] = 0x5a                     # the AND is bitwise, not a comparison
    put = (lambda a: torch.from_numpy(a.copy()).cuda()) if where == "device" else (lambda a: a.copy())
    ds, dw = put(seam), put(warped)
    for kw, kh in ELEMENTS:
        dil = R.dilate(seam, kw, kh)
        grey = R.resize(dil, (d[1], d[0]))
        assert np.array_equal(R.dilate_resize_and(seam, warped, kw, kh), grey & warped)
        # the three calls it replaces
        three = gpu.resize(gpu.dilate_and(ds, kw, kh), (d[1], d[0]))
        assert np.array_equal(_np(three), grey), (kw, kh)
        for w in (None, dw):
            got = gpu.dilate_resize_and(ds, (d[1], d[0]), kw, kh, other=w) if w is None else gpu.dilate_resize_and(ds, w, kw, kh)
            want = grey if w is None else grey & warped
            assert np.array_equal(_np(got), want), (kw, kh, w is None, int((_np(got) != want).sum()))
            assert np.array_equal(_np(got), _np(three) if w is None else _np(three) & warped)
    if d != s:
        assert len(np.unique(grey)) > 2                       # the resize's ramp is kept
    assert np.array_equal(_np(ds), seam) and np.array_equal(_np(dw), warped)
    # in place: out is the warped mask
    gpu.dilate_resize_and(ds, dw, 3, 3, out=dw)
    assert np.array_equal(_np(dw), R.dilate_resize_and(seam, warped, 3, 3))


# ---- stream capture ----------------------------------------------------------------------------------------------------------------------------

def test_captured_resize_then_mask_stage_replays(gpu):
    """resize -> dilate_resize_and on device mats captured on a side stream and replayed twice on rewritten inputs: every replay equals the
    eager calls and the model.  A captured call on host mats returns ISX_ERR_STATE with nothing enqueued and leaves the capture usable."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    H, W = 61, 83
    with torch.cuda.stream(s):
        img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        small = torch.zeros((23, 31, 3), dtype=torch.uint8, device="cuda")
        seam = torch.zeros((23, 31), dtype=torch.uint8, device="cuda")
        warped = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        out = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    host_img, host_small = np.zeros((H, W, 3), np.uint8), np.full((23, 31, 3), 7, np.uint8)
    g = torch.cuda.CUDAGraph()
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            gpu.resize(host_img, (31, 23), dst=host_small, stream=s)
        assert e.value.code == ERR_STATE and "host" in e.value.msg, e.value.msg
        with pytest.raises(gpu.IsxError) as e:
            gpu.resize(img, (31, 23), dst=host_small, stream=s)
        assert e.value.code == ERR_STATE
        with pytest.raises(gpu.IsxError) as e:
            gpu.dilate_resize_and(np.zeros((23, 31), np.uint8), warped, out=out, stream=s)
        assert e.value.code == ERR_STATE and "host" in e.value.msg, e.value.msg
        gpu.resize(img, (31, 23), dst=small, stream=s)
        gpu.dilate_resize_and(seam, warped, 3, 3, out=out, stream=s)
    assert (host_small == 7).all()
    for k in range(2):
        a = _src(np.uint8, 3, (H, W), 40 + k)
        m = _seam_mask(23, 31, 50 + k)
        w = np.where(np.random.default_rng(60 + k).random((H, W)) < 0.8, 255, 0).astype(np.uint8)
        with torch.cuda.stream(s):
            img.copy_(torch.from_numpy(a).cuda()); seam.copy_(torch.from_numpy(m).cuda()); warped.copy_(torch.from_numpy(w).cuda())
            small.zero_(); out.zero_()
        s.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert float(x[0]) == k + 1.0
        got_small, got_out = _np(small).copy(), _np(out).copy()
        assert np.array_equal(got_small, R.resize(a, (31, 23))) and np.array_equal(got_out, R.dilate_resize_and(m, w, 3, 3)), k
        with torch.cuda.stream(s):
            e_small = gpu.resize(img, (31, 23), stream=s)
            e_out = gpu.dilate_resize_and(seam, warped, 3, 3, stream=s)
        torch.cuda.synchronize()
        assert np.array_equal(_np(e_small), got_small) and np.array_equal(_np(e_out), got_out), k
