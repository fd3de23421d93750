"""isx_resize and isx_mask_dilate_resize_and where tests/test_gpu_resize.py, test_gpu_resize_guard.py and test_gpu_seam_scaled.py do not reach,
against the NumPy model (tests/helpers/resize_np.py), np.array_equal throughout (CV_32F on the uint32 views; NaNs by position only):

  a  seam masks of 1..4 rows x 1..5 columns - narrower than the 4 columns dilated_taps3 loads as one dword, so its pixel-by-pixel branch is the
     only one, and of 1 or 2 rows, where three of its four row indices clamp to one row - under six elements;
  b  the fused kernel at the ratio it was written for (7.4 x by 9.1 x: a lane's four pixels share a tap set or change it in the middle, its four
     rows reuse the cached taps), outputs around and beyond one wave's 256 pixels with the 3 x 3 element, steep and non-half downscales, one
     axis up and the other down, the largest element;
  c  steep and tiny resizes of all four types;
  d  the row and column limits of resize.hip, at them and one past them;
  e  values: 0 / 255 patterns on CV_8U (255 under both taps, the coefficient pairs, the vertical clamp), denormals, signed zeros, overflow to
     infinity, infinities and NaNs on CV_32F;
  f  the taps the device computes, (float)((dx + 0.5) * scale - 0.5) in double, on 416 pairs of lengths up to 4096 as rows and as columns;
  and the overlapping mats both entries reject.

Sizes are rows x cols."""
import ctypes as C
import gc
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import resize_np as R  # noqa: E402

from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 6
TYPES = [(np.uint8, 1), (np.uint8, 3), (np.float32, 1), (np.float32, 3)]
INTERPS = (R.LINEAR, R.NEAREST)


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _src(dtype, cn, shape, seed):
    """as tests/test_gpu_resize.py draws its sources: bytes, or floats of either sign and magnitudes up to 1e6"""
    rng = np.random.default_rng(seed)
    full = tuple(shape) + ((cn,) if cn > 1 else ())
    if dtype == np.uint8:
        return rng.integers(0, 256, full, dtype=np.uint8)
    return (rng.standard_normal(full) * 10.0 ** rng.uniform(0, 6, full)).astype(np.float32)


def _resize_equals_model(gpu, src, d, interp, note):
    """src (host array) -> d = (rows, cols) on device mats: the result's bits are the model's, the source is unchanged"""
    want = R.resize(src, (d[1], d[0]), interp)
    a = _dev(src)
    got = _np(gpu.resize(a, (d[1], d[0]), interpolation=interp))
    assert got.dtype == want.dtype and got.shape == want.shape, note
    assert np.array_equal(_bits(got), _bits(want)), (note, int((_bits(got) != _bits(want)).sum()), np.argwhere(_bits(got) != _bits(want))[:3])
    assert np.array_equal(_bits(_np(a)), _bits(src)), note


# ---- a. small seam masks ----------------------------------------------------------------------------------------------------------------------

SMALL_ELEMENTS = [(3, 3), (1, 1), (2, 2), (4, 1), (1, 5), (7, 9)]
SMALL_OUTPUTS = [(1, 1), (1, 3), (3, 2), (5, 7), (19, 37)]


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_small_seam_masks(gpu, rows):
    """Every seam mask of `rows` x 1..5 with 0 or 1..255 at density 0.4, to 1 x 1, 1 x 3, 3 x 2, 5 x 7, 19 x 37 and (both even) its half, six
    elements, with and without a warped mask; the 3 x 3 element on host mats too."""
    rng = np.random.default_rng(4100 + rows)
    for cols in (1, 2, 3, 4, 5):
        seam = np.where(rng.random((rows, cols)) < 0.4, rng.integers(1, 256, (rows, cols)), 0).astype(np.uint8)
        seam[rng.integers(0, rows), rng.integers(0, cols)] = 255                    # never empty
        ds = _dev(seam)
        outs = SMALL_OUTPUTS + ([(rows // 2, cols // 2)] if rows % 2 == 0 and cols % 2 == 0 else [])
        for d in outs:
            warped = rng.integers(0, 256, d, dtype=np.uint8)
            dw = _dev(warped)
            for kw, kh in SMALL_ELEMENTS:
                grey = R.dilate_resize_and(seam, None, kw, kh, (d[1], d[0]))
                wants = {False: grey, True: grey & warped}
                places = [("device", ds, dw)] + ([("host", seam.copy(), warped.copy())] if (kw, kh) == (3, 3) else [])
                for where, s, w in places:
                    for with_warped in (False, True):
                        got = gpu.dilate_resize_and(s, w, kw, kh) if with_warped else gpu.dilate_resize_and(s, (d[1], d[0]), kw, kh)
                        g = _np(got)
                        assert g.shape == d and np.array_equal(g, wants[with_warped]), ((rows, cols), d, (kw, kh), where, with_warped, g.tolist(),
                                                                                       wants[with_warped].tolist())
                    assert np.array_equal(_np(s), seam) and np.array_equal(_np(w), warped)


# ---- b. ratio and width of the fused kernel ------------------------------------------------------------------------------------------------

FUSED = [((5, 113), (37, 1030)),                                   # 7.4 x by 9.1 x, five workgroups in x
         ((7, 29), (33, 255)), ((7, 29), (33, 256)), ((7, 29), (33, 257)), ((7, 29), (33, 513)),      # around one wave's 256 pixels
         ((61, 83), (7, 9)),                                       # steep downscale
         ((46, 62), (19, 27)),                                     # non-half downscale
         ((23, 31), (91, 13)), ((9, 120), (40, 14))]               # up in y, down in x
FUSED_ELEMENTS = [(3, 3), (2, 5)]


def _blob_mask(shape, seed):
    """mostly 0 / 255 at density 0.08 with a few other values: a 3 x 3 dilate leaves both zeros and ramps"""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random(shape) < 0.08, 255, 0).astype(np.uint8)
    few = rng.random(shape) < 0.02
    m[few] = rng.integers(1, 255, shape, dtype=np.uint8)[few]
    m[shape[0] // 2, shape[1] // 2] = 255
    return m


def _warped_mask(shape, seed):
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(shape) < 0.7, 255, 0).astype(np.uint8)
    w[rng.random(shape) < 0.1] = 0x5a                               # the AND is bitwise, not a comparison
    w.flat[0] = 0x5a
    return w


def _fused_case(gpu, s, d, elements, seed):
    seam, warped = _blob_mask(s, seed), _warped_mask(d, seed + 1)
    assert (warped == 0x5a).any()
    ds = _dev(seam)
    for kw, kh in elements:
        grey = R.dilate_resize_and(seam, None, kw, kh, (d[1], d[0]))
        want = grey & warped
        dw = _dev(warped)
        got = _np(gpu.dilate_resize_and(ds, dw, kw, kh))
        assert np.array_equal(got, want), (s, d, (kw, kh), int((got != want).sum()), np.argwhere(got != want)[:3])
        assert np.array_equal(_np(dw), warped) and np.array_equal(_np(ds), seam)
        gpu.dilate_resize_and(ds, dw, kw, kh, out=dw)               # in place: out is the warped mask
        got = _np(dw)
        assert np.array_equal(got, want), (s, d, (kw, kh), "in place", int((got != want).sum()), np.argwhere(got != want)[:3])
        yield (kw, kh), grey


@pytest.mark.parametrize("s,d", FUSED, ids=["%dx%d-%dx%d" % (s + d) for s, d in FUSED])
def test_fused_kernel_ratios_and_widths(gpu, s, d):
    if (s, d) == ((5, 113), (37, 1030)):
        # a lane owns output columns 4 g .. 4 g + 3: at 9.1 x most lanes sit on one source column, and some change it in the middle
        sx, _ = R.col_taps(s[1], d[1])
        lanes = sx[:d[1] // 4 * 4].reshape(-1, 4)
        assert (lanes.min(axis=1) != lanes.max(axis=1)).any() and (lanes.min(axis=1) == lanes.max(axis=1)).any()
        sy0, _, _ = R.row_taps(s[0], d[0])
        rows = sy0[:d[0] // 4 * 4].reshape(-1, 4)
        assert (rows.min(axis=1) == rows.max(axis=1)).any()          # and all DR_ROWS rows of some lane reuse one tap set
    for element, grey in _fused_case(gpu, s, d, FUSED_ELEMENTS, 7000 + s[0] + d[1]):
        if d[0] > s[0]:                                              # up-scaled (in y at least): the resize's grey ramp is kept
            assert len(np.unique(grey)) > 2, (s, d, element)


def test_fused_kernel_largest_element(gpu):
    """4 x 5 under the 4096 x 4096 element, the largest allowed, to 9 x 11.  Every window covers the whole mask, so the dilated mask is the
    constant max(mask) and so is the model's output: this one up-scaled case has no ramp to keep, by construction."""
    for element, grey in _fused_case(gpu, (4, 5), (9, 11), [(4096, 4096)], 7100):
        assert (grey == 255).all()


# ---- c. steep and tiny resizes ---------------------------------------------------------------------------------------------------------------

STEEP = [((36, 300), (4, 33)), ((4, 33), (36, 300)),
         ((4, 300), (36, 33)),                                      # up in y, down in x
         ((40, 2060), (5, 226)), ((5, 226), (40, 2060)),
         ((31, 45), (1, 1))]


@pytest.mark.parametrize("s,d", STEEP, ids=["%dx%d-%dx%d" % (s + d) for s, d in STEEP])
def test_steep_resizes(gpu, s, d):
    for dtype, cn in TYPES:
        src = _src(dtype, cn, s, 100 * s[0] + s[1] + d[0] + cn)
        for interp in INTERPS:
            _resize_equals_model(gpu, src, d, interp, (np.dtype(dtype).name, cn, interp))


def test_tiny_sources(gpu):
    """every source of 1..3 x 1..3 to 1 x 1, 2 x 3 and 7 x 5"""
    for sh in (1, 2, 3):
        for sw in (1, 2, 3):
            for dtype, cn in TYPES:
                src = _src(dtype, cn, (sh, sw), 10 * sh + sw + cn)
                for d in ((1, 1), (2, 3), (7, 5)):
                    for interp in INTERPS:
                        _resize_equals_model(gpu, src, d, interp, ((sh, sw), d, np.dtype(dtype).name, cn, interp))


# ---- d. the row and column limits ------------------------------------------------------------------------------------------------------------

def _limits():
    """RZ_MAX_ROWS as tools/fuzz_parity.py reads a kernel's constants; RZ_MAX_COLS is written as a shift, which that reader leaves out"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    with open(os.path.join(ROOT, "imagestitch_amd", "csrc", "resize.hip")) as f:
        shift = re.search(r"\bRZ_MAX_COLS\s*=\s*1\s*<<\s*(\d+)\s*;", f.read())
    return fuzz_parity._kernel_consts("resize.hip")["RZ_MAX_ROWS"], 1 << int(shift.group(1))


def test_at_the_row_limit(gpu):
    max_rows, max_cols = _limits()
    assert (max_rows, max_cols) == (262140, 1 << 26)
    small = _src(np.uint8, 1, (3, 2), 1)
    for interp in INTERPS:
        _resize_equals_model(gpu, small, (max_rows, 1), interp, ("up", interp))          # 65535 workgroups in y
    tall = _src(np.uint8, 1, (max_rows, 1), 2)
    for interp in INTERPS:
        _resize_equals_model(gpu, tall, (3, 2), interp, ("down", interp))
    # the mask stage too: 16384 workgroups in y, and a source as high as the limit
    seam = np.array([[0, 255], [9, 0], [0, 0]], np.uint8)
    got = _np(gpu.dilate_resize_and(_dev(seam), (1, max_rows), 3, 3))
    assert np.array_equal(got, R.dilate_resize_and(seam, None, 3, 3, (1, max_rows)))
    tall_mask = np.where(tall > 200, 255, 0).astype(np.uint8)
    got = _np(gpu.dilate_resize_and(_dev(tall_mask), (2, 3), 1, 1))
    assert np.array_equal(got, R.resize(tall_mask, (2, 3)))         # (the 1 x 1 element dilates nothing; the model's dilate walks rows in Python)


def test_past_the_limits(gpu):
    """one row or one column more is ISX_ERR_UNSUPPORTED from both entries, as source and as destination, and the output keeps its bytes"""
    lib = _lib.load()
    max_rows, max_cols = _limits()
    small = np.full((3, 2), 9, np.uint8)
    tall = np.full((max_rows + 1, 1), 7, np.uint8)
    wide = np.full((1, max_cols + 1), 7, np.uint8)                  # a real 64 MB array
    for big in (tall, wide):
        for src, dst in ((big, small), (small, big)):
            dst[...] = 7
            ms, md = _lib.as_mat(src), _lib.as_mat(dst)
            for interp in INTERPS:
                assert lib.isx_resize(C.byref(ms), C.byref(md), interp, 0, None) == ERR_UNSUPPORTED
            assert (dst == 7).all()
            assert lib.isx_mask_dilate_resize_and(C.byref(ms), None, 3, 3, C.byref(md), 0, None) == ERR_UNSUPPORTED
            assert (dst == 7).all()
            mw = _lib.as_mat(np.full(dst.shape, 255, np.uint8)) if dst is small else md       # (with an AND operand of out's size)
            assert lib.isx_mask_dilate_resize_and(C.byref(ms), C.byref(mw), 3, 3, C.byref(md), 0, None) == ERR_UNSUPPORTED
            assert (dst == 7).all()
            small[...] = 9


# ---- e. values --------------------------------------------------------------------------------------------------------------------------------

VALUE_SIZES = [((31, 45), (101, 131)), ((101, 131), (31, 45)), ((74, 106), (37, 53))]          # the last: the area rule
_IDS = ["%dx%d-%dx%d" % (s + d) for s, d in VALUE_SIZES]


def _patterns(shape, cn):
    y, x = np.indices(shape)
    base = {"zeros": np.zeros(shape, np.uint8), "all_255": np.full(shape, 255, np.uint8), "checkerboard": (((x + y) & 1) * 255).astype(np.uint8),
            "vertical_stripes": ((x & 1) * 255).astype(np.uint8), "horizontal_stripes": ((y & 1) * 255).astype(np.uint8)}
    return {k: (np.repeat(v[:, :, None], 3, axis=2) if cn == 3 else v) for k, v in base.items()}


@pytest.mark.parametrize("s,d", VALUE_SIZES, ids=_IDS)
def test_byte_patterns(gpu, s, d):
    for cn in (1, 3):
        for name, src in _patterns(s, cn).items():
            for interp in INTERPS:
                _resize_equals_model(gpu, src, d, interp, (name, cn, interp))


F32 = np.float32
FINITE_SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3.4028235e38, -3.4028235e38, 1.0, -1.0], F32)


def _float_mixture(shape, cn, seed, non_finite):
    """Normal noise with patches (1..3 x 1..4 pixels, so that both taps of an output pixel fall on one kind) of +-0.0, +-1e-40, +-1.4e-45,
    +-FLT_MAX and +-1.0, and single pixels of them; with non_finite, of +-inf and NaN too."""
    rng = np.random.default_rng(seed)
    full = tuple(shape) + ((cn,) if cn > 1 else ())
    a = (rng.standard_normal(full) * 10.0 ** rng.uniform(-3, 3, full)).astype(F32)
    kinds = FINITE_SPECIALS if not non_finite else np.concatenate([FINITE_SPECIALS, np.array([np.inf, -np.inf, np.nan], F32)])
    for _ in range(shape[0] * shape[1] // 6):
        y, x = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))
        a[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 5))] = kinds[int(rng.integers(0, len(kinds)))]
    single = rng.random(full) < 0.1
    a[single] = kinds[rng.integers(0, len(kinds), full)][single]
    if non_finite:                                                   # the clamped first column reads two taps with fx = 0: a finite one, then an infinity
        a[2:5, 0], a[2:5, 1] = F32(2.0), F32(np.inf)
    return a


def _is_denormal(a):
    b = np.ascontiguousarray(a).view(np.uint32)
    return ((b & 0x7f800000) == 0) & ((b & 0x007fffff) != 0)


def _can_overflow(s, d):
    """Whether finite inputs can give an infinity at these sizes.  The area rule adds four values: two FLT_MAX overflow.  The general path
    weighs two values by 1 - f and f, twice; rounding is monotonic, so no input gives more than FLT_MAX under every tap does, and that is
    fl(fl(M (1 - f)) + fl(M f)) per axis - computed here for every column and row of the pair."""
    if R.is_half(s, d):
        return True
    m = F32(3.4028235e38)
    _, fx = R.col_taps(s[1], d[1])
    _, _, fy = R.row_taps(s[0], d[0])
    with np.errstate(over="ignore"):
        return any(bool(np.isinf(((m * (F32(1) - f)).astype(F32) + (m * f).astype(F32)).astype(F32)).any()) for f in (fx, fy))


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("s,d", VALUE_SIZES, ids=_IDS)
def test_float_specials_finite(gpu, s, d, seed):
    """Denormals in and out, signed zeros, sums that overflow: bit for bit.  (A build that flushes denormals to zero fails this.)  The model's
    output must hold a denormal, a -0.0 and an infinity for the case to prove anything - the infinity only where these sizes can overflow at
    all (_can_overflow): of the three pairs that is the area rule's; at the taps of the other two even FLT_MAX under all four stays FLT_MAX,
    and the test asserts that the model's output then holds no infinity."""
    for cn in (1, 3):
        src = _float_mixture(s, cn, 100 * seed + cn, False)
        assert np.isfinite(src).all() and _is_denormal(src).any()
        want = R.resize(src, (d[1], d[0]), R.LINEAR)
        assert _is_denormal(want).any() and (want.view(np.uint32) == 0x80000000).any(), (cn, "the case proves nothing")
        assert np.isinf(want).any() == _can_overflow(s, d), (cn, "the case proves nothing")
        for interp in INTERPS:
            _resize_equals_model(gpu, src, d, interp, (cn, interp))


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("s,d", VALUE_SIZES, ids=_IDS)
def test_float_specials_non_finite(gpu, s, d, seed):
    """With +-inf and NaN among the inputs: the NaNs at the model's positions (payload and sign not compared), every other value bit for bit."""
    for cn in (1, 3):
        src = _float_mixture(s, cn, 200 * seed + cn, True)
        assert np.isnan(src).any() and np.isinf(src).any()
        want = R.resize(src, (d[1], d[0]), R.LINEAR)
        if d[1] > s[1]:                                              # an upscale clamps its first column to (sx, fx) = (0, 0), and 2 + inf * 0 is NaN
            sx, fx = R.col_taps(s[1], d[1])
            sy0, sy1, _ = R.row_taps(s[0], d[0])
            assert sx[0] == 0 and fx[0] == 0 and s[1] > 1
            rows = [y for y in range(d[0]) if 2 <= sy0[y] and sy1[y] <= 4]
            assert rows and np.isnan(want[rows, 0]).all() and not np.isnan(src[2:5, :2]).any()
        for interp in INTERPS:
            w = want if interp == R.LINEAR else R.resize(src, (d[1], d[0]), interp)
            got = _np(gpu.resize(_dev(src), (d[1], d[0]), interpolation=interp))
            assert got.dtype == w.dtype and got.shape == w.shape
            assert np.array_equal(np.isnan(got), np.isnan(w)), (cn, interp, np.argwhere(np.isnan(got) != np.isnan(w))[:3])
            ok = ~np.isnan(w)
            assert np.array_equal(got.view(np.uint32)[ok], w.view(np.uint32)[ok]), (cn, interp, int((got.view(np.uint32)[ok] != w.view(np.uint32)[ok]).sum()))


# ---- f. tap sweep -----------------------------------------------------------------------------------------------------------------------------

def sweep_pairs():
    """(n_src, n_dst): 400 seeded pairs from 1..4096, the 4K <-> 0.1 Mpix lengths, and 2 k, 2 k + 1, 2 k - 1 -> k"""
    rng = np.random.default_rng(20261019)
    pairs = [(int(a), int(b)) for a, b in rng.integers(1, 4097, (400, 2))]
    pairs += [(3840, 422), (2160, 237), (422, 3840), (237, 2160)]
    for k in (1, 2, 37, 1000):
        pairs += [(2 * k, k), (2 * k + 1, k), (2 * k - 1, k)]
    return pairs


def sweep_inputs(n_src):
    """per source length: floats as _src draws them, the indices 0 .. n - 1 as floats, noise bytes"""
    return (_src(np.float32, 1, (n_src,), 31 * n_src + 1), np.arange(n_src, dtype=np.float32), _src(np.uint8, 1, (n_src,), 31 * n_src + 2))


def test_tap_sweep(gpu):
    """Each pair as a row (1 x n) and as a column (n x 1): CV_32FC1 LINEAR on floats (fx's last bit moves the result), CV_32FC1 NEAREST on
    arange (the output is the tap index), CV_8UC1 LINEAR on noise.  Prints how many pairs and pixels differ before it asserts."""
    import torch
    pairs = sweep_pairs()
    assert len(pairs) == 416
    kinds = ("float LINEAR", "float NEAREST of arange", "byte LINEAR")
    bad_pairs, bad_pixels, first = [0, 0, 0], [0, 0, 0], None
    for n_src, n_dst in pairs:
        values, index, noise = sweep_inputs(n_src)
        runs = [(values, R.LINEAR), (index, R.NEAREST), (noise, R.LINEAR)]
        got = []
        for a, interp in runs:
            t = _dev(a)
            got.append((gpu.resize(t.view(1, n_src), (n_dst, 1), interpolation=interp), gpu.resize(t.view(n_src, 1), (1, n_dst), interpolation=interp)))
        torch.cuda.synchronize()
        for k, ((a, interp), (row, col)) in enumerate(zip(runs, got)):
            diff = 0
            for g, want in ((row, R.resize(a.reshape(1, n_src), (n_dst, 1), interp)), (col, R.resize(a.reshape(n_src, 1), (1, n_dst), interp))):
                assert g.shape == want.shape
                diff += int((_bits(_np(g)) != _bits(want)).sum())
            if diff:
                bad_pairs[k] += 1; bad_pixels[k] += diff
                first = first or (n_src, n_dst, kinds[k])
    for k, kind in enumerate(kinds):
        print("tap sweep, %s: %d of %d pairs differ, %d pixels" % (kind, bad_pairs[k], len(pairs), bad_pixels[k]))
    assert bad_pairs == [0, 0, 0], (bad_pairs, bad_pixels, first)


# ---- overlapping mats ---------------------------------------------------------------------------------------------------------------------------

def _mat(ptr, rows, cols, step, device, type_=None):
    return _lib.IsxMat(ptr, rows, cols, _lib.ISX_8UC1 if type_ is None else type_, step, device)


@pytest.mark.parametrize("where", ["device", "host"])
def test_overlapping_mats_are_rejected(gpu, where):
    """A dst that shares a byte with src, an out that shares one with seam_mask, and an out that lies over warped_mask without being the same
    view of it: ISX_ERR_INVALID with both mats named and not one byte written.  Views of one buffer that lie one after the other work."""
    lib = _lib.load()
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, (40, 64), dtype=np.uint8)
    buf = _dev(host) if where == "device" else host.copy()
    base = buf.data_ptr() if where == "device" else buf.ctypes.data
    device = 0 if where == "device" else -1
    pitch = 64

    def resize(src, dst):
        return lib.isx_resize(C.byref(src), C.byref(dst), R.LINEAR, 0, None)

    def stage(seam, warped, out):
        return lib.isx_mask_dilate_resize_and(C.byref(seam), C.byref(warped) if warped is not None else None, 3, 3, C.byref(out), 0, None)

    def rejected(rc, *names):
        msg = lib.isx_last_error().decode()
        assert rc == ERR_INVALID and all(n in msg for n in names), (rc, msg)
        assert np.array_equal(_np(buf), host)

    whole = _mat(base, 40, 64, pitch, device)
    rejected(resize(whole, whole), "src", "dst")                                              # identical mats
    rejected(resize(whole, _mat(base + 5 * pitch + 7, 10, 20, pitch, device)), "src", "dst")      # a sub-view of src's buffer
    rejected(resize(_mat(base, 10, 20, pitch, device), _mat(base + 9 * pitch + 19, 10, 20, pitch, device)), "src", "dst")      # one shared byte
    rejected(resize(_mat(base, 10, 20, pitch, device), _mat(base + 30, 10, 20, pitch, device)), "src", "dst")      # side by side: the ranges interleave
    rejected(stage(whole, None, whole), "seam_mask", "out")
    rejected(stage(whole, None, _mat(base + 5 * pitch + 7, 10, 20, pitch, device)), "seam_mask", "out")
    top, low = _mat(base, 10, 64, pitch, device), _mat(base + 20 * pitch, 16, 40, pitch, device)
    rejected(stage(top, low, _mat(base + 20 * pitch + 1, 16, 40, pitch, device)), "warped_mask", "out")      # shifted by one byte
    rejected(stage(top, low, _mat(base + 21 * pitch, 16, 40, pitch, device)), "warped_mask", "out")          # shifted by one row
    rejected(stage(top, _mat(base + 20 * pitch, 8, 20, 2 * pitch, device), _mat(base + 20 * pitch, 8, 20, pitch, device)), "warped_mask", "out")      # another pitch
    # mats in different memories share nothing, whatever their addresses say
    other = np.zeros((10, 20), np.uint8) if where == "device" else _dev(np.zeros((10, 20), np.uint8))
    assert resize(_mat(base, 10, 20, pitch, device), _lib.as_mat(other)) == 0
    # disjoint views of one buffer: rows 0..9 -> rows 20..35, and the mask stage in place on those rows (out is warped_mask, as the same view)
    assert resize(_mat(base, 10, 20, pitch, device), low) == 0
    want = host.copy()
    want[20:36, :40] = R.resize(host[:10, :20], (40, 16))
    import torch
    torch.cuda.synchronize()
    assert np.array_equal(_np(buf), want)
    assert stage(top, low, _mat(base + 20 * pitch, 16, 40, pitch, device)) == 0
    torch.cuda.synchronize()
    want[20:36, :40] = R.dilate_resize_and(host[:10], want[20:36, :40].copy(), 3, 3)
    assert np.array_equal(_np(buf), want)


def test_overlap_error_leaves_a_capture_usable(gpu):
    """the check comes before anything touches the stream: a rejected call inside a capture enqueues nothing and the capture goes on"""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        img = torch.zeros((40, 64), dtype=torch.uint8, device="cuda")
        small = torch.zeros((10, 16), dtype=torch.uint8, device="cuda")
        out = torch.zeros((40, 64), dtype=torch.uint8, device="cuda")
        x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            gpu.resize(img, (16, 10), dst=img[4:14, 8:24], stream=s)
        assert e.value.code == ERR_INVALID and "src" in e.value.msg and "dst" in e.value.msg, e.value.msg
        with pytest.raises(gpu.IsxError) as e:
            gpu.dilate_resize_and(img, (64, 40), 3, 3, out=img, stream=s)
        assert e.value.code == ERR_INVALID and "seam_mask" in e.value.msg, e.value.msg
        with pytest.raises(gpu.IsxError) as e:
            gpu.dilate_resize_and(small, out[:, 1:], 3, 3, out=out[:, :63], stream=s)
        assert e.value.code == ERR_INVALID and "warped_mask" in e.value.msg, e.value.msg
        gpu.resize(img, (16, 10), dst=small, stream=s)
        gpu.dilate_resize_and(small, out, 3, 3, out=out, stream=s)
    a = _src(np.uint8, 1, (40, 64), 77)
    w = _warped_mask((40, 64), 78)
    with torch.cuda.stream(s):
        img.copy_(_dev(a)); out.copy_(_dev(w))
    s.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    sm = R.resize(a, (16, 10))
    assert np.array_equal(_np(small), sm) and np.array_equal(_np(out), R.dilate_resize_and(sm, w, 3, 3)) and np.array_equal(_np(img), a)
