"""NumPy model of cv::resize(src, dst, dsize, 0, 0, INTER_NEAREST | INTER_LINEAR) on CV_8U / CV_32F and of the compose loop's mask stage
resize(dilate(seam, MORPH_RECT kw x kh), size, INTER_LINEAR) & warped (isx_resize, isx_mask_dilate_resize_and): the standard of record.
Restated from OpenCV 3.4.2 imgproc/src/resize.cpp, plain C++ path; parity with OpenCV itself is unpinned.  Integers in int64, floats one
rounded float32 operation at a time, the scales in double - nothing is normalised or simplified (a0 + a1 is not always 2048).

    inv_x = (double)dst_w / src_w, scale_x = 1.0 / inv_x                                       (the same in y)
    NEAREST   sx = min(floor(dx * scale_x), src_w - 1)
    LINEAR    src_w == 2 dst_w and src_h == 2 dst_h (BOTH): the 2 x 2 area rule; else
              fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> (0, 0); sx >= src_w - 1 -> (src_w - 1, 0)
              fy alike but KEPT, the row indices sy, sy + 1 each clamped to [0, src_h - 1]
"""
import numpy as np

NEAREST, LINEAR = 0, 1
f32 = np.float32


def scale_of(src_n, dst_n):
    return 1.0 / (float(dst_n) / float(src_n))


def col_taps(src_w, dst_w):
    """(sx int64[dst_w], fx float32[dst_w])"""
    d = np.arange(dst_w, dtype=np.float64)
    fx = ((d + 0.5) * scale_of(src_w, dst_w) - 0.5).astype(f32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(f32)).astype(f32)
    lo = sx < 0
    sx = np.where(lo, 0, sx)
    fx = np.where(lo, f32(0), fx)
    hi = sx >= src_w - 1
    sx = np.where(hi, src_w - 1, sx)
    fx = np.where(hi, f32(0), fx).astype(f32)
    return sx, fx


def row_taps(src_h, dst_h):
    """(sy0, sy1 int64[dst_h], fy float32[dst_h]): fy is kept where an index is clamped"""
    d = np.arange(dst_h, dtype=np.float64)
    fy = ((d + 0.5) * scale_of(src_h, dst_h) - 0.5).astype(f32)
    sy = np.floor(fy).astype(np.int64)
    fy = (fy - sy.astype(f32)).astype(f32)
    return np.clip(sy, 0, src_h - 1), np.clip(sy + 1, 0, src_h - 1), fy


def nearest_taps(src_n, dst_n):
    return np.minimum(np.floor(np.arange(dst_n, dtype=np.float64) * scale_of(src_n, dst_n)).astype(np.int64), src_n - 1)


def coef(f):
    """saturate_cast<short>(cvRound(f * 2048)): ties to even (np.rint)"""
    return np.clip(np.rint((np.asarray(f, f32) * f32(2048)).astype(f32)).astype(np.int64), -32768, 32767)


def is_half(src_hw, dst_hw):
    return src_hw[0] == 2 * dst_hw[0] and src_hw[1] == 2 * dst_hw[1]


def resize(src, dsize, interpolation=LINEAR):
    """src: (h, w) or (h, w, c) uint8 / float32; dsize = (width, height)."""
    src = np.asarray(src)
    assert src.dtype in (np.uint8, np.float32) and interpolation in (NEAREST, LINEAR)
    dw, dh = int(dsize[0]), int(dsize[1])
    sh, sw = src.shape[:2]
    assert dw > 0 and dh > 0 and sw > 0 and sh > 0
    s = src.reshape(sh, sw, -1)
    if interpolation == NEAREST:
        out = s[nearest_taps(sh, dh)][:, nearest_taps(sw, dw)]
    elif is_half((sh, sw), (dh, dw)):
        a, b, c, d = s[0::2, 0::2], s[0::2, 1::2], s[1::2, 0::2], s[1::2, 1::2]
        if src.dtype == np.uint8:
            out = ((a.astype(np.int64) + b + c + d + 2) >> 2).astype(np.uint8)
        else:
            out = ((((a + b).astype(f32) + c).astype(f32) + d).astype(f32) * f32(0.25)).astype(f32)
    else:
        sx, fx = col_taps(sw, dw)
        sy0, sy1, fy = row_taps(sh, dh)
        two = (sx + 1 < sw)[None, :, None]
        sx1 = np.minimum(sx + 1, sw - 1)
        if src.dtype == np.uint8:
            a0, a1 = coef((f32(1) - fx).astype(f32))[None, :, None], coef(fx)[None, :, None]
            b0, b1 = coef((f32(1) - fy).astype(f32))[:, None, None], coef(fy)[:, None, None]
            si = s.astype(np.int64)
            H = si[:, sx] * a0 + np.where(two, si[:, sx1] * a1, 0)                  # every source row's horizontal sums
            v = (((b0 * (H[sy0] >> 4)) >> 16) + ((b1 * (H[sy1] >> 4)) >> 16) + 2) >> 2
            out = np.clip(v, 0, 255).astype(np.uint8)
        else:
            with np.errstate(all="ignore"):
                fxb, fyb = fx[None, :, None], fy[:, None, None]
                a0 = (f32(1) - fxb).astype(f32)
                full = ((s[:, sx] * a0).astype(f32) + (s[:, sx1] * fxb).astype(f32)).astype(f32)
                H = np.where(two, full, s[:, sx]).astype(f32)
                b0 = (f32(1) - fyb).astype(f32)
                out = ((H[sy0] * b0).astype(f32) + (H[sy1] * fyb).astype(f32)).astype(f32)
    return np.ascontiguousarray(out.reshape((dh, dw) + src.shape[2:]))


def dilate(mask, kw, kh):
    """dilate(mask, MORPH_RECT kw x kh), anchor (kw / 2, kh / 2); pixels outside the image take no part"""
    m = np.asarray(mask, np.uint8)
    h, w = m.shape
    ax, ay = kw // 2, kh // 2
    rows = np.zeros_like(m)
    for x in range(w):
        rows[:, x] = m[:, max(x - ax, 0):min(x - ax + kw, w)].max(axis=1)
    out = np.zeros_like(m)
    for y in range(h):
        out[y] = rows[max(y - ay, 0):min(y - ay + kh, h)].max(axis=0)
    return out


def dilate_resize_and(seam, warped, kw, kh, out_size=None):
    """resize(dilate(seam, kw x kh), out_size, LINEAR) & warped; out_size = (width, height), warped's when None; warped may be None"""
    if out_size is None:
        out_size = (warped.shape[1], warped.shape[0])
    r = resize(dilate(seam, kw, kh), out_size, LINEAR)
    return r if warped is None else r & np.asarray(warped, np.uint8)
