"""A NumPy model of BlocksGainCompensator (OpenCV 3.4.2, modules/stitching/src/exposure_compensate.cpp) and of the cv::resize(INTER_LINEAR) on
CV_32F its apply() goes through (modules/imgproc/src/resize.cpp), one rounded operation at a time: float32 where OpenCV computes in float,
float64 where it computes in double.  The spec of isx_blocks_gain_feed / isx_blocks_gain_apply; neither OpenCV source is in the reference
tree, so parity with OpenCV itself is unpinned.  Built on feed_model of tests/test_gain_model.py (GainCompensator::feed on the blocks as if
each were an image).

    feed:   nx = ceil(cols / bl_width), bw = ceil(cols / nx); block (bx, by) = [bx bw, min(bx bw + bw, cols)) x the same in y, its corner the
            image's plus (bx bw, by bh); blocks numbered image by image, by outer, bx inner; gains = GainCompensator::feed over all blocks;
            gain_map(by, bx) = (float)gain, then sepFilter2D with [0.25, 0.5, 0.25] (BORDER_REFLECT_101) twice.
    apply:  g = the map itself when it has the image's size, else resize(map, image.size(), 0, 0, INTER_LINEAR);
            out = saturate_cast<uchar>(cvRound((float)p * g)) for every channel byte."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_gain_model import ALPHA, BETA, feed_model  # noqa: E402

F32 = np.float32


# ---- the block grid ----------------------------------------------------------------------------------------------------------------------

def block_grid(cols, rows, bl_width=32, bl_height=32):
    """(nx, ny, bw, bh) of an image of cols x rows."""
    nx, ny = (cols + bl_width - 1) // bl_width, (rows + bl_height - 1) // bl_height
    return nx, ny, (cols + nx - 1) // nx, (rows + ny - 1) // ny


def block_rects(cols, rows, bl_width=32, bl_height=32):
    """[(x, y, w, h)] of every block inside its image, by outer, bx inner."""
    nx, ny, bw, bh = block_grid(cols, rows, bl_width, bl_height)
    return [(bx * bw, by * bh, min(bx * bw + bw, cols) - bx * bw, min(by * bh + bh, rows) - by * bh) for by in range(ny) for bx in range(nx)]


def split_blocks(corners, images, masks, bl_width=32, bl_height=32):
    """(block corners, block images, block masks, image of each block, [(nx, ny)] per image)."""
    bc, bi, bm, owner, counts = [], [], [], [], []
    for k, (c, img, m) in enumerate(zip(corners, images, masks)):
        rows, cols = img.shape[:2]
        counts.append(block_grid(cols, rows, bl_width, bl_height)[:2])
        for x, y, w, h in block_rects(cols, rows, bl_width, bl_height):
            bc.append((c[0] + x, c[1] + y)); bi.append(img[y:y + h, x:x + w]); bm.append(m[y:y + h, x:x + w]); owner.append(k)
    return bc, bi, bm, owner, counts


# ---- feed --------------------------------------------------------------------------------------------------------------------------------

def smooth(m):
    """sepFilter2D(m, m, CV_32F, ker, ker), ker = [0.25, 0.5, 0.25], BORDER_REFLECT_101, twice; float32: x[0] * 0.5 + (x[-1] + x[1]) * 0.25."""
    m = np.asarray(m, F32)

    def idx(n):
        i = np.arange(n)
        if n == 1:
            return i * 0, i * 0
        lo, hi = i - 1, i + 1
        lo[0], hi[-1] = 1, n - 2
        return lo, hi
    for _ in range(2):
        lo, hi = idx(m.shape[1])
        side = (m[:, lo] + m[:, hi]).astype(F32)
        m = ((m * F32(0.5)).astype(F32) + (side * F32(0.25)).astype(F32)).astype(F32)
        lo, hi = idx(m.shape[0])
        side = (m[lo] + m[hi]).astype(F32)
        m = ((m * F32(0.5)).astype(F32) + (side * F32(0.25)).astype(F32)).astype(F32)
    return m


def maps_from_gains(gains, counts):
    """gain_map(by, bx) = (float)gains[block], smoothed: one ny x nx float32 map per image."""
    out, k = [], 0
    for nx, ny in counts:
        out.append(smooth(np.asarray(gains[k:k + nx * ny], np.float64).astype(F32).reshape(ny, nx)))
        k += nx * ny
    return out


def feed_blocks_model(corners, images, masks, bl_width=32, bl_height=32):
    """dict: counts [(nx, ny)], owner (image of each block), N, I, A, b (dense, over all blocks), gains (np.linalg.solve), maps, and the
    sparse statistics the library reports - pairs [(block_i, block_j, N, I_ij, I_ji)] for i < j of different images with N > 0, diag_n."""
    bc, bi, bm, owner, counts = split_blocks(corners, images, masks, bl_width, bl_height)
    N, I, _, A, b, gains = feed_model(bc, bi, bm)
    B = len(bc)
    for i in range(B):
        for j in range(B):
            assert i == j or owner[i] != owner[j] or N[i, j] == 0          # blocks of one image never overlap
    pairs = [(i, j, int(N[i, j]), float(I[i, j]), float(I[j, i])) for i in range(B) for j in range(i + 1, B) if N[i, j] > 0]
    return dict(counts=counts, owner=owner, N=N, I=I, A=A, b=b, gains=gains, maps=maps_from_gains(gains, counts), pairs=pairs,
                diag_n=np.diag(N).copy())


def sparse_system(pairs, diag_n):
    """(rows, cols, values, b) of OpenCV's system from the sparse statistics, row i's terms added in OpenCV's order (j ascending)."""
    B = len(diag_n)
    adj = [[(i, float(diag_n[i]), 0.0, 0.0)] for i in range(B)]
    for i, j, n, iij, iji in pairs:
        adj[int(i)].append((int(j), float(n), float(iij), float(iji)))
        adj[int(j)].append((int(i), float(n), float(iji), float(iij)))
    rows, cols, vals, b = [], [], [], np.zeros(B)
    for i in range(B):
        d = 0.0
        for j, n, iij, iji in sorted(adj[i]):
            b[i] += BETA * n
            d += BETA * n
            if j == i:
                continue
            d += 2 * ALPHA * iij * iij * n
            rows.append(i); cols.append(j); vals.append(0.0 - 2 * ALPHA * iij * iji * n)
        rows.append(i); cols.append(i); vals.append(d)
    return np.array(rows), np.array(cols), np.array(vals), b


# ---- hal::LU -----------------------------------------------------------------------------------------------------------------------------

def hal_lu_solve(A, b):
    """OpenCV's hal::LU and its back substitution in float64: (x, row swaps), or (None, swaps) for a pivot below 100 DBL_EPSILON.
    The pivot is the first row of largest |value| (strict >); d = -1 / pivot; A[j][c] += (A[j][i] d) A[i][c], b[j] += (A[j][i] d) b[i]."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = b.size
    swaps = 0
    for i in range(n):
        k = i + int(np.argmax(np.abs(A[i:, i])))          # argmax: the first of the largest
        if abs(A[k, i]) < 100 * np.finfo(np.float64).eps:
            return None, swaps
        if k != i:
            A[[i, k], i:] = A[[k, i], i:]
            b[[i, k]] = b[[k, i]]
            swaps += 1
        d = -1.0 / A[i, i]
        alpha = A[i + 1:, i] * d
        A[i + 1:, i + 1:] += alpha[:, None] * A[i, i + 1:][None, :]      # a rounded product, then a rounded sum: no FMA in NumPy
        b[i + 1:] += alpha * b[i]
    for i in range(n - 1, -1, -1):
        s = b[i]
        for c in range(i + 1, n):
            s -= A[i, c] * b[c]
        b[i] = s / A[i, i]
    return b, swaps


# ---- apply -------------------------------------------------------------------------------------------------------------------------------

def resize_taps(src, dst):
    """(s0, s1, f) of cv::resize's linear coefficients along one axis BEFORE either axis' edge rule: f float32, s0 = floor."""
    scale = 1.0 / (float(dst) / src)
    f = ((np.arange(dst) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(F32)).astype(F32)


def resize_linear(m, w, h):
    """cv::resize(m, Size(w, h), 0, 0, INTER_LINEAR) on CV_32F.  Columns: sx < 0 -> (0, fx = 0), sx >= src_w - 1 -> (src_w - 1, fx = 0),
    h = S[sx] (1 - fx) + S[sx + 1] fx, and S[sx] where no tap lies to the right.  Rows: fy is kept, sy and sy + 1 are each clamped:
    g = h_sy (1 - fy) + h_{sy+1} fy."""
    m = np.asarray(m, F32)
    sh, sw = m.shape
    sx, fx = resize_taps(sw, w)
    fx = np.where((sx < 0) | (sx >= sw - 1), F32(0), fx).astype(F32)
    sx = np.clip(sx, 0, sw - 1)
    right = np.minimum(sx + 1, sw - 1)
    two = ((m[:, sx] * (F32(1) - fx)[None, :]).astype(F32) + (m[:, right] * fx[None, :]).astype(F32)).astype(F32)
    hrow = np.where((sx + 1 < sw)[None, :], two, m[:, sx]).astype(F32)
    sy, fy = resize_taps(sh, h)
    sy0, sy1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    return ((hrow[sy0] * (F32(1) - fy)[:, None]).astype(F32) + (hrow[sy1] * fy[:, None]).astype(F32)).astype(F32)


def gain_image(m, w, h):
    """The per-pixel gains apply() multiplies by: the map itself when it has the image's size, else the resized map."""
    m = np.asarray(m, F32)
    return m if m.shape == (h, w) else resize_linear(m, w, h)


def apply_model(img, m):
    """saturate_cast<uchar>(cvRound((float)p * g)) per channel byte: the product in float32, ties to even (cvtss2si: NaN or |v| >= 2^31
    gives INT_MIN), clamped to [0, 255]."""
    h, w = img.shape[:2]
    g = gain_image(m, w, h)
    prod = (img.astype(F32) * g[:, :, None]).astype(F32)
    with np.errstate(invalid="ignore"):
        r = np.rint(prod.astype(np.float64))
        r = np.where(np.isfinite(r) & (np.abs(r) < 2.0 ** 31), r, -2.0 ** 31)
    return np.clip(r, 0, 255).astype(np.uint8)
