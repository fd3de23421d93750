"""The specification of isx_find_homography (DESIGN.md §8 "Homography"): BestOf2NearestMatcher::match from R:836 to R:909 (R = the
reference's 计算单应性矩阵 demo, a hand-unrolled OpenCV 3.4.2 findHomography(RANSAC)) without the Levenberg-Marquardt polish, in NumPy.

float64 arithmetic is IEEE + - * / sqrt only, evaluated in the order written (no fused multiply-add), so a device compiled with
-ffp-contract=off can agree bit for bit; the float32 arithmetic of computeError runs on float32 arrays.  The one exception is pow / log
in the iteration-count update (R:51-56): `margin` reports how far every such update stayed from a rounding boundary.

cv::eigen (JacobiImpl_), cv::RNG, haveCollinearPoints and cvRound are in neither tree; they are restated here from OpenCV's published
behaviour, so parity with OpenCV is unpinned and this file is what the GPU is held to.  The hypotheses of a RANSAC run are solved in
batches (the sample stream depends on the points alone, never on the scores), then scanned in order as the sequential loop does."""
import math

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
MAX_ATTEMPTS = 10000
ST_H, ST_PASS2, ST_PASS2_FAILED, ST_CLAMPED, ST_DEGENERATE = 1, 2, 4, 8, 16
_BATCHES = (2, 6, 16, 104, 256)    # hypotheses solved ahead per batch: small first, most runs stop within a few iterations


class RNG:
    """cv::RNG: a multiply-with-carry generator."""

    def __init__(self, state=(1 << 64) - 1):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4294883355 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a + self.next() % (b - a)


def det3(a):
    """The determinant by cofactors along the first row; a: 9 floats, row-major."""
    return (a[0] * (a[4] * a[8] - a[7] * a[5]) - a[1] * (a[3] * a[8] - a[6] * a[5])) + a[2] * (a[3] * a[7] - a[6] * a[4])


def have_collinear_points(pts, count):
    """Tests the last point only, as OpenCV's haveCollinearPoints does; pts: count x 2 float32."""
    i = count - 1
    xi, yi = float(pts[i][0]), float(pts[i][1])
    for j in range(i):
        dx1, dy1 = float(pts[j][0]) - xi, float(pts[j][1]) - yi
        for k in range(j):
            dx2, dy2 = float(pts[k][0]) - xi, float(pts[k][1]) - yi
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


_TT = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))


def check_subset(ms1, ms2):
    """R:253-288 for count = 4."""
    if have_collinear_points(ms1, 4) or have_collinear_points(ms2, 4):
        return False
    negative = 0
    for t in _TT:
        a = [v for q in t for v in (float(ms1[q][0]), float(ms1[q][1]), 1.0)]
        b = [v for q in t for v in (float(ms2[q][0]), float(ms2[q][1]), 1.0)]
        negative += det3(a) * det3(b) < 0
    return negative == 0 or negative == 4


def get_subset(src, dst, rng):
    """R:111-136 with 10000 attempts: (found, the four rows, attempts made)."""
    count = len(src)
    for attempt in range(MAX_ATTEMPTS):
        idx = []
        while len(idx) < 4:
            v = rng.uniform(0, count)
            if v not in idx:
                idx.append(v)
        if check_subset(src[idx], dst[idx]):
            return True, idx, attempt + 1
    return False, None, MAX_ATTEMPTS


def _hypot(a, b):
    """OpenCV's own hypot, elementwise."""
    a, b = np.abs(a), np.abs(b)
    with np.errstate(all="ignore"):
        big = a * np.sqrt(1.0 + (b / a) * (b / a))
        small = np.where(b > 0, b * np.sqrt(1.0 + (a / b) * (a / b)), 0.0)
    return np.where(a > b, big, small)


def _hypot1(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b /= a
        return a * math.sqrt(1.0 + b * b)
    if b > 0:
        a /= b
        return b * math.sqrt(1.0 + a * a)
    return 0.0


def jacobi_scalar(A):
    """JacobiImpl_ as OpenCV writes it, for one 9 x 9 matrix in Python floats: what jacobi() computes for a batch, line by line (the two
    are tested to agree bit for bit).  Returns (W, V, rotations) as lists / nested lists."""
    n = 9
    A = [float(v) for v in np.asarray(A, np.float64).reshape(n * n)]
    V = [0.0] * (n * n)
    for i in range(n):
        V[i * n + i] = 1.0
    W = [A[(n + 1) * k] for k in range(n)]
    indR, indC = [0] * n, [0] * n

    def scan_r(k):
        m, mv = k + 1, abs(A[n * k + k + 1])
        for i in range(k + 2, n):
            val = abs(A[n * k + i])
            if mv < val:
                mv, m = val, i
        return m

    def scan_c(k):
        m, mv = 0, abs(A[k])
        for i in range(1, k):
            val = abs(A[n * i + k])
            if mv < val:
                mv, m = val, i
        return m

    for k in range(n):
        if k < n - 1:
            indR[k] = scan_r(k)
        if k > 0:
            indC[k] = scan_c(k)
    rot = 0
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[indR[0]])
        for i in range(1, n - 1):
            val = abs(A[n * i + indR[i]])
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[n * indC[i] + i])
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[n * k + l]
        if abs(p) <= DBL_EPSILON:
            break
        rot += 1
        y = (W[l] - W[k]) * 0.5
        t = abs(y) + _hypot1(p, y)
        s = _hypot1(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[n * k + l] = 0.0
        W[k] -= t
        W[l] += t

        for i in range(k):                    # rotate rows and columns k and l: v0 = a0 c - b0 s, v1 = a0 s + b0 c
            i0, i1 = n * i + k, n * i + l
            a0, b0 = A[i0], A[i1]
            A[i0], A[i1] = a0 * c - b0 * s, a0 * s + b0 * c
        for i in range(k + 1, l):
            i0, i1 = n * k + i, n * i + l
            a0, b0 = A[i0], A[i1]
            A[i0], A[i1] = a0 * c - b0 * s, a0 * s + b0 * c
        for i in range(l + 1, n):
            i0, i1 = n * k + i, n * l + i
            a0, b0 = A[i0], A[i1]
            A[i0], A[i1] = a0 * c - b0 * s, a0 * s + b0 * c
        for i in range(n):
            i0, i1 = n * k + i, n * l + i
            a0, b0 = V[i0], V[i1]
            V[i0], V[i1] = a0 * c - b0 * s, a0 * s + b0 * c
        for idx in (k, l):
            if idx < n - 1:
                indR[idx] = scan_r(idx)
            if idx > 0:
                indC[idx] = scan_c(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            for i in range(n):
                V[n * m + i], V[n * k + i] = V[n * k + i], V[n * m + i]
    return W, [V[n * i:n * i + n] for i in range(n)], rot


SCALAR_BATCH = 16               # up to this many matrices jacobi() solves one by one: cheaper than the masked batch


def jacobi(A, batched=False):
    """OpenCV's JacobiImpl_ for a batch of symmetric 9 x 9 matrices (only the upper triangles are read): cyclic by largest pivot with
    the indR / indC tables, at most 9 * 9 * 30 rotations, stopping at |p| <= DBL_EPSILON; eigenvalues selection-sorted descending with the
    rows of V.  A: (B, 9, 9) float64.  Returns (W (B, 9), V (B, 9, 9), rotations (B,))."""
    n = 9
    A = np.array(A, np.float64).reshape(-1, n * n)
    B = A.shape[0]
    if B <= SCALAR_BATCH and not batched:
        res = [jacobi_scalar(a) for a in A]
        return (np.array([r[0] for r in res]).reshape(B, n), np.array([r[1] for r in res]).reshape(B, n, n),
                np.array([r[2] for r in res], np.int64))
    V = np.tile(np.eye(n).reshape(1, n * n), (B, 1))
    W = A[:, ::n + 1].copy()
    indR, indC = np.zeros((B, n), np.int64), np.zeros((B, n), np.int64)
    rot = np.zeros(B, np.int64)

    ar = np.arange(n)[None, :]

    def upd_r(A, r, idx):          # the row scan: the largest |A[idx][i]|, i > idx (the first of equals: argmax)
        vals = np.where(ar > idx[:, None], np.abs(A[r[:, None], n * idx[:, None] + ar]), -1.0)
        return np.argmax(vals, 1)

    def upd_c(A, r, idx):          # the column scan: the largest |A[i][idx]|, i < idx
        vals = np.where(ar < idx[:, None], np.abs(A[r[:, None], n * ar + idx[:, None]]), -1.0)
        return np.argmax(vals, 1)

    r = np.arange(B)
    for k in range(n):
        kk = np.full(B, k)
        if k < n - 1:
            indR[:, k] = upd_r(A, r, kk)
        if k > 0:
            indC[:, k] = upd_c(A, r, kk)
    act = np.arange(B)
    rows, colsc = np.arange(n - 1)[None, :], np.arange(1, n)[None, :]
    for _ in range(n * n * 30):
        if act.size == 0:
            break
        a, iR, iC = A[act], indR[act], indC[act]
        r = np.arange(act.size)
        # the pivot: rows 0..7 through indR, then columns 1..8 through indC, the first of equals
        cand = np.abs(np.concatenate([a[r[:, None], n * rows + iR[:, :n - 1]], a[r[:, None], n * iC[:, 1:] + colsc]], 1))
        j = np.argmax(cand, 1)
        isr = j < n - 1
        jr, jc = np.minimum(j, n - 2), np.maximum(j - (n - 1) + 1, 1)
        k = np.where(isr, jr, iC[r, jc])
        l = np.where(isr, iR[r, jr], jc)
        p = a[r, n * k + l]
        go = ~(np.abs(p) <= DBL_EPSILON)
        act = act[go]
        if act.size == 0:
            break
        a, iR, iC, k, l, p = a[go], iR[go], iC[go], k[go], l[go], p[go]
        w, v = W[act], V[act]
        r = np.arange(act.size)
        rot[act] += 1
        y = (w[r, l] - w[r, k]) * 0.5
        t = np.abs(y) + _hypot(p, y)
        s = _hypot(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        neg = y < 0
        s, t = np.where(neg, -s, s), np.where(neg, -t, t)
        a[r, n * k + l] = 0.0
        w[r, k] -= t
        w[r, l] += t
        k2, l2, c2, s2, r2 = k[:, None], l[:, None], c[:, None], s[:, None], r[:, None]
        lo, hi = ar < k2, ar > l2
        valid = (ar != k2) & (ar != l2)
        i0 = np.where(lo, n * ar + k2, n * k2 + ar)          # i < k: A[i][k], A[i][l]; k < i < l: A[k][i], A[i][l]; l < i: A[k][i], A[l][i]
        i1 = np.where(hi, n * l2 + ar, n * ar + l2)
        a0, b0 = a[r2, i0], a[r2, i1]
        n0, n1 = a0 * c2 - b0 * s2, a0 * s2 + b0 * c2
        rv = np.broadcast_to(r2, valid.shape)[valid]
        a[rv, i0[valid]] = n0[valid]
        a[rv, i1[valid]] = n1[valid]
        ik, il = n * k2 + ar, n * l2 + ar
        a0, b0 = v[r2, ik], v[r2, il]
        v[r2, ik] = a0 * c2 - b0 * s2
        v[r2, il] = a0 * s2 + b0 * c2
        for idx in (k, l):
            m = upd_r(a, r, idx)
            sel = idx < n - 1
            iR[r[sel], idx[sel]] = m[sel]
            m = upd_c(a, r, idx)
            sel = idx > 0
            iC[r[sel], idx[sel]] = m[sel]
        A[act], W[act], V[act], indR[act], indC[act] = a, w, v, iR, iC
    V = V.reshape(B, n, n)
    r = np.arange(B)
    for k in range(n - 1):
        m = np.full(B, k)
        for i in range(k + 1, n):
            m = np.where(W[r, m] < W[r, i], i, m)
        wk, wm = W[r, k].copy(), W[r, m].copy()
        W[r, k], W[r, m] = wm, wk
        vk, vm = V[r, k].copy(), V[r, m].copy()
        V[r, k], V[r, m] = vm, vk
    return W, V, rot


def build_ltl(M, m):
    """R:319-362 for a batch: M (src), m (dst): (B, count, 2) float32.  Returns (ok (B,), LtL (B, 9, 9), invHnorm (B, 9), Hnorm2 (B, 9))."""
    M, m = np.asarray(M, np.float32).astype(np.float64), np.asarray(m, np.float32).astype(np.float64)
    B, count = M.shape[0], M.shape[1]
    z = np.zeros(B)
    cmx, cmy, cMx, cMy = z.copy(), z.copy(), z.copy(), z.copy()
    for i in range(count):
        cmx = cmx + m[:, i, 0]; cmy = cmy + m[:, i, 1]
        cMx = cMx + M[:, i, 0]; cMy = cMy + M[:, i, 1]
    cmx, cmy, cMx, cMy = cmx / count, cmy / count, cMx / count, cMy / count
    smx, smy, sMx, sMy = z.copy(), z.copy(), z.copy(), z.copy()
    for i in range(count):
        smx = smx + np.abs(m[:, i, 0] - cmx); smy = smy + np.abs(m[:, i, 1] - cmy)
        sMx = sMx + np.abs(M[:, i, 0] - cMx); sMy = sMy + np.abs(M[:, i, 1] - cMy)
    ok = ~((np.abs(smx) < DBL_EPSILON) | (np.abs(smy) < DBL_EPSILON) | (np.abs(sMx) < DBL_EPSILON) | (np.abs(sMy) < DBL_EPSILON))
    with np.errstate(all="ignore"):
        smx, smy, sMx, sMy = count / smx, count / smy, count / sMx, count / sMy
        one = np.ones(B)
        inv = np.stack([1.0 / smx, z, cmx, z, 1.0 / smy, cmy, z, z, one], 1)
        hn2 = np.stack([sMx, z, -cMx * sMx, z, sMy, -cMy * sMy, z, z, one], 1)
        LtL = np.zeros((B, 9, 9))
        for i in range(count):
            x, y = (m[:, i, 0] - cmx) * smx, (m[:, i, 1] - cmy) * smy
            X, Y = (M[:, i, 0] - cMx) * sMx, (M[:, i, 1] - cMy) * sMy
            Lx = np.stack([X, Y, one, z, z, z, -x * X, -x * Y, -x], 1)
            Ly = np.stack([z, z, z, X, Y, one, -y * X, -y * Y, -y], 1)
            LtL = LtL + (Lx[:, :, None] * Lx[:, None, :] + Ly[:, :, None] * Ly[:, None, :])
    return ok, LtL, inv, hn2


def _mul3(a, b):
    """3 x 3 products for a batch, each sum k = 0, 1, 2 left to right."""
    out = np.empty_like(a)
    for i in range(3):
        for j in range(3):
            out[:, 3 * i + j] = (a[:, 3 * i] * b[:, j] + a[:, 3 * i + 1] * b[:, 3 + j]) + a[:, 3 * i + 2] * b[:, 6 + j]
    return out


def run_kernel(M, m):
    """R:304-373 for a batch of point sets of one size: (ok (B,), H (B, 9) float64; rows with ok False are undefined)."""
    ok, LtL, inv, hn2 = build_ltl(M, m)
    H = np.zeros((LtL.shape[0], 9))
    if ok.any():
        _, V, _ = jacobi(LtL[ok])
        with np.errstate(all="ignore"):
            h0 = _mul3(_mul3(inv[ok], V[:, 8, :]), hn2[ok])
            H[ok] = h0 * (1.0 / h0[:, 8])[:, None]
    return ok, H


def compute_error(src, dst, H):
    """R:383-402 in float32: src, dst (n, 2) float32, H 9 float64."""
    with np.errstate(all="ignore"):
        Hf = np.asarray(H, np.float64).astype(np.float32)
        Mx, My, mx, my = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
        one = np.float32(1)
        ww = one / ((Hf[6] * Mx + Hf[7] * My) + one)
        dx = ((Hf[0] * Mx + Hf[1] * My) + Hf[2]) * ww - mx
        dy = ((Hf[3] * Mx + Hf[4] * My) + Hf[5]) * ww - my
        return dx * dx + dy * dy


def find_inliers(src, dst, H, thresh):
    """R:67-86: (the count, the mask)."""
    with np.errstate(invalid="ignore"):
        mask = (compute_error(src, dst, H) <= np.float32(thresh * thresh)).astype(np.uint8)
    return int(mask.sum()), mask


def _cv_round(v):
    return int(round(v))       # Python rounds half to even


def update_num_iters(p, ep, model_points, max_iters, margins=None):
    """R:39-59.  Appends to `margins` the relative distance of num / denom from the nearest half-integer and from max_iters."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    if denom >= 0:
        return max_iters
    q = num / denom
    if margins is not None:
        d = abs(q - max_iters)
        if q < max_iters:                   # only then is q rounded
            d = min(d, abs(q - (math.floor(q) + 0.5)))
        margins.append(d / max(abs(q), 1.0))
    return max_iters if -num >= max_iters * (-denom) else _cv_round(q)


class _Run:
    def __init__(self):
        self.ok, self.H, self.mask, self.iters, self.win, self.attempts = False, None, None, 0, -1, 0


def ransac(src, dst, thresh, max_iters, confidence, margins):
    """RANSACPointSetRegistrator1::run (R:139-233, with `nmodels = cb->runKernel(ms1, ms2, model)` restored between R:196 and R:197) for
    count > 4."""
    out = _Run()
    count = len(src)
    rng = RNG()
    niters = max(max_iters, 1)
    max_good = 0
    hyp = []                      # per iteration drawn so far: (found, attempts, H or None)
    it = 0
    stage = 0
    exhausted = False
    while it < niters:
        if it >= len(hyp):
            assert not exhausted
            want = min(_BATCHES[min(stage, len(_BATCHES) - 1)], niters - len(hyp))
            stage += 1
            sets, first = [], len(hyp)
            for _ in range(want):
                found, idx, att = get_subset(src, dst, rng)
                hyp.append([found, att, None])
                if not found:
                    exhausted = True
                    break
                sets.append(idx)
            if sets:
                sets = np.asarray(sets)
                ok, H = run_kernel(src[sets], dst[sets])
                for b in range(len(sets)):
                    if ok[b]:
                        hyp[first + b][2] = H[b]
        found, att, H = hyp[it]
        out.attempts += att
        if not found:
            if it == 0:
                out.iters = 0
                return out
            break
        if H is not None:
            good, mask = find_inliers(src, dst, H, thresh)
            if good > max(max_good, 3):
                out.mask, out.H, max_good, out.win = mask, H.copy(), good, it
                niters = update_num_iters(confidence, float(count - good) / count, 4, niters, margins)
        it += 1
    out.iters = it
    out.ok = max_good > 0
    return out


def find_homography2(src, dst, thresh, max_iters, confidence, margins):
    """findHomography2 (R:602-693) with RANSAC, without the LM polish of R:672.  Returns a _Run: ok False means an empty H; the mask is
    always count rows (zeros on failure, R:687)."""
    n = len(src)
    if thresh <= 0:
        thresh = 3.0
    if n == 4:
        out = _Run()
        ok, H = run_kernel(src[None], dst[None])
        out.ok = bool(ok[0])
        out.H = H[0] if out.ok else None
        out.mask = np.ones(4, np.uint8)
    elif n < 4:
        out = _Run()
    else:
        out = ransac(src, dst, thresh, max_iters, confidence, margins)
    if out.ok and n > 4:
        sel = out.mask.astype(bool)
        if sel.any():
            ok, H = run_kernel(src[sel][None], dst[sel][None])
            if ok[0]:
                out.H = H[0]
    if not out.ok:
        out.H = None
        out.mask = np.zeros(n, np.uint8)
    return out


def find_homography_np(points, count=None, reproj_thresh=3.0, max_iters=2000, confidence=0.995, num_matches_thresh1=6, num_matches_thresh2=6,
                       mask_rows=None):
    """One pair of isx_find_homography.  points: rows x 4 float32 (src.x, src.y, dst.x, dst.y); count: the matcher's count (default: all
    rows), clamped to the rows of points and to mask_rows.  Returns a dict: H (3 x 3 float64, zeros when empty), mask (uint8 of the count's
    rows, None when it is not written), stats (8 int32), conf (float), margin (1.0 when no update ran)."""
    points = np.asarray(points, np.float32)
    cap = points.shape[0] if mask_rows is None else min(points.shape[0], mask_rows)
    n = points.shape[0] if count is None else int(count)
    status = 0
    if n > cap:
        n, status = cap, ST_CLAMPED
    if n < 0:
        n = 0
    src, dst = np.ascontiguousarray(points[:n, 0:2]), np.ascontiguousarray(points[:n, 2:4])
    res = {"H": np.zeros((3, 3)), "mask": None, "stats": np.zeros(8, np.int32), "conf": 0.0, "margin": 1.0}
    margins = []
    st = res["stats"]
    try:
        if n < num_matches_thresh1:                                   # R:836
            return res
        p1 = find_homography2(src, dst, reproj_thresh, max_iters, confidence, margins)
        res["mask"] = p1.mask
        st[2], st[3], st[6] = p1.iters, p1.win, p1.attempts
        st[5] = -1
        if not p1.ok:
            return res
        status |= ST_H
        res["H"] = p1.H.reshape(3, 3).copy()
        if abs(det3(p1.H)) < DBL_EPSILON:                              # R:863
            status |= ST_DEGENERATE
            return res
        num_inliers = int(p1.mask.sum())                             # R:867-878
        st[1] = num_inliers
        c = num_inliers / (8 + 0.3 * n)
        res["conf"] = 0.0 if c > 3.0 else c
        if num_inliers < num_matches_thresh2:                         # R:881
            return res
        sel = p1.mask.astype(bool)
        p2 = find_homography2(src[sel], dst[sel], reproj_thresh, max_iters, confidence, margins)      # R:909
        status |= ST_PASS2
        st[4], st[5] = p2.iters, p2.win
        st[6] += p2.attempts
        if p2.ok:
            res["H"] = p2.H.reshape(3, 3).copy()
        else:
            status = (status | ST_PASS2_FAILED) & ~ST_H
            res["H"] = np.zeros((3, 3))
        return res
    finally:
        st[0] = status
        res["margin"] = min(margins) if margins else 1.0
