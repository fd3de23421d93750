"""The specification of isx_find_homography_lm (DESIGN.md §8 "Homography"): tests/helpers/homography_np.py's findHomography2 followed by the
Levenberg-Marquardt polish of R:672 (R = the reference's 计算单应性矩阵 demo), createLMSolver1(HomographyRefineCallback(src, dst), 10)->run(H8)
over the inliers, in Python floats.  homography_np is composed, not edited: find_homography2_lm calls find_homography2 and, under R:657-661's
condition, replaces H[0:8]; H[8] keeps the bits runKernel left (H8 aliases the first eight doubles of H, R:669).

compute() is R:432-453 and lm_run() is R:476-580, line by line.  float64 throughout from float32 points, + - * / sqrt fabs only, every
expression evaluated as written, left to right, no fused multiply-add: a device compiled with -ffp-contract=off can agree bit for bit.

The OpenCV calls inside LMSolverImpl1::run are in neither tree.  They are restated here from OpenCV 3.4.2's published source - each one
"recalled, unpinned", as cv::eigen already is - so parity with OpenCV is not pinned and this file is what the GPU is held to:
  mulTransposed(J, A, true)        recalled, unpinned: A[i][j], i <= j, is the sum over the rows k = 0 .. 2n-1 in order of J[k][i] J[k][j],
                                   from +0.0, mirrored.  (A structurally zero product adds +-0 to a sum that started at +0.0: skipping it
                                   gives the same bits while every J is finite - mul_transposed(skip_zeros=True) is tested against it.)
  gemm(J, r, 1, -, 0, v, GEMM_1_T) recalled, unpinned: v[i] is the sum over k in order of J[k][i] r[k], from +0.0.
  norm(., NORM_L2SQR)              recalled, unpinned: s += ((v0 v0 + v1 v1) + v2 v2) + v3 v3 while four remain, then one by one.
  norm(., NORM_INF)                recalled, unpinned: max |.|, a NaN is never taken (m < a is false).
  solve(Ap, v, d, DECOMP_EIG)      recalled, unpinned: JacobiImpl_ at n = 8 on Ap (jacobi_n, homography_np.jacobi_scalar's algorithm with n
                                   free; only the upper triangle is read), W descending with the rows of V, then SVBkSb: threshold =
                                   (sum of W[e] in order from +0.0) * (2 DBL_EPSILON); for e = 0 .. 7 with |W[e]| > threshold:
                                   s = (sum over j in order of V[e][j] v[j], from +0.0) * (1 / W[e]); d[j] = d[j] + s V[e][j]; d from zeros.
  gemm(A, d, -1, v, 2, temp_d)     recalled, unpinned: temp_d[i] = (-(sum over k in order of A[i][k] d[k], from +0.0)) + 2 v[i].
  a.dot(b), length 8               recalled, unpinned: two groups of four, r += ((a0 b0 + a1 b1) + a2 b2) + a3 b3, r from +0.0.
  invert(A, Ap, DECOMP_EIG)        recalled, unpinned: only its diagonal is read (R:541-542).  Jacobi on A, the same threshold rule,
                                   Ap[i][i] = the sum over the kept e in order of V[e][i] (V[e][i] (1 / W[e])), from +0.0.
  std::min / std::max              as the library writes them: max(a, b) = a < b ? b : a, min(a, b) = b < a ? b : a.
This model decides where OpenCV's text could be read otherwise (OpenCV's norm and dot are vectorised on some builds; the scalar loops above
are the ones restated); the device follows the model.

No pow or log is added: the `margin` rule of homography_np's iteration-count update carries over unchanged."""
import numpy as np

from . import homography_np as hm

DBL_EPSILON, FLT_EPSILON = hm.DBL_EPSILON, hm.FLT_EPSILON
ST_H, ST_PASS2, ST_PASS2_FAILED, ST_CLAMPED, ST_DEGENERATE = hm.ST_H, hm.ST_PASS2, hm.ST_PASS2_FAILED, hm.ST_CLAMPED, hm.ST_DEGENERATE
COUNTERS = ("r_hi", "lambda_zero", "r_lo", "invert", "accept", "reject", "stop_d", "stop_r", "stop_iter")


def jacobi_n(A, n):
    """homography_np.jacobi_scalar with n free: JacobiImpl_ for one symmetric n x n matrix in Python floats (the upper triangle is what is
    read).  Returns (W, V, rotations): W descending, the rows of V the eigenvectors."""
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
        t = abs(y) + hm._hypot1(p, y)
        s = hm._hypot1(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[n * k + l] = 0.0
        W[k] -= t
        W[l] += t
        for i in range(k):
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


def compute(h, src, dst, want_J):
    """HomographyRefineCallback::compute (R:432-453).  h: 8 floats; src, dst: (n, 2) float32.  Returns (err: 2n floats, J: 2n rows of 8
    floats, or None)."""
    err, J = [], [] if want_J else None
    for i in range(len(src)):
        Mx, My = float(src[i][0]), float(src[i][1])
        ww = (h[6] * Mx + h[7] * My) + 1.0
        ww = 1.0 / ww if abs(ww) > DBL_EPSILON else 0.0
        xi = ((h[0] * Mx + h[1] * My) + h[2]) * ww
        yi = ((h[3] * Mx + h[4] * My) + h[5]) * ww
        err.append(xi - float(dst[i][0]))
        err.append(yi - float(dst[i][1]))
        if want_J:
            J.append([Mx * ww, My * ww, ww, 0.0, 0.0, 0.0, ((-Mx) * ww) * xi, ((-My) * ww) * xi])
            J.append([0.0, 0.0, 0.0, Mx * ww, My * ww, ww, ((-Mx) * ww) * yi, ((-My) * ww) * yi])
    return err, J


_STRUCTURAL_ZERO = ((3, 4, 5), (0, 1, 2))         # the columns of an even row and of an odd row that compute() writes as 0.


def mul_transposed(J, skip_zeros=False):
    """mulTransposed(J, A, true): 8 rows of 8 floats."""
    A = [[0.0] * 8 for _ in range(8)]
    for i in range(8):
        for j in range(i, 8):
            s = 0.0
            for k, row in enumerate(J):
                if skip_zeros and (i in _STRUCTURAL_ZERO[k & 1] or j in _STRUCTURAL_ZERO[k & 1]):
                    continue
                s = s + row[i] * row[j]
            A[i][j] = A[j][i] = s
    return A


def gemm_1t(J, r):
    """gemm(J, r, 1, noArray(), 0, v, GEMM_1_T)."""
    v = []
    for i in range(8):
        s = 0.0
        for k, row in enumerate(J):
            s = s + row[i] * r[k]
        v.append(s)
    return v


def norm_l2sqr(v):
    s, k, n = 0.0, 0, len(v)
    while k + 4 <= n:
        s = s + (((v[k] * v[k] + v[k + 1] * v[k + 1]) + v[k + 2] * v[k + 2]) + v[k + 3] * v[k + 3])
        k += 4
    while k < n:
        s = s + v[k] * v[k]
        k += 1
    return s


def norm_inf(v):
    m = 0.0
    for x in v:
        a = abs(x)
        if m < a:
            m = a
    return m


def dot8(a, b):
    r = 0.0
    for k in (0, 4):
        r = r + (((a[k] * b[k] + a[k + 1] * b[k + 1]) + a[k + 2] * b[k + 2]) + a[k + 3] * b[k + 3])
    return r


def _eig_kept(A):
    """Jacobi at n = 8 and SVBkSb's threshold: (W, V, the e kept)."""
    W, V, _ = jacobi_n(A, 8)
    t = 0.0
    for e in range(8):
        t = t + W[e]
    t = t * (2.0 * DBL_EPSILON)
    return W, V, [e for e in range(8) if abs(W[e]) > t]


def solve_eig(Ap, v):
    """solve(Ap, v, d, DECOMP_EIG)."""
    W, V, kept = _eig_kept(Ap)
    d = [0.0] * 8
    for e in kept:
        s = 0.0
        for j in range(8):
            s = s + V[e][j] * v[j]
        s = s * (1.0 / W[e])
        for j in range(8):
            d[j] = d[j] + s * V[e][j]
    return d


def invert_eig_diag(A):
    """The diagonal of invert(A, Ap, DECOMP_EIG)."""
    W, V, kept = _eig_kept(A)
    out = []
    for i in range(8):
        s = 0.0
        for e in kept:
            s = s + V[e][i] * (V[e][i] * (1.0 / W[e]))
        out.append(s)
    return out


def lm_run(h8, src, dst, max_iters):
    """LMSolverImpl1::run (R:476-580) with HomographyRefineCallback(src, dst).  Returns (x: 8 floats, run()'s return value, nfJ, the branch
    counters, (the starting S, the final S))."""
    ctr = dict.fromkeys(COUNTERS, 0)
    x = [float(v) for v in h8]
    r, J = compute(x, src, dst, True)
    S = norm_l2sqr(r)
    S0 = S
    nfJ = 2
    A = mul_transposed(J)
    v = gemm_1t(J, r)
    D = [A[i][i] for i in range(8)]
    Rlo, Rhi = 0.25, 0.75
    lam, lc = 1.0, 0.75
    it = 0
    while True:
        Ap = [row[:] for row in A]
        for i in range(8):
            Ap[i][i] = Ap[i][i] + lam * D[i]
        d = solve_eig(Ap, v)
        xd = [x[i] - d[i] for i in range(8)]
        rd, _ = compute(xd, src, dst, False)
        nfJ += 1
        Sd = norm_l2sqr(rd)
        temp_d = []
        for i in range(8):
            s = 0.0
            for k in range(8):
                s = s + A[i][k] * d[k]
            temp_d.append((-s) + 2.0 * v[i])
        dS = dot8(d, temp_d)
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1.0)
        if R > Rhi:
            ctr["r_hi"] += 1
            lam = lam * 0.5
            if lam < lc:
                lam = 0.0
                ctr["lambda_zero"] += 1
        elif R < Rlo:
            ctr["r_lo"] += 1
            t = dot8(d, v)
            nu = (Sd - S) / (t if abs(t) > DBL_EPSILON else 1.0) + 2.0
            nu = 2.0 if nu < 2.0 else nu
            nu = 10.0 if 10.0 < nu else nu
            if lam == 0:
                ctr["invert"] += 1
                maxval = DBL_EPSILON
                for a in invert_eig_diag(A):
                    a = abs(a)
                    if maxval < a:
                        maxval = a
                lam = lc = 1.0 / maxval
                nu = nu * 0.5
            lam = lam * nu
        if Sd < S:
            ctr["accept"] += 1
            nfJ += 1
            S = Sd
            x, xd = xd, x
            r, J = compute(x, src, dst, True)
            A = mul_transposed(J)
            v = gemm_1t(J, r)
        else:
            ctr["reject"] += 1
        it += 1
        by_iter, by_d, by_r = not it < max_iters, not norm_inf(d) >= FLT_EPSILON, not norm_inf(r) >= FLT_EPSILON
        if by_iter or by_d or by_r:
            ctr["stop_iter"] += by_iter
            ctr["stop_d"] += by_d
            ctr["stop_r"] += by_r
            break
    return x, (-it if it == max_iters else it), nfJ, ctr, (S0, S)


def find_homography2_lm(src, dst, thresh, max_iters, confidence, margins, lm_max_iters=10):
    """findHomography2 (R:602-693) with RANSAC and the LM polish of R:672.  homography_np's _Run with three more fields: lm = (run()'s return
    value, nfJ) - (0, 0) where LM did not run -, counters (None then) and S = (starting, final)."""
    out = hm.find_homography2(src, dst, thresh, max_iters, confidence, margins)
    out.lm, out.counters, out.S = (0, 0), None, None
    if out.ok and len(src) > 4 and out.mask.any():                    # R:657-661; n == 4 never comes here
        sel = out.mask.astype(bool)
        H = np.array(out.H, np.float64).reshape(9).copy()
        x, ret, nfJ, out.counters, out.S = lm_run(H[0:8], src[sel], dst[sel], lm_max_iters)
        H[0:8] = x                                                    # H[8] keeps runKernel's bits (R:669)
        out.H, out.lm = H, (ret, nfJ)
    return out


def find_homography_lm_np(points, count=None, reproj_thresh=3.0, max_iters=2000, confidence=0.995, num_matches_thresh1=6, num_matches_thresh2=6,
                          mask_rows=None, lm_max_iters=10):
    """One pair of isx_find_homography_lm: homography_np.find_homography_np around find_homography2_lm (R:836-909; the degenerate test of R:863
    sees the polished H).  The same dict with 12 stats - columns 8, 9: run()'s return value and nfJ of pass 1; 10, 11: of pass 2 - and
    `counters`: per pass the branch counters of lm_run, or None."""
    points = np.asarray(points, np.float32)
    cap = points.shape[0] if mask_rows is None else min(points.shape[0], mask_rows)
    n = points.shape[0] if count is None else int(count)
    status = 0
    if n > cap:
        n, status = cap, ST_CLAMPED
    if n < 0:
        n = 0
    src, dst = np.ascontiguousarray(points[:n, 0:2]), np.ascontiguousarray(points[:n, 2:4])
    res = {"H": np.zeros((3, 3)), "mask": None, "stats": np.zeros(12, np.int32), "conf": 0.0, "margin": 1.0, "counters": [None, None],
           "S": [None, None]}
    margins = []
    st = res["stats"]
    try:
        if n < num_matches_thresh1:                                   # R:836
            return res
        p1 = find_homography2_lm(src, dst, reproj_thresh, max_iters, confidence, margins, lm_max_iters)
        res["mask"] = p1.mask
        st[2], st[3], st[6] = p1.iters, p1.win, p1.attempts
        st[5] = -1
        st[8], st[9] = p1.lm
        res["counters"][0], res["S"][0] = p1.counters, p1.S
        if not p1.ok:
            return res
        status |= ST_H
        res["H"] = p1.H.reshape(3, 3).copy()
        if abs(hm.det3(p1.H)) < DBL_EPSILON:                          # R:863
            status |= ST_DEGENERATE
            return res
        num_inliers = int(p1.mask.sum())                              # R:867-878
        st[1] = num_inliers
        c = num_inliers / (8 + 0.3 * n)
        res["conf"] = 0.0 if c > 3.0 else c
        if num_inliers < num_matches_thresh2:                         # R:881
            return res
        sel = p1.mask.astype(bool)
        p2 = find_homography2_lm(src[sel], dst[sel], reproj_thresh, max_iters, confidence, margins, lm_max_iters)      # R:909
        status |= ST_PASS2
        st[4], st[5] = p2.iters, p2.win
        st[6] += p2.attempts
        st[10], st[11] = p2.lm
        res["counters"][1], res["S"][1] = p2.counters, p2.S
        if p2.ok:
            res["H"] = p2.H.reshape(3, 3).copy()
        else:
            status = (status | ST_PASS2_FAILED) & ~ST_H
            res["H"] = np.zeros((3, 3))
        return res
    finally:
        st[0] = status
        res["margin"] = min(margins) if margins else 1.0
