"""The specification of isx_bundle_adjust_reproj and isx_wave_correct (DESIGN.md §8 "Reprojection adjuster", "Wave correction"):
detail::BundleAdjusterReproj and detail::waveCorrect - commented out in every main of the reference (W:190, W:198; C:340, C:355-361), the
defaults of cv::Stitcher and of stitching_detailed (--ba reproj, --wave_correct horiz) - in Python scalars.

The adjuster is helpers/bundle_np.py with another cost: lev_marq, chol_solve, lstsq_solve, Rodrigues both ways, the polar factor, inv3 and
mul3 are imported from there, and its three decisions (the Cholesky solve with the trace rule, the restated sin / cos / acos, the summation
orders fixed by TILE) hold here unchanged.  Restated from OpenCV 3.4.2's published source - recalled, UNPINNED, as every OpenCV call of
this project:
  BundleAdjusterReproj::setUpInitialCameraParams   7 parameters a camera: focal, ppx, ppy, aspect, rvec[3]; rvec as BundleAdjusterRay's (the
                                                   float32 R, its polar factor, Rodrigues, read as float32);
  calcError                                        per edge (i, j): H = ((K2 * R2.inv()) * R1) * K1.inv() with
                                                   K = [[f, 0, ppx], [0, f * aspect, ppy], [0, 0, 1]] and R = Rodrigues(rvec); per inlier
                                                   match x, y, z = H (p1.x, p1.y, 1), each row summed as bundle_np.ray sums it; the two
                                                   residuals p2.x - x / z and p2.y - y / z (a z of 0: what IEEE division gives);
  calcJacobian                                     central differences, step 1e-4, val - step, val + step, restore; (e1 - e0) / (2 step); a
                                                   parameter whose refinement bit is clear has no column computed: it stays zero, its pivot
                                                   falls under the trace rule of chol_solve, its step is 0 and ST_DROPPED is set;
  obtainRefinedCameraParams                        focal, ppx, ppy, aspect = the parameters; R = Rodrigues(rvec) as float32; then
                                                   BundleAdjusterBase's R_i = R_center.inv() * R_i.
refine_flags is OpenCV's refinement mask as bits: 1 (0,0) focal, 2 (0,1) unused, 4 (0,2) ppx, 8 (1,1) aspect, 16 (1,2) ppy.
Summation orders: tiles of TILE matches, the two residuals of a match in order, tiles then edges in order; a tile carries 120 sums - the
105 upper entries of its 14 x 14 block over the edge's two cameras, 14 of J^T err, the sum of err^2.

wave_correct is waveCorrect(rmats, kind) in np.float32 scalars, one rounded operation per parenthesis: moment = sum of col0 col0^T in image
order; cv::eigen by the Jacobi of homography_lm_np.jacobi_n run in float32 with the threshold FLT_EPSILON (eigenvalues descending,
eigenvectors as rows); rg1 = row 2 (HORIZ) or row 0 (VERT); img_k = sum of col2; rg0 = rg1 x img_k; norm(rg0) <= DBL_MIN passes the rig
through; rg0 /= norm; rg2 = rg0 x rg1; conf = sum of rg0 . col0 (HORIZ) or minus the sum of rg1 . col0 (VERT), accumulated in float32 (THIS
PROJECT'S: OpenCV holds the norm and conf in a double); conf < 0 negates rg0 and rg1; R_i = [rg0; rg1; rg2] * R_i.  A rig of one image
passes through."""
import numpy as np

from . import bundle_np as bm
from . import estimator_np as em
from .bundle_np import (DBL_EPSILON, LAMBDA, MAX_IMAGES, RIG_EDGES, RIG_ERR_EVALS, RIG_ITERS, RIG_JAC_EVALS, RIG_LAMBDA_LG10,  # noqa: F401
                        RIG_MATCHES, RIG_STATUS, ST_DROPPED, ST_EST_ASSERT, ST_NAN, ST_NO_EDGES, ST_SINGULAR_R, TILE, _div, _f32, _sqrt, _tiles,
                        chol_solve, inv3, lev_marq, lstsq_solve, mul3, polar, rodrigues_mat, rodrigues_vec)

STEP = 1e-4
PC = 7                                        # parameters a camera: focal, ppx, ppy, aspect, rvec[3]
REFINE_FOCAL, REFINE_PPX, REFINE_ASPECT, REFINE_PPY, REFINE_ALL = 1, 4, 8, 16, 31
_BIT = (REFINE_FOCAL, REFINE_PPX, REFINE_PPY, REFINE_ASPECT)      # of parameters 0 - 3
WAVE_HORIZ, WAVE_VERT = 0, 1
WAVE_DEGENERATE, WAVE_SINGLE = 1, 2
DBL_MIN = 2.2250738585072014e-308
_UPPER = [(a, b) for a in range(14) for b in range(a, 14)]


def refined(flags, q):
    return q >= 4 or bool(flags & _BIT[q])


def cam_k(p):
    return [p[0], 0.0, p[1], 0.0, p[0] * p[3], p[2], 0.0, 0.0, 1.0]


def edge_h(p1, p2):
    """calcError's H of the edge (camera 1 = from, camera 2 = to) from the seven parameters of each."""
    R1, R2 = rodrigues_mat(p1[4:7]), rodrigues_mat(p2[4:7])
    return mul3(mul3(mul3(cam_k(p2), inv3(R2)), R1), inv3(cam_k(p1)))


def reproj_err(H, x1, y1, x2, y2):
    X = ((H[0] * x1) + (H[1] * y1)) + H[2]
    Y = ((H[3] * x1) + (H[4] * y1)) + H[5]
    Z = ((H[6] * x1) + (H[7] * y1)) + H[8]
    return (x2 - _div(X, Z), y2 - _div(Y, Z))


class Rig:
    """One rig's problem: n cameras and edges [(i, j, pts)], pts the inlier matches of the edge in order as (x1, y1, x2, y2) floats."""

    def __init__(self, n, edges, flags=REFINE_ALL):
        self.n, self.edges, self.flags = n, edges, flags

    def errors(self, p):
        out = []
        for (i, j, pts) in self.edges:
            H = edge_h(p[PC * i:PC * i + PC], p[PC * j:PC * j + PC]) if pts else None
            out.append([reproj_err(H, *pt) for pt in pts])
        return out

    def err_norm(self, p):
        s = 0.0
        for rows in self.errors(p):
            for (t0, t1) in _tiles(len(rows)):
                ts = 0.0
                for e in rows[t0:t1]:
                    for k in range(2):
                        ts = ts + e[k] * e[k]
                s = s + ts
        return _sqrt(s)

    def jacobian(self, p):
        """calcJacobian, compact: per edge, per inlier match (err[2], J[2][14]) with columns 0 - 6 the parameters of camera i and 7 - 13
        those of camera j (every other column of the row is structurally zero)."""
        h2 = 2.0 * STEP
        out = []
        for (i, j, pts) in self.edges:
            if not pts:
                out.append([])
                continue
            a, b = list(p[PC * i:PC * i + PC]), list(p[PC * j:PC * j + PC])
            H0 = edge_h(a, b)
            Hv = {}
            for col in range(14):
                q = col % PC
                if not refined(self.flags, q):
                    continue
                val = (b if col >= PC else a)[q]
                for sg, v in ((0, val - STEP), (1, val + STEP)):
                    aa, bb = list(a), list(b)
                    (bb if col >= PC else aa)[q] = v
                    Hv[(col, sg)] = edge_h(aa, bb)
            rows = []
            for (x1, y1, x2, y2) in pts:
                err = list(reproj_err(H0, x1, y1, x2, y2))
                J = [[0.0] * 14 for _ in range(2)]
                for col in range(14):
                    if (col, 0) not in Hv:
                        continue
                    e0, e1 = reproj_err(Hv[(col, 0)], x1, y1, x2, y2), reproj_err(Hv[(col, 1)], x1, y1, x2, y2)
                    for k in range(2):
                        J[k][col] = _div(e1[k] - e0[k], h2)
                rows.append((err, J))
            out.append(rows)
        return out

    def tile_sums(self, jac):
        """Per edge the list of its tiles' (105 upper entries of the 14 x 14 block, 14 of J^T err, the sum of err^2): 120 sums a tile."""
        out = []
        for rows in jac:
            ts = []
            for (t0, t1) in _tiles(len(rows)):
                blk = []
                for (a, b) in _UPPER:
                    s = 0.0
                    for (err, J) in rows[t0:t1]:
                        for k in range(2):
                            s = s + J[k][a] * J[k][b]
                    blk.append(s)
                g = []
                for a in range(14):
                    s = 0.0
                    for (err, J) in rows[t0:t1]:
                        for k in range(2):
                            s = s + J[k][a] * err[k]
                    g.append(s)
                s = 0.0
                for (err, J) in rows[t0:t1]:
                    for k in range(2):
                        s = s + err[k] * err[k]
                ts.append((blk, g, s))
            out.append(ts)
        return out

    def jac_err(self, p):
        """(JtJ, JtErr, |err|) at p: the tiles of every edge that touches the camera(s) in edge order, tile order, from +0.0."""
        n, N = self.n, PC * self.n
        tiles = self.tile_sums(self.jacobian(p))
        upper = {ab: k for k, ab in enumerate(_UPPER)}
        edge_of = {(i, j): e for e, (i, j, _) in enumerate(self.edges)}
        JtJ = [[0.0] * N for _ in range(N)]
        JtErr = [0.0] * N
        for c in range(n):
            touching = []                                      # (edge, 0 or 7: where c's columns start) in edge order
            for o in range(n):
                if o < c and (o, c) in edge_of:
                    touching.append((edge_of[(o, c)], PC))
                elif o > c and (c, o) in edge_of:
                    touching.append((edge_of[(c, o)], 0))
            for a in range(PC):
                s = 0.0
                for (e, off) in touching:
                    for (blk, g, ss) in tiles[e]:
                        s = s + g[off + a]
                JtErr[PC * c + a] = s
                for b in range(a, PC):
                    s = 0.0
                    for (e, off) in touching:
                        for (blk, g, ss) in tiles[e]:
                            s = s + blk[upper[(off + a, off + b)]]
                    JtJ[PC * c + a][PC * c + b] = JtJ[PC * c + b][PC * c + a] = s
            for d in range(c + 1, n):
                if (c, d) not in edge_of:
                    continue
                for a in range(PC):
                    for b in range(PC):
                        s = 0.0
                        for (blk, g, ss) in tiles[edge_of[(c, d)]]:
                            s = s + blk[upper[(a, PC + b)]]
                        JtJ[PC * c + a][PC * d + b] = JtJ[PC * d + b][PC * c + a] = s
        s = 0.0
        for ts in tiles:
            for (blk, g, ss) in ts:
                s = s + ss
        return JtJ, JtErr, _sqrt(s)

    def dense_jtj(self, p):
        """The test's dense reference: J whole (2 total_matches x 7n), J^T J and J^T err over all rows in order - no tiles, zeros multiplied.
        Equal to jac_err's bits where no edge has more than one tile (and J is finite)."""
        jac = self.jacobian(p)
        N = PC * self.n
        rows, errs = [], []
        for (i, j, _), ms in zip(self.edges, jac):
            for (err, J) in ms:
                for k in range(2):
                    r = [0.0] * N
                    r[PC * i:PC * i + PC] = J[k][0:PC]
                    r[PC * j:PC * j + PC] = J[k][PC:2 * PC]
                    rows.append(r)
                    errs.append(err[k])
        JtJ = [[0.0] * N for _ in range(N)]
        JtErr = [0.0] * N
        for a in range(N):
            s = 0.0
            for r, e in zip(rows, errs):
                s = s + r[a] * e
            JtErr[a] = s
            for b in range(a, N):
                s = 0.0
                for r in rows:
                    s = s + r[a] * r[b]
                JtJ[a][b] = JtJ[b][a] = s
        return JtJ, JtErr


def _kr_row(c, R32):
    with np.errstate(all="ignore"):
        k = np.array([c[0], 0.0, c[2], 0.0, c[0] * c[1], c[3], 0.0, 0.0, 1.0], np.float64).astype(np.float32)
    return np.concatenate([k, np.asarray(R32, np.float32)])


def gather_edges(keypoints, pairs, matches, masks, counts, conf, conf_thresh):
    """The edges of a rig as BundleAdjusterBase::estimate lays them out (bundle_np.adjust_rig's rule)."""
    order = sorted(range(len(pairs)), key=lambda k: (pairs[k][0], pairs[k][1]))
    edges = []
    for k in order:
        if not float(conf[k]) > conf_thresh:
            continue
        i, j = pairs[k]
        m = np.asarray(matches[k]).reshape(-1, 3)
        mk = np.asarray(masks[k]).reshape(-1)
        cnt = max(0, min(int(counts[k]), m.shape[0], mk.shape[0]))
        ki, kj = np.asarray(keypoints[i], np.float32).reshape(-1, 2), np.asarray(keypoints[j], np.float32).reshape(-1, 2)
        pts = []
        for r in range(cnt):
            q, t = int(m[r, 0]), int(m[r, 1])
            if mk[r] != 0 and 0 <= q < ki.shape[0] and 0 <= t < kj.shape[0]:
                pts.append((float(ki[q, 0]), float(ki[q, 1]), float(kj[t, 0]), float(kj[t, 1])))
        edges.append((i, j, pts))
    return edges


def adjust_rig(sizes, keypoints, pairs, matches, masks, counts, conf, est_rig_stats, cameras_in, conf_thresh=1.0, max_iter=1000,
               eps=DBL_EPSILON, refine_flags=REFINE_ALL, solve=chol_solve):
    """BundleAdjusterReproj on one rig; arguments and the returned dict as bundle_np.adjust_rig's (sizes only counts the images)."""
    n = len(sizes)
    cams_in = np.asarray(cameras_in, np.float64).reshape(n, 16)
    edges = gather_edges(keypoints, pairs, matches, masks, counts, conf, conf_thresh)
    total = sum(len(e[2]) for e in edges)
    status = 0
    center = int(est_rig_stats[em.RIG_CENTER0])
    if int(est_rig_stats[em.RIG_STATUS]) & em.EST_ASSERT or not 0 <= center < n:
        status |= ST_EST_ASSERT
    if not edges:
        status |= ST_NO_EDGES
    stats = np.zeros(8, np.int32)
    stats[RIG_EDGES], stats[RIG_MATCHES] = len(edges), total
    if status:
        stats[RIG_STATUS] = status
        cams, kr = bm._passthrough(cams_in)
        return dict(cameras=cams, kr32=kr, rig_stats=stats, rig_err=np.zeros(2))
    param = []
    for i in range(n):                                         # setUpInitialCameraParams
        Q, ok = polar([_f32(v) for v in cams_in[i, 4:13]])
        if not ok:
            status |= ST_SINGULAR_R
        param += [float(cams_in[i, 0]), float(cams_in[i, 2]), float(cams_in[i, 3]), float(cams_in[i, 1])] + [_f32(v) for v in rodrigues_vec(Q)]
    rig = Rig(n, edges, refine_flags)
    param, info = lev_marq(param, rig.jac_err, rig.err_norm, max_iter, eps, solve)
    if info["dropped"]:
        status |= ST_DROPPED
    stats[RIG_ITERS], stats[RIG_JAC_EVALS], stats[RIG_ERR_EVALS], stats[RIG_LAMBDA_LG10] = info["iters"], info["jac_evals"], info["err_evals"], info["lambda_lg10"]
    err = np.array([info["first"], info["last"]])
    if any(p != p for p in param):                             # estimate returns false
        stats[RIG_STATUS] = status | ST_NAN
        cams, kr = bm._passthrough(cams_in)
        return dict(cameras=cams, kr32=kr, rig_stats=stats, rig_err=err, param=param, info=info)
    R32 = [[_f32(v) for v in rodrigues_mat(param[PC * i + 4:PC * i + 7])] for i in range(n)]      # obtainRefinedCameraParams
    Rinv = inv3(R32[center])
    cams = cams_in.copy()
    kr = np.zeros((n, 18), np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            Ri = np.array(mul3(Rinv, R32[i]), np.float64).astype(np.float32)
            cams[i, 0], cams[i, 2], cams[i, 3], cams[i, 1] = param[PC * i:PC * i + 4]
            cams[i, 4:13] = Ri.astype(np.float64)
            kr[i] = _kr_row(cams[i], Ri)
    stats[RIG_STATUS] = status
    return dict(cameras=cams, kr32=kr, rig_stats=stats, rig_err=err, param=param, info=info)


def adjust(sizes, keypoints, pairs, matches, masks, counts, conf, est_rig_stats, cameras_in, rig_first=None, conf_thresh=1.0, max_iter=1000,
           eps=DBL_EPSILON, refine_flags=REFINE_ALL):
    """isx_bundle_adjust_reproj: every rig of a call.  pairs: global image indices.  Returns (cameras, kr32, rig_stats, rig_err) stacked."""
    n = len(sizes)
    rig_first = [0, n] if rig_first is None else [int(v) for v in rig_first]
    est = np.asarray(est_rig_stats).reshape(len(rig_first) - 1, -1)
    counts, conf = np.asarray(counts).reshape(-1), np.asarray(conf).reshape(-1)
    outs = []
    for r in range(len(rig_first) - 1):
        a, b = rig_first[r], rig_first[r + 1]
        ks = [k for k, (i, j) in enumerate(pairs) if a <= i < b]
        outs.append(adjust_rig([sizes[i] for i in range(a, b)], [keypoints[i] for i in range(a, b)], [(pairs[k][0] - a, pairs[k][1] - a) for k in ks],
                               [matches[k] for k in ks], [masks[k] for k in ks], [counts[k] for k in ks], [conf[k] for k in ks], est[r],
                               np.asarray(cameras_in, np.float64)[a:b], conf_thresh, max_iter, eps, refine_flags))
    return (np.concatenate([o["cameras"] for o in outs]), np.concatenate([o["kr32"] for o in outs]), np.stack([o["rig_stats"] for o in outs]),
            np.stack([o["rig_err"] for o in outs]))


# ---- waveCorrect ----------------------------------------------------------------------------------------------------------------------------
_T = np.float32
FLT_EPSILON = _T(1.1920929e-07)


def _hypot32(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(_T(1) + (b * b))
    if b > 0:
        a = a / b
        return b * np.sqrt(_T(1) + (a * a))
    return _T(0)


def jacobi3_f32(A):
    """homography_lm_np.jacobi_n at n = 3 in np.float32 scalars, the threshold FLT_EPSILON: cv::eigen of a CV_32F 3 x 3.  Returns (W
    descending, V: the eigenvectors as rows)."""
    n = 3
    A = [_T(v) for v in np.asarray(A, np.float32).reshape(9)]
    V = [_T(0)] * 9
    for i in range(n):
        V[i * n + i] = _T(1)
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
    with np.errstate(all="ignore"):
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
            if abs(p) <= FLT_EPSILON:
                break
            y = (W[l] - W[k]) * _T(0.5)
            t = abs(y) + _hypot32(p, y)
            s = _hypot32(p, t)
            c = t / s
            s = p / s
            t = (p / t) * p
            if y < 0:
                s, t = -s, -t
            A[n * k + l] = _T(0)
            W[k] = W[k] - t
            W[l] = W[l] + t

            def rot(M, i0, i1):
                a0, b0 = M[i0], M[i1]
                M[i0], M[i1] = (a0 * c) - (b0 * s), (a0 * s) + (b0 * c)

            for i in range(k):
                rot(A, n * i + k, n * i + l)
            for i in range(k + 1, l):
                rot(A, n * k + i, n * i + l)
            for i in range(l + 1, n):
                rot(A, n * k + i, n * l + i)
            for i in range(n):
                rot(V, n * k + i, n * l + i)
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
    return W, [V[0:3], V[3:6], V[6:9]]


def _cross(a, b):
    return [(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])]


def wave_matrix(Rs, kind=WAVE_HORIZ):
    """(the correction [rg0; rg1; rg2] of a rig: 9 np.float32, its status, whether conf < 0 negated rg0 and rg1); Rs: per image 9 values,
    rounded to float32 here."""
    Rs = [[_T(v) for v in np.asarray(R, np.float64).reshape(9)] for R in Rs]
    if len(Rs) <= 1:
        return None, WAVE_SINGLE, False
    with np.errstate(all="ignore"):
        moment = [_T(0)] * 9
        k = [_T(0)] * 3
        for R in Rs:
            col = (R[0], R[3], R[6])
            for r in range(3):
                for q in range(3):
                    moment[3 * r + q] = moment[3 * r + q] + (col[r] * col[q])
            k = [k[0] + R[2], k[1] + R[5], k[2] + R[8]]
        _, V = jacobi3_f32(moment)
        rg1 = list(V[2] if kind == WAVE_HORIZ else V[0])
        rg0 = _cross(rg1, k)
        nrm = np.sqrt(((rg0[0] * rg0[0]) + (rg0[1] * rg0[1])) + (rg0[2] * rg0[2]))
        if float(nrm) <= DBL_MIN:
            return None, WAVE_DEGENERATE, False
        rg0 = [v / nrm for v in rg0]
        rg2 = _cross(rg0, rg1)
        rg = rg0 if kind == WAVE_HORIZ else rg1
        conf = _T(0)
        for R in Rs:
            d = ((rg[0] * R[0]) + (rg[1] * R[3])) + (rg[2] * R[6])
            conf = conf + d if kind == WAVE_HORIZ else conf - d
        flipped = bool(conf < 0)
        if flipped:
            rg0, rg1 = [-v for v in rg0], [-v for v in rg1]
    return [_T(v) for v in rg0 + rg1 + rg2], 0, flipped


def wave_correct(cameras_in, rig_first=None, kind=WAVE_HORIZ):
    """isx_wave_correct: cameras_in n x 16 float64.  Returns (cameras n x 16 float64, kr32 n x 18 float32, rig_stats rigs x 2 int32)."""
    cams_in = np.asarray(cameras_in, np.float64)
    n = cams_in.shape[0]
    rig_first = [0, n] if rig_first is None else [int(v) for v in rig_first]
    cams = cams_in.copy()
    kr = np.zeros((n, 18), np.float32)
    stats = np.zeros((len(rig_first) - 1, 2), np.int32)
    with np.errstate(all="ignore"):
        for r in range(len(rig_first) - 1):
            a, b = rig_first[r], rig_first[r + 1]
            Rw, status, _ = wave_matrix([cams_in[i, 4:13] for i in range(a, b)], kind)
            stats[r] = [status, b - a]
            for i in range(a, b):
                R = [_T(v) for v in cams_in[i, 4:13]]
                if status == 0:
                    R = [((Rw[3 * p] * R[q]) + (Rw[3 * p + 1] * R[3 + q])) + (Rw[3 * p + 2] * R[6 + q]) for p in range(3) for q in range(3)]
                    cams[i, 4:13] = np.array(R, np.float32).astype(np.float64)
                kr[i] = _kr_row(cams_in[i], R)
    return cams, kr, stats
