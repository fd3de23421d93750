"""The specification of isx_estimate_cameras (DESIGN.md §8 "Camera estimator"): HomographyBasedEstimator1 of the reference's 恢复相机内参数
demo (C = its 恢复相机内参数.cpp) in NumPy - focalsFromHomography1 (C:26-54), estimateFocal1 (C:55-105), findMaxSpanningTree (C:145-213),
CalcRotation (C:215-243), estimate (C:246-284) and the float32 conversions of C:329-334 and C:385-386.

float64 arithmetic is IEEE + - * / sqrt only, on np.float64 scalars, one rounded operation per statement or per parenthesis, in the order
written (no fused multiply-add), so a device compiled with -ffp-contract=off can agree bit for bit.  Run it under np.errstate(all="ignore")
(estimate() does): a division by zero gives inf or NaN as in C++.

Restated, because their source is in neither tree (parity with OpenCV is therefore UNPINNED; this file is what the GPU is held to):
  Mat::inv() of a 3 x 3 CV_64F   cofactors times the reciprocal determinant, as OpenCV 3.4.2's invert() does for 3 x 3; a determinant of
                                 exactly 0 gives nine zeros (inv3);
  Mat * Mat of 3 x 3             three-term sums, left to right (mul3);
  CameraParams()                 focal 1, aspect 1, ppx = ppy = 0, R = eye, t = 0;  CameraParams::K();
  Graph::walkBreadthFirst        adjacency in insertion order, func(edge) on each edge to an unvisited vertex (util_inl.hpp).
The one choice the reference leaves open is the order of std::sort among edges of equal weight (C:169; (i, j) and (j, i) always tie).  It
is fixed here: weight descending, then i * num_images + j ascending.  The weight (float)num_inliers (C:158) is compared as the integer it
came from: a float32 holds every integer up to 2^24 and the matcher's row limit keeps num_inliers below 2^21.

A pair list is the homography stage's: (from, to) with from < to, H (3 x 3), stats (column 0 the status bits, column 1 num_inliers).  The
entry of the ordered pair (i, j), i < j, is that H where status bit ST_H is set; the entry of (j, i) is the dual the reference's matcher
stores, inv3(H) with the same num_inliers.  Image indices inside a rig are local to it."""
import numpy as np

F = np.float64
ST_H = 1                                      # ISX_HOMOGRAPHY_H
EST_MEDIAN, EST_ASSERT, EST_UNREACHED = 1, 2, 4
MAX_IMAGES = 64
RIG_STATUS, RIG_CANDIDATES, RIG_CENTER0, RIG_CENTER1, RIG_TREE_EDGES, RIG_REACHED, RIG_NUM_CENTERS, RIG_MIN_MAX_DIST = range(8)
_ZERO, _ONE, _HALF = F(0.0), F(1.0), F(0.5)


def inv3(m):
    """Mat::inv() (DECOMP_LU) of a 3 x 3 CV_64F as OpenCV 3.4.2 computes it; m: 9 float64, row-major."""
    a = (m[4] * m[8]) - (m[5] * m[7])
    b = (m[3] * m[8]) - (m[5] * m[6])
    c = (m[3] * m[7]) - (m[4] * m[6])
    d = ((m[0] * a) - (m[1] * b)) + (m[2] * c)
    if not d != _ZERO:
        return [_ZERO] * 9
    d = _ONE / d
    return [((m[4] * m[8]) - (m[5] * m[7])) * d, ((m[2] * m[7]) - (m[1] * m[8])) * d, ((m[1] * m[5]) - (m[2] * m[4])) * d,
            ((m[5] * m[6]) - (m[3] * m[8])) * d, ((m[0] * m[8]) - (m[2] * m[6])) * d, ((m[2] * m[3]) - (m[0] * m[5])) * d,
            ((m[3] * m[7]) - (m[4] * m[6])) * d, ((m[1] * m[6]) - (m[0] * m[7])) * d, ((m[0] * m[4]) - (m[1] * m[3])) * d]


def mul3(a, b):
    """Mat * Mat of two 3 x 3 CV_64F: each element a three-term sum, left to right."""
    return [((a[3 * r] * b[c]) + (a[3 * r + 1] * b[3 + c])) + (a[3 * r + 2] * b[6 + c]) for r in range(3) for c in range(3)]


def focals_from_homography(h):
    """C:26-54; h: 9 float64.  Returns (f0, f1, f0_ok, f1_ok); a focal that is not ok is returned as 0."""
    d1 = h[6] * h[7]                                                                # C:36
    d2 = (h[7] - h[6]) * (h[7] + h[6])                                              # C:37
    v1 = (-((h[0] * h[1]) + (h[3] * h[4]))) / d1                                    # C:38
    v2 = ((((h[0] * h[0]) + (h[3] * h[3])) - (h[1] * h[1])) - (h[4] * h[4])) / d2   # C:39
    f1, f1_ok = _ZERO, True
    if v1 < v2:                                                                     # C:40
        v1, v2 = v2, v1
    if v1 > 0 and v2 > 0:                                                           # C:41
        f1 = np.sqrt(v1 if abs(d1) > abs(d2) else v2)
    elif v1 > 0:                                                                    # C:42
        f1 = np.sqrt(v1)
    else:                                                                           # C:43
        f1_ok = False
    d1 = (h[0] * h[3]) + (h[1] * h[4])                                              # C:46
    d2 = (((h[0] * h[0]) + (h[1] * h[1])) - (h[3] * h[3])) - (h[4] * h[4])          # C:47
    v1 = ((-h[2]) * h[5]) / d1                                                      # C:48
    v2 = ((h[5] * h[5]) - (h[2] * h[2])) / d2                                       # C:49
    f0, f0_ok = _ZERO, True
    if v1 < v2:                                                                     # C:50
        v1, v2 = v2, v1
    if v1 > 0 and v2 > 0:                                                           # C:51
        f0 = np.sqrt(v1 if abs(d1) > abs(d2) else v2)
    elif v1 > 0:                                                                    # C:52
        f0 = np.sqrt(v1)
    else:                                                                           # C:53
        f0_ok = False
    return f0, f1, f0_ok, f1_ok


def pair_entries(n, pairs, H, stats):
    """pairwise_matches as the estimator reads it: {(i, j): (9 float64, num_inliers)} for every ordered pair whose H is not empty."""
    out = {}
    for k, (i, j) in enumerate(pairs):
        assert 0 <= i < j < n, (i, j, n)
        if int(stats[k][0]) & ST_H:
            h = [F(v) for v in np.asarray(H[k], np.float64).reshape(9)]
            w = int(stats[k][1])
            out[(i, j)] = (h, w)
            out[(j, i)] = (inv3(h), w)
    return out


def estimate_focal(n, sizes_wh, entries):
    """C:55-105.  Returns (focal, used_median, number of candidates)."""
    all_focals = []
    for i in range(n):
        for j in range(n):
            if (i, j) not in entries:
                continue
            f0, f1, ok0, ok1 = focals_from_homography(entries[(i, j)][0])
            if ok0 and ok1:
                all_focals.append(np.sqrt(f0 * f1))                                 # C:76
    cnt = len(all_focals)
    if cnt >= n - 1:                                                                # C:84
        all_focals.sort()
        if cnt % 2 == 1:
            return all_focals[cnt // 2], True, cnt
        return (all_focals[cnt // 2 - 1] + all_focals[cnt // 2]) * _HALF, True, cnt  # C:92
    s = _ZERO
    for i in range(n):
        s = s + F(int(sizes_wh[i][0]) + int(sizes_wh[i][1]))                        # C:101: an int sum, then one double add
    return s / F(n), False, cnt                                                     # C:103


def walk_breadth_first(adj, start, func):
    """Graph::walkBreadthFirst of OpenCV's util_inl.hpp."""
    was = [False] * len(adj)
    was[start] = True
    queue = [start]
    at = 0
    while at < len(queue):
        v = queue[at]
        at += 1
        for to in adj[v]:
            if not was[to]:
                func(v, to)
                was[to] = True
                queue.append(to)


def find_max_spanning_tree(n, entries):
    """C:145-213.  Returns (adjacency of the tree, tree edges in the order chosen, centers, min-max distance)."""
    edges = sorted(entries, key=lambda e: (-entries[e][1], e[0] * n + e[1]))        # C:169 with the tie rule of this file
    comp = list(range(n))
    adj = [[] for _ in range(n)]
    powers = [0] * n
    tree = []
    for (a, b) in edges:
        if comp[a] != comp[b]:
            ca, cb = comp[a], comp[b]
            comp = [ca if c == cb else c for c in comp]
            adj[a].append(b)
            adj[b].append(a)
            powers[a] += 1
            powers[b] += 1
            tree.append((a, b))
    leafs = [i for i in range(n) if powers[i] == 1]
    max_dists = [0] * n
    for leaf in leafs:
        cur = [0] * n

        def inc(frm, to, cur=cur):
            cur[to] = cur[frm] + 1
        walk_breadth_first(adj, leaf, inc)
        max_dists = [max(a, b) for a, b in zip(max_dists, cur)]
    min_max = min(max_dists)
    centers = [i for i in range(n) if max_dists[i] == min_max]
    return adj, tree, centers, min_max


def estimate_rig(sizes_wh, pairs, H, stats, focals_in=None):
    """C:246-284 for one rig plus the conversions of C:329-334 and C:385-386.  sizes_wh: (width, height) per image; pairs, H, stats: see the
    header; focals_in: None (is_focals_estimated = false) or per image (focal, aspect, ppx, ppy).  Returns a dict: cameras (n x 16
    float64: focal, aspect, ppx, ppy, R[9], t[3]), kr32 (n x 18 float32: K()[9], R[9]), tree (n x 2 int32: parent, -1 the root, -2 not
    reached; depth, -1 not reached), rig_stats (8 int32: status bits, focal candidates, the two centers or -1, tree edges, cameras reached,
    centers, the min-max distance), tree_edges."""
    n = len(sizes_wh)
    assert 2 <= n <= MAX_IMAGES
    with np.errstate(all="ignore"):
        entries = pair_entries(n, pairs, H, stats)
        status, cand = 0, 0
        if focals_in is None:                                                       # C:253-261
            f, med, cand = estimate_focal(n, sizes_wh, entries)
            status |= EST_MEDIAN if med else 0
            focal, aspect, ppx, ppy = [f] * n, [_ONE] * n, [_ZERO] * n, [_ZERO] * n
        else:                                                                       # C:264-268
            fi = np.asarray(focals_in, np.float64).reshape(n, 4)
            focal, aspect = [F(v) for v in fi[:, 0]], [F(v) for v in fi[:, 1]]
            ppx = [F(fi[i, 2]) - (_HALF * F(int(sizes_wh[i][0]))) for i in range(n)]
            ppy = [F(fi[i, 3]) - (_HALF * F(int(sizes_wh[i][1]))) for i in range(n)]
        adj, tree_edges, centers, min_max = find_max_spanning_tree(n, entries)
        eye = [_ONE, _ZERO, _ZERO, _ZERO, _ONE, _ZERO, _ZERO, _ZERO, _ONE]
        R = [list(eye) for _ in range(n)]
        parent, depth = [-2] * n, [-1] * n
        reached = 0
        if 1 <= len(centers) <= 2:                                                  # C:212
            def K(i):
                return [focal[i], _ZERO, ppx[i], _ZERO, focal[i] * aspect[i], ppy[i], _ZERO, _ZERO, _ONE]

            def calc(frm, to):                                                      # C:220-238
                r_edge = mul3(mul3(inv3(K(frm)), inv3(entries[(frm, to)][0])), K(to))
                R[to] = mul3(R[frm], r_edge)
                parent[to], depth[to] = frm, depth[frm] + 1
            parent[centers[0]], depth[centers[0]] = -1, 0
            walk_breadth_first(adj, centers[0], calc)                               # C:275
            reached = sum(1 for p in parent if p != -2)
            if reached < n:
                status |= EST_UNREACHED
        else:
            status |= EST_ASSERT
        for i in range(n):                                                          # C:278-282
            ppx[i] = ppx[i] + (_HALF * F(int(sizes_wh[i][0])))
            ppy[i] = ppy[i] + (_HALF * F(int(sizes_wh[i][1])))
        cams = np.zeros((n, 16), np.float64)
        kr32 = np.zeros((n, 18), np.float32)
        for i in range(n):
            cams[i, 0:4] = [focal[i], aspect[i], ppx[i], ppy[i]]
            cams[i, 4:13] = R[i]
            k = [focal[i], _ZERO, ppx[i], _ZERO, focal[i] * aspect[i], ppy[i], _ZERO, _ZERO, _ONE]     # CameraParams::K()
            kr32[i, 0:9] = np.array(k, np.float64).astype(np.float32)               # C:386
            kr32[i, 9:18] = np.array(R[i], np.float64).astype(np.float32)           # C:332
        rig = np.array([status, cand, centers[0] if len(centers) > 0 else -1, centers[1] if len(centers) > 1 else -1, len(tree_edges), reached,
                        len(centers), min_max], np.int32)
        return {"cameras": cams, "kr32": kr32, "tree": np.array([parent, depth], np.int32).T.copy(), "rig_stats": rig, "tree_edges": tree_edges}


def estimate(sizes_wh, pairs, H, stats, rig_first=None, focals_in=None):
    """isx_estimate_cameras: every rig of a call.  pairs: global image indices; H: num_pairs x 3 x 3 (or 3 num_pairs x 3); stats: num_pairs x
    >= 2; rig_first: num_rigs + 1 image offsets (None: one rig).  Returns (cameras, kr32, tree, rig_stats) stacked over rigs."""
    n = len(sizes_wh)
    rig_first = [0, n] if rig_first is None else [int(v) for v in rig_first]
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    stats = np.asarray(stats)
    outs = []
    for r in range(len(rig_first) - 1):
        a, b = rig_first[r], rig_first[r + 1]
        ks = [k for k, (i, j) in enumerate(pairs) if a <= i < b]
        assert all(a <= pairs[k][1] < b for k in ks)
        outs.append(estimate_rig([sizes_wh[i] for i in range(a, b)], [(pairs[k][0] - a, pairs[k][1] - a) for k in ks], [H[k] for k in ks],
                                 [stats[k] for k in ks], None if focals_in is None else np.asarray(focals_in, np.float64)[a:b]))
    return (np.concatenate([o["cameras"] for o in outs]), np.concatenate([o["kr32"] for o in outs]), np.concatenate([o["tree"] for o in outs]),
            np.stack([o["rig_stats"] for o in outs]))
