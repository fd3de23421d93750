"""NumPy model of OpenCV 3.4.2's GraphCutSeamFinder(COST_COLOR) (PairwiseSeamFinder::run + GraphCutSeamFinder::Impl::findInPair +
setGraphWeightsColor), the specification of isx_graphcut_seam_find (DESIGN.md §8 "graph-cut seam finder").  OpenCV parity is unpinned:
OpenCV is not installed where this was written, and its Boykov-Kolmogorov max-flow picks one of the minimum cuts by its search order.
This model takes the MAXIMAL source side instead (every node from which the sink cannot be reached in the residual graph of a maximum
flow), which is unique: every exact max-flow gives the same set.

    find(src, corners, masks): for i < j (outer i, inner j) with a non-empty overlapRoi, on the masks as the earlier pairs left them:
        padded grid (roi.h + 2 gap) x (roi.w + 2 gap), gap = 10; a pixel outside a tile reads image 0 and mask 0
        terminal links: mask1 only -> source 10000; mask2 only -> sink 10000; both or neither -> none
        right / down edges: w = |img1(p) - img2(p)|^2 + |img1(q) - img2(q)|^2 + 1 (+ 1000 when any of the four mask bytes is 0)
        write-back over the roi: source side and mask1 set -> mask2 = 0; otherwise mask2 set -> mask1 = 0
The max-flow is scipy.sparse.csgraph.maximum_flow (Dinic), exact in integers; graph construction and the certificate checks need NumPy
only."""
import numpy as np

GAP = 10
TERMINAL = 10000
PENALTY = 1000


class Unsupported(ValueError):
    """A CV_32FC3 value that is not an integer in [0, 255]: the capacities would not be exact integers."""


def overlap_roi(tl1, tl2, sz1, sz2):
    """cv::detail::overlapRoi: (x, y, w, h) or None.  sz = (width, height)."""
    x_tl, y_tl = max(tl1[0], tl2[0]), max(tl1[1], tl2[1])
    x_br, y_br = min(tl1[0] + sz1[0], tl2[0] + sz2[0]), min(tl1[1] + sz1[1], tl2[1] + sz2[1])
    if x_tl < x_br and y_tl < y_br:
        return x_tl, y_tl, x_br - x_tl, y_br - y_tl
    return None


def as_int_image(img):
    """int64 HxWx3 of a CV_8UC3 or CV_32FC3 tile; raises Unsupported for a float that is not an integer in [0, 255]."""
    a = np.asarray(img)
    if a.dtype == np.uint8:
        return a.astype(np.int64)
    f = a.astype(np.float32)
    if not (np.all(f >= 0) and np.all(f <= 255) and np.all(f == np.floor(f))):
        raise Unsupported("CV_32FC3 values must be integers in [0, 255]")
    return f.astype(np.int64)


def _cut(a, tl, roi, fill_shape):
    """The padded grid's window of a tile (rows / cols -gap .. roi + gap relative to the roi), zero outside the tile."""
    x0, y0, w, h = roi
    Hp, Wp = h + 2 * GAP, w + 2 * GAP
    out = np.zeros((Hp, Wp) + fill_shape, a.dtype)
    oy, ox = y0 - tl[1] - GAP, x0 - tl[0] - GAP          # tile coordinates of the grid's (0, 0)
    ys, xs = max(0, -oy), max(0, -ox)
    ye, xe = min(Hp, a.shape[0] - oy), min(Wp, a.shape[1] - ox)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[oy + ys:oy + ye, ox + xs:ox + xe]
    return out


def pair_graph(img1, img2, mask1, mask2, tl1, tl2, roi):
    """The sub-problem of one pair: dict with int64 arrays over the padded grid: src, snk (terminal capacities), right (edge (y, x) -
    (y, x + 1), 0 in the last column), down (edge (y, x) - (y + 1, x), 0 in the last row)."""
    s1, s2 = _cut(as_int_image(img1), tl1, roi, (3,)), _cut(as_int_image(img2), tl2, roi, (3,))
    m1, m2 = _cut(np.asarray(mask1), tl1, roi, ()) != 0, _cut(np.asarray(mask2), tl2, roi, ()) != 0
    d = ((s1 - s2) ** 2).sum(axis=2)                    # normL2 of Point3f: the squared distance
    ok = m1 & m2
    Hp, Wp = d.shape
    right = np.zeros((Hp, Wp), np.int64)
    down = np.zeros((Hp, Wp), np.int64)
    right[:, :-1] = d[:, :-1] + d[:, 1:] + 1 + PENALTY * ~(ok[:, :-1] & ok[:, 1:])
    down[:-1, :] = d[:-1, :] + d[1:, :] + 1 + PENALTY * ~(ok[:-1, :] & ok[1:, :])
    src = np.where(m1 & ~m2, TERMINAL, 0).astype(np.int64)
    snk = np.where(m2 & ~m1, TERMINAL, 0).astype(np.int64)
    return dict(src=src, snk=snk, right=right, down=down, roi=roi)


def _edges(g):
    """(u, v, capacity) of every grid edge with capacity > 0, once per undirected edge."""
    Hp, Wp = g["src"].shape
    idx = np.arange(Hp * Wp).reshape(Hp, Wp)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    c = np.concatenate([g["right"][:, :-1].ravel(), g["down"][:-1, :].ravel()])
    return u, v, c


def max_flow(g):
    """Exact maximum flow (scipy Dinic).  Returns (flow value, certificate) - the certificate in the layout isx_graphcut_seam_find_pair
    returns: residuals int64 Hp x Wp x 6 = (to the right, to the left, down, up, from the source, to the sink), labels = maximal source
    side (1 = source)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import maximum_flow
    Hp, Wp = g["src"].shape
    n = Hp * Wp
    S, T = n, n + 1
    u, v, c = _edges(g)
    src, snk = g["src"].ravel(), g["snk"].ravel()
    si, ti = np.nonzero(src)[0], np.nonzero(snk)[0]
    rows = np.concatenate([u, v, np.full(len(si), S), ti])
    cols = np.concatenate([v, u, si, np.full(len(ti), T)])
    caps = np.concatenate([c, c, src[si], snk[ti]])
    A = sp.csr_matrix((caps.astype(np.int32), (rows, cols)), shape=(n + 2, n + 2))
    r = maximum_flow(A, S, T, method="dinic")
    F = r.flow.tocsr()
    def at(rows, cols):                                  # F[rows, cols] as int64; an empty index pair (no terminal of that kind) gives a matrix, not an array
        return np.asarray(F[rows, cols]).ravel().astype(np.int64) if len(rows) else np.zeros(0, np.int64)
    fe = at(u, v)                                        # net flow u -> v of each grid edge
    fs = at(np.full(len(si), S), si)
    ft = at(ti, np.full(len(ti), T))
    res = np.zeros((n, 6), np.int64)
    nr = Hp * (Wp - 1)
    ru, rv = c - fe, c + fe                              # residual u -> v and v -> u
    res[u[:nr], 0] = ru[:nr]; res[v[:nr], 1] = rv[:nr]
    res[u[nr:], 2] = ru[nr:]; res[v[nr:], 3] = rv[nr:]
    res[si, 4] = src[si] - fs
    res[ti, 5] = snk[ti] - ft
    res = res.reshape(Hp, Wp, 6)
    return int(r.flow_value), dict(residuals=res, labels=maximal_source_side(res))


def reaches_sink(res):
    """bool Hp x Wp: the nodes from which the sink can be reached over residual edges (a BFS from the sink over reverse residual
    edges), from the certificate's residuals alone.  scipy's BFS when it is installed, a plain one otherwise."""
    Hp, Wp, _ = res.shape
    n = Hp * Wp
    idx = np.arange(n).reshape(Hp, Wp)
    # reverse residual edges v -> u for every residual u -> v; node n is the sink
    us = [idx[:, :-1][res[:, :-1, 0] > 0], idx[:, 1:][res[:, 1:, 1] > 0], idx[:-1, :][res[:-1, :, 2] > 0], idx[1:, :][res[1:, :, 3] > 0]]
    vs = [idx[:, 1:][res[:, :-1, 0] > 0], idx[:, :-1][res[:, 1:, 1] > 0], idx[1:, :][res[:-1, :, 2] > 0], idx[:-1, :][res[1:, :, 3] > 0]]
    ts = idx[res[:, :, 5] > 0]
    u = np.concatenate(us + [ts]); v = np.concatenate(vs + [np.full(len(ts), n)])
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import breadth_first_order
    except ImportError:
        sp = None
    seen = np.zeros(n + 1, bool)
    if sp is not None:
        A = sp.csr_matrix((np.ones(len(u), np.int8), (v, u)), shape=(n + 1, n + 1))
        seen[breadth_first_order(A, n, directed=True, return_predecessors=False)] = True
    else:
        import collections
        order = np.argsort(v, kind="stable")
        us_, vs_ = u[order], v[order]
        start = np.searchsorted(vs_, np.arange(n + 2))
        seen[n] = True
        q = collections.deque([n])
        while q:
            a = q.popleft()
            for b in us_[start[a]:start[a + 1]]:
                if not seen[b]:
                    seen[b] = True
                    q.append(b)
    return seen[:n].reshape(Hp, Wp)


def maximal_source_side(res):
    """uint8 Hp x Wp: 1 where the sink cannot be reached (the maximal source side of a maximum flow's residual graph)."""
    return (~reaches_sink(res)).astype(np.uint8)


def minimal_source_side(g, res):
    """uint8 Hp x Wp: the nodes the source reaches over residual edges (the minimal source side)."""
    import collections
    Hp, Wp = g["src"].shape
    seen = res[:, :, 4] > 0
    q = collections.deque(zip(*np.nonzero(seen)))
    while q:
        y, x = q.popleft()
        for dy, dx, k in ((0, 1, 0), (0, -1, 1), (1, 0, 2), (-1, 0, 3)):
            yy, xx = y + dy, x + dx
            if 0 <= yy < Hp and 0 <= xx < Wp and not seen[yy, xx] and res[y, x, k] > 0:
                seen[yy, xx] = True
                q.append((yy, xx))
    return seen.astype(np.uint8)


def cut_capacity(g, labels):
    """Capacity of the cut (source side = labels != 0) in the graph g."""
    s = labels != 0
    cap = int(g["src"][~s].sum()) + int(g["snk"][s].sum())
    cap += int(g["right"][:, :-1][s[:, :-1] != s[:, 1:]].sum())
    cap += int(g["down"][:-1, :][s[:-1, :] != s[1:, :]].sum())
    return cap


def check_certificate(g, flow, res, labels):
    """Asserts that (flow, residuals, labels) prove a maximum flow of g and its maximal minimum cut (NumPy only)."""
    res = np.asarray(res, np.int64)
    labels = np.asarray(labels)
    Hp, Wp = g["src"].shape
    assert res.shape == (Hp, Wp, 6) and labels.shape == (Hp, Wp)
    assert (res >= 0).all()
    # r(u -> v) + r(v -> u) = 2 w on every grid edge, and 0 where there is no edge
    assert np.array_equal(res[:, :-1, 0] + res[:, 1:, 1], 2 * g["right"][:, :-1])
    assert np.array_equal(res[:-1, :, 2] + res[1:, :, 3], 2 * g["down"][:-1, :])
    assert not res[:, -1, 0].any() and not res[:, 0, 1].any() and not res[-1, :, 2].any() and not res[0, :, 3].any()
    assert (res[:, :, 4] <= g["src"]).all() and (res[:, :, 5] <= g["snk"]).all()
    # excess from the residuals: flow in from the source and the neighbours, minus flow out
    fr = g["right"] - res[:, :, 0]                      # net flow to the right
    fd = g["down"] - res[:, :, 2]
    ex = (g["src"] - res[:, :, 4]) - (g["snk"] - res[:, :, 5]) - fr - fd
    ex[:, 1:] += fr[:, :-1]
    ex[1:, :] += fd[:-1, :]
    assert (ex >= 0).all()
    reach = reaches_sink(res)
    assert not ex[reach].any()
    assert np.array_equal(labels.astype(bool), ~reach)
    s = ~reach
    # no residual edge from the source side into the rest (incl. the source's own links)
    assert not (res[:, :-1, 0][s[:, :-1] & ~s[:, 1:]]).any() and not (res[:, 1:, 1][s[:, 1:] & ~s[:, :-1]]).any()
    assert not (res[:-1, :, 2][s[:-1, :] & ~s[1:, :]]).any() and not (res[1:, :, 3][s[1:, :] & ~s[:-1, :]]).any()
    assert not res[:, :, 4][~s].any()
    assert flow == int((g["snk"] - res[:, :, 5]).sum()) == cut_capacity(g, labels)


def write_back(labels, mask1, mask2, tl1, tl2, roi):
    """findInPair's write-back over the roi (not the gap), in place."""
    x0, y0, w, h = roi
    src = labels[GAP:GAP + h, GAP:GAP + w] != 0
    a = mask1[y0 - tl1[1]:y0 - tl1[1] + h, x0 - tl1[0]:x0 - tl1[0] + w]
    b = mask2[y0 - tl2[1]:y0 - tl2[1] + h, x0 - tl2[0]:x0 - tl2[0] + w]
    clear2 = src & (a != 0)
    clear1 = ~src & (b != 0)
    b[clear2] = 0
    a[clear1] = 0


def find(src, corners, masks, per_pair=None):
    """GraphCutSeamFinder(COST_COLOR).find(src, corners, masks) with the maximal minimum cut: masks (uint8 arrays) edited in place.
    per_pair(i, j, graph, flow, certificate) is called after every pair's max-flow."""
    n = len(src)
    if n < 2:
        return masks
    for i in range(n):                                  # every float value is checked before the first pair writes
        as_int_image(src[i])
    sizes = [(np.asarray(a).shape[1], np.asarray(a).shape[0]) for a in src]
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = overlap_roi(corners[i], corners[j], sizes[i], sizes[j])
            if roi is None:
                continue
            g = pair_graph(src[i], src[j], masks[i], masks[j], corners[i], corners[j], roi)
            flow, cert = max_flow(g)
            if per_pair is not None:
                per_pair(i, j, g, flow, cert)
            write_back(cert["labels"], masks[i], masks[j], corners[i], corners[j], roi)
    return masks
