"""NumPy model of OpenCV 3.4.2's GraphCutSeamFinder(COST_COLOR_GRAD) (GraphCutSeamFinder::Impl::find + findInPair +
setGraphWeightsColorGrad), the specification of isx_graphcut_seam_find with ISX_GC_COST_COLOR_GRAD.  Everything that is not
the edge weight is COST_COLOR's and comes from tests/helpers/graphcut_np.py: pair order, gap 10, padded grid, terminal links, the +1000
penalty, the write-back over the roi, the maximal source side.  OpenCV parity is unpinned, as there.

    per image, over the whole tile: dx_ = |Sobel(src, CV_32F, 1, 0)|^2, dy_ = |Sobel(src, CV_32F, 0, 1)|^2 (3 x 3, three channels, the
        squared norm over the channels, BORDER_REFLECT_101 at the tile's own edges; a node outside a tile reads 0)
    edge p -> q:  grad = dx1(p) + dx1(q) + dx2(p) + dx2(q) + 1.f  (dy for a down edge),
                  weight = (|img1(p) - img2(p)|^2 + |img1(q) - img2(q)|^2) / grad + 1.f, + 1000.f when any of the four mask bytes is 0
On integer tiles every operand of the division is an exact integer below 2^24, so the weight is one correctly rounded float32 division
and one or two rounded float32 additions: a float32 >= 1, hence a multiple of 2^-23.  Capacities are weight * 2^23 as int64 (Q23), exact;
terminals 10000 * 2^23.  The maximum flow of that integer graph is exact and its maximal source side unique.

scipy's maximum_flow is int32 only, so the max-flow here is a plain Dinic on Python ints; it needs NumPy alone."""
import numpy as np

from . import graphcut_np as G

COST_COLOR, COST_COLOR_GRAD = 0, 1
SHIFT = 23
SCALE = 1 << SHIFT


def _reflect101(a, axis):
    """a with one more element at both ends of `axis`, BORDER_REFLECT_101; a dimension of size 1 reads index 0."""
    n = a.shape[axis]
    first = np.take(a, [1 if n > 1 else 0], axis=axis)
    last = np.take(a, [n - 2 if n > 1 else 0], axis=axis)
    return np.concatenate([first, a, last], axis=axis)


def sobel_sq(img):
    """(dx_, dy_) of a tile: int64 H x W, the squared norm over the three channels of Sobel(img, CV_32F, 1, 0) and (0, 1), 3 x 3, scale
    1, BORDER_REFLECT_101.  On integer tiles every value is an integer of at most 3 * 1020^2."""
    a = G.as_int_image(img)
    px = _reflect101(a, 1)
    diff = px[:, 2:] - px[:, :-2]                        # [-1 0 1] along x
    smooth = px[:, 2:] + px[:, :-2] + 2 * a              # [1 2 1] along x
    pd, ps = _reflect101(diff, 0), _reflect101(smooth, 0)
    dx = pd[2:] + pd[:-2] + 2 * diff                     # ... then [1 2 1] along y
    dy = ps[2:] - ps[:-2]                                # ... then [-1 0 1] along y
    return (dx * dx).sum(axis=2), (dy * dy).sum(axis=2)


def _q23(w):
    """float32 weights >= 1 as exact int64 multiples of 2^-23."""
    q = w.astype(np.float64) * float(SCALE)
    assert (w >= 1).all() and (q == np.floor(q)).all() and (q < 2.0 ** 42).all()    # the scaling is exact
    return q.astype(np.int64)


def pair_graph_grad(img1, img2, mask1, mask2, tl1, tl2, roi):
    """The COST_COLOR_GRAD sub-problem of one pair, in the layout of graphcut_np.pair_graph with every capacity in Q23."""
    s1, s2 = G._cut(G.as_int_image(img1), tl1, roi, (3,)), G._cut(G.as_int_image(img2), tl2, roi, (3,))
    m1, m2 = G._cut(np.asarray(mask1), tl1, roi, ()) != 0, G._cut(np.asarray(mask2), tl2, roi, ()) != 0
    gx1, gy1 = (G._cut(a, tl1, roi, ()) for a in sobel_sq(img1))
    gx2, gy2 = (G._cut(a, tl2, roi, ()) for a in sobel_sq(img2))
    d = ((s1 - s2) ** 2).sum(axis=2)
    ok = m1 & m2
    f32, one, pen = np.float32, np.float32(1), np.float32(G.PENALTY)

    def weights(dp, dq, gp, gq, okp, okq):
        grad = gp + gq + 1
        num = dp + dq
        assert grad.max(initial=0) < 1 << 24 and num.max(initial=0) < 1 << 24       # exact in float32
        w = (num.astype(f32) / grad.astype(f32)).astype(f32) + one
        return _q23(np.where(okp & okq, w, (w + pen).astype(f32)).astype(f32))

    gx, gy = gx1 + gx2, gy1 + gy2
    Hp, Wp = d.shape
    right, down = np.zeros((Hp, Wp), np.int64), np.zeros((Hp, Wp), np.int64)
    right[:, :-1] = weights(d[:, :-1], d[:, 1:], gx[:, :-1], gx[:, 1:], ok[:, :-1], ok[:, 1:])
    down[:-1, :] = weights(d[:-1, :], d[1:, :], gy[:-1, :], gy[1:, :], ok[:-1, :], ok[1:, :])
    src = np.where(m1 & ~m2, G.TERMINAL * SCALE, 0).astype(np.int64)
    snk = np.where(m2 & ~m1, G.TERMINAL * SCALE, 0).astype(np.int64)
    return dict(src=src, snk=snk, right=right, down=down, roi=roi)


def pair_graph(img1, img2, mask1, mask2, tl1, tl2, roi, cost_type=COST_COLOR_GRAD):
    if cost_type == COST_COLOR:
        return G.pair_graph(img1, img2, mask1, mask2, tl1, tl2, roi)
    return pair_graph_grad(img1, img2, mask1, mask2, tl1, tl2, roi)


def max_flow(g):
    """Exact maximum flow of a graph of any integer size (Dinic on Python ints).  Returns (flow value, certificate) as
    graphcut_np.max_flow does: residuals int64 Hp x Wp x 6, labels = the maximal source side."""
    Hp, Wp = g["src"].shape
    n = Hp * Wp
    S, T = n, n + 1
    u, v, c = G._edges(g)
    src, snk = g["src"].ravel(), g["snk"].ravel()
    si, ti = np.nonzero(src)[0], np.nonzero(snk)[0]
    # edge 2 k: tail -> head, edge 2 k + 1: head -> tail; a grid edge has its capacity both ways, a terminal link one way
    tail = u.tolist() + [S] * len(si) + ti.tolist()
    head = v.tolist() + si.tolist() + [T] * len(ti)
    fwd = c.tolist() + src[si].tolist() + snk[ti].tolist()
    ne, ns = len(u), len(si)
    to, cap = [0] * (2 * len(tail)), [0] * (2 * len(tail))
    adj = [[] for _ in range(n + 2)]
    for k, (a, b, w) in enumerate(zip(tail, head, fwd)):
        to[2 * k], to[2 * k + 1] = b, a
        cap[2 * k], cap[2 * k + 1] = w, (w if k < ne else 0)
        adj[a].append(2 * k)
        adj[b].append(2 * k + 1)
    flow = 0
    while True:
        level = [-1] * (n + 2)                           # distance to the sink over residual edges
        level[T] = 0
        frontier = [T]
        while frontier and level[S] < 0:
            nxt = []
            for b in frontier:
                lb = level[b] + 1
                for e in adj[b]:
                    a = to[e]
                    if level[a] < 0 and cap[e ^ 1] > 0:
                        level[a] = lb
                        nxt.append(a)
            frontier = nxt
        if level[S] < 0:
            break
        it = [0] * (n + 2)
        path = []                                        # edges of the current path from S
        a = S
        while True:
            if a == T:
                d = min(cap[e] for e in path)
                for e in path:
                    cap[e] -= d
                    cap[e ^ 1] += d
                flow += d
                k = next(i for i, e in enumerate(path) if cap[e] == 0)   # back to the tail of the first saturated edge
                a = to[path[k] ^ 1]
                del path[k:]
                continue
            la, ea, i = level[a] - 1, adj[a], it[a]
            while i < len(ea):
                e = ea[i]
                if cap[e] > 0 and level[to[e]] == la:
                    break
                i += 1
            it[a] = i
            if i < len(ea):
                path.append(ea[i])
                a = to[ea[i]]
            elif path:
                level[a] = -1                            # a dead end in this phase
                a = to[path.pop() ^ 1]
            else:
                break
    res = np.zeros((n, 6), np.int64)
    capa = np.array(cap[:2 * ne], dtype=np.int64).reshape(ne, 2) if ne else np.zeros((0, 2), np.int64)
    nr = Hp * (Wp - 1)
    res[u[:nr], 0] = capa[:nr, 0]; res[v[:nr], 1] = capa[:nr, 1]
    res[u[nr:], 2] = capa[nr:, 0]; res[v[nr:], 3] = capa[nr:, 1]
    res[si, 4] = np.array(cap[2 * ne:2 * (ne + ns):2], dtype=np.int64)
    res[ti, 5] = np.array(cap[2 * (ne + ns)::2], dtype=np.int64)
    res = res.reshape(Hp, Wp, 6)
    return flow, dict(residuals=res, labels=G.maximal_source_side(res))


def find(src, corners, masks, cost_type=COST_COLOR_GRAD, per_pair=None):
    """GraphCutSeamFinder(cost_type).find(src, corners, masks) with the maximal minimum cut: masks (uint8 arrays) edited in place.
    per_pair(i, j, graph, flow, certificate) is called after every pair's max-flow.  Flow values of COST_COLOR_GRAD are in Q23."""
    n = len(src)
    if n < 2:
        return masks
    for i in range(n):                                  # every float value is checked before the first pair writes
        G.as_int_image(src[i])
    sizes = [(np.asarray(a).shape[1], np.asarray(a).shape[0]) for a in src]
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = G.overlap_roi(corners[i], corners[j], sizes[i], sizes[j])
            if roi is None:
                continue
            g = pair_graph(src[i], src[j], masks[i], masks[j], corners[i], corners[j], roi, cost_type)
            flow, cert = max_flow(g)
            if per_pair is not None:
                per_pair(i, j, g, flow, cert)
            G.write_back(cert["labels"], masks[i], masks[j], corners[i], corners[j], roi)
    return masks
