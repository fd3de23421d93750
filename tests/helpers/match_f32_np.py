"""The float features matcher's specification in NumPy (isx_match_features_f32, DESIGN.md §8 "Features matcher, float descriptors"): what
the GPU is held to with np.array_equal.  Everything after the search - the 1->2 / 2->1 order, the de-duplication, the point gather - is
tests/helpers/match_np.py's.

For a pair (from, to) of n x cols float32 descriptor arrays, 1 <= cols <= 128:
    s(q, t)  float32, s = 0; for c = 0 .. cols - 1 in that order e = a[c] - b[c], s = s + e * e, every operation rounded on its own (no
             FMA); an s that is not finite (overflow, NaN from non-finite input) becomes +inf.  s >= +0, so its bits order as an integer.
    knn      per query the two smallest train rows by (s, row); n_query x 4 int32: row0, bits(d0), row1, bits(d1) with d = sqrt(s),
             correctly rounded; -1, -1 where there is no such neighbour.  Two distinct s can round to one d: the order is by s.
    ratio    d0 < k * d1, k = float32(1) - float32(match_conf), the product one rounded float32 multiply.
    matches  (queryIdx, trainIdx, bits(d0)) int32, in match_np's order.
An accepted match has d0 < k d1 <= d1, hence s0 < s1: a unique nearest neighbour."""
import numpy as np

from . import match_np as M

F32 = np.float32
BLOCK_ELEMS = 4 << 20       # the largest temporary of sqdist: a block of (queries, train rows) float32
_Q_BLOCK = 256


def _rows(a):
    a = np.asarray(a, F32)
    return np.ascontiguousarray(a if a.ndim == 2 else a.reshape(-1, 1))


def sqdist(q, t):
    """(nq, nt) float32 squared distances in the stated order; not finite -> +inf."""
    q, t = _rows(q), _rows(t)
    s = np.zeros((q.shape[0], t.shape[0]), F32)
    with np.errstate(all="ignore"):
        for c in range(q.shape[1]):
            e = q[:, c, None] - t[None, :, c]
            s = s + e * e
        s[~np.isfinite(s)] = np.inf
    return s


def bits(x):
    return np.asarray(x, F32).view(np.int32)


def from_bits(x):
    return np.ascontiguousarray(np.asarray(x, np.int32)).view(F32)


def knn2(q, t):
    """n_query x 4 int32: (row0, bits(d0), row1, bits(d1)), the two nearest rows of t by (s, row); -1, -1 where there is none.  Blocked like
    match_np.knn2, with keys bits(s) << 32 | row."""
    q, t = _rows(q), _rows(t)
    nq, nt = q.shape[0], t.shape[0]
    out = np.full((nq, 4), -1, np.int32)
    if nq == 0 or nt == 0:
        return out
    none = np.iinfo(np.int64).max                  # above bits(+inf) << 32 | row
    for r0 in range(0, nq, _Q_BLOCK):
        qb = q[r0:r0 + _Q_BLOCK]
        step = max(1, BLOCK_ELEMS // qb.shape[0])
        best = np.full((qb.shape[0], 2), none, np.int64)
        for c0 in range(0, nt, step):
            s = sqdist(qb, t[c0:c0 + step])
            keys = (s.view(np.int32).astype(np.int64) << 32) | np.arange(c0, c0 + s.shape[1], dtype=np.int64)[None, :]
            if keys.shape[1] > 2:
                keys = np.partition(keys, 1, axis=1)[:, :2]
            best = np.sort(np.concatenate([best, keys], axis=1), axis=1)[:, :2]
        for k in range(2):
            has = best[:, k] != none
            sk = (best[:, k] >> 32).astype(np.int32).view(F32)
            with np.errstate(all="ignore"):
                d = np.sqrt(np.where(has, sk, F32(0)).astype(F32))
            out[r0:r0 + _Q_BLOCK, 2 * k] = np.where(has, best[:, k] & 0xFFFFFFFF, -1)
            out[r0:r0 + _Q_BLOCK, 2 * k + 1] = np.where(has, d.view(np.int32), -1)
    return out


def accepted(knn, match_conf):
    """Boolean per query: has two neighbours and d0 < k * d1 in float32."""
    k = M.ratio_k(match_conf)
    d0, d1 = from_bits(knn[:, 1]), from_bits(knn[:, 3])
    has = knn[:, 2] >= 0
    with np.errstate(all="ignore"):
        prod = (k * np.where(has, d1, F32(0))).astype(F32)
        return has & (np.where(has, d0, F32(0)) < prod)


def match_pair(a, b, match_conf):
    """(matches (m, 3) int32, knn 1->2, knn 2->1, kinds) of one pair, as match_np.match_pair."""
    a, b = _rows(a), _rows(b)
    k12, k21 = knn2(a, b), knn2(b, a)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros((0, 3), np.int32), k12, k21, (0, 0, 0)
    ok12, ok21 = accepted(k12, match_conf), accepted(k21, match_conf)
    rows = [(q, k12[q, 0], k12[q, 1]) for q in np.flatnonzero(ok12)]
    both = 0
    for q in np.flatnonzero(ok21):
        r0 = k21[q, 0]
        if ok12[r0] and k12[r0, 0] == q:
            both += 1
        else:
            rows.append((r0, q, k21[q, 1]))
    m = np.array(rows, np.int32).reshape(-1, 3)
    return m, k12, k21, (both, int(ok12.sum()) - both, int(ok21.sum()) - both)


def match_model(descriptors, pairs, match_conf, keypoints=None, img_sizes=None):
    """One dict per pair: count, matches, knn (the two directions), kinds, skipped and - with keypoints - points."""
    out = []
    for i, j in pairs:
        m, k12, k21, kinds = match_pair(descriptors[i], descriptors[j], match_conf)
        rec = dict(count=m.shape[0], matches=m, knn=(k12, k21), kinds=kinds, skipped=len(descriptors[i]) == 0 or len(descriptors[j]) == 0)
        if keypoints is not None:
            rec["points"] = M.points_of(m, keypoints[i], keypoints[j], img_sizes[i], img_sizes[j])
        out.append(rec)
    return out


near_pairs = M.near_pairs
