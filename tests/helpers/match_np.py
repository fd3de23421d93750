"""The features matcher's specification in NumPy (isx_match_features, DESIGN.md §8 "Features matcher"): what the GPU is held to with
np.array_equal.

For a pair (from, to) of n x 32 uint8 descriptor arrays:
    skipped when either image has no row: count 0, nothing else
    1->2   with n_to >= 2: the two nearest rows of `to` by (Hamming distance, row) for every row q of `from`; accepted when
           float32(d0) < k * float32(d1), k = float32(1) - float32(match_conf), the product one rounded float32 multiply; appended as
           (q, row0, d0) in order of q
    2->1   the same with the roles swapped (n_from >= 2); appended as (row0, q, d0) in order of q unless 1->2 accepted (row0, q)
    points row r = (kp_from[queryIdx] - size_from * 0.5f, kp_to[trainIdx] - size_to * 0.5f) in float32
    knn    per direction n_query x 4: row0, d0, row1, d1; -1, -1 where there is no such neighbour
An accepted match has d0 < k d1 <= d1, a unique nearest neighbour: the (distance, row) order of ties shows in knn only."""
import numpy as np

F32 = np.float32
_POP = np.array([bin(v).count("1") for v in range(256)], np.uint8)


BLOCK_BYTES = 32 << 20      # the largest temporary of hamming / knn2: a block of XORed rows (and its popcounts, a second one of this size)
_Q_BLOCK = 256


def _train_block(nq):
    return max(1, BLOCK_BYTES // (32 * max(1, min(nq, _Q_BLOCK))))


def _block(q, t):
    """(len(q), len(t)) int32 distances of one block: the XOR is the temporary BLOCK_BYTES bounds."""
    if hasattr(np, "bitwise_count"):                       # popcounts of 4 x 64 bits a row: the same integers, an eighth of the lookups
        x = q.view(np.uint64)[:, None, :] ^ t.view(np.uint64)[None, :, :]
        return np.bitwise_count(x).sum(axis=2, dtype=np.int32)
    return _POP[q[:, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)


def _rows(a):
    return np.ascontiguousarray(np.asarray(a, np.uint8).reshape(-1, 32))


def hamming(q, t):
    """(nq, nt) int32 Hamming distances between the rows of two n x 32 uint8 arrays, in blocks over both."""
    q, t = _rows(q), _rows(t)
    out = np.zeros((q.shape[0], t.shape[0]), np.int32)
    step = _train_block(q.shape[0])
    for r0 in range(0, q.shape[0], _Q_BLOCK):
        for c0 in range(0, t.shape[0], step):
            out[r0:r0 + _Q_BLOCK, c0:c0 + step] = _block(q[r0:r0 + _Q_BLOCK], t[c0:c0 + step])
    return out


def knn2(q, t):
    """n_query x 4 int32: (row0, d0, row1, d1), the two nearest rows of t by (distance, row); -1, -1 where there is none.  Blocked over
    queries and train rows: a block's distances become keys distance << 32 | row, unique per query, and the two smallest of a block are
    merged with the two kept so far - the order of (distance, row) whatever the blocking, as a stable sort of the whole row gives it."""
    q, t = _rows(q), _rows(t)
    nq, nt = q.shape[0], t.shape[0]
    out = np.full((nq, 4), -1, np.int32)
    if nq == 0 or nt == 0:
        return out
    none = np.int64(1) << 62
    step = _train_block(nq)
    for r0 in range(0, nq, _Q_BLOCK):
        qb = q[r0:r0 + _Q_BLOCK]
        best = np.full((qb.shape[0], 2), none, np.int64)
        for c0 in range(0, nt, step):
            d = _block(qb, t[c0:c0 + step])
            keys = (d.astype(np.int64) << 32) | np.arange(c0, c0 + d.shape[1], dtype=np.int64)[None, :]
            if keys.shape[1] > 2:
                keys = np.partition(keys, 1, axis=1)[:, :2]
            best = np.sort(np.concatenate([best, keys], axis=1), axis=1)[:, :2]
        for k in range(2):
            has = best[:, k] != none
            out[r0:r0 + _Q_BLOCK, 2 * k] = np.where(has, best[:, k] & 0xFFFFFFFF, -1)
            out[r0:r0 + _Q_BLOCK, 2 * k + 1] = np.where(has, best[:, k] >> 32, -1)
    return out


def ratio_k(match_conf):
    return F32(1.0) - F32(match_conf)


def accepted(knn, match_conf):
    """Boolean per query: has two neighbours and float32(d0) < k * float32(d1)."""
    k = ratio_k(match_conf)
    prod = (k * knn[:, 3].astype(F32)).astype(F32)
    return (knn[:, 2] >= 0) & (knn[:, 1].astype(F32) < prod)


def match_pair(a, b, match_conf):
    """(matches (m, 3) int32, knn 1->2, knn 2->1, kinds) of one pair; kinds = (mutual, 1->2 only, 2->1 only) counts of accepted matches."""
    a, b = np.asarray(a, np.uint8).reshape(-1, 32), np.asarray(b, np.uint8).reshape(-1, 32)
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


def points_of(matches, kp_from, kp_to, size_from, size_to):
    """(m, 4) float32: src.x, src.y, dst.x, dst.y."""
    out = np.zeros((matches.shape[0], 4), F32)
    if matches.shape[0]:
        hf = np.array([F32(size_from[0]) * F32(0.5), F32(size_from[1]) * F32(0.5)], F32)
        ht = np.array([F32(size_to[0]) * F32(0.5), F32(size_to[1]) * F32(0.5)], F32)
        out[:, 0:2] = np.asarray(kp_from, F32)[matches[:, 0]] - hf
        out[:, 2:4] = np.asarray(kp_to, F32)[matches[:, 1]] - ht
    return out


def match_model(descriptors, pairs, match_conf, keypoints=None, img_sizes=None):
    """One dict per pair: count, matches, knn (the two directions), kinds and - with keypoints - points."""
    out = []
    for i, j in pairs:
        m, k12, k21, kinds = match_pair(descriptors[i], descriptors[j], match_conf)
        rec = dict(count=m.shape[0], matches=m, knn=(k12, k21), kinds=kinds, skipped=len(descriptors[i]) == 0 or len(descriptors[j]) == 0)
        if keypoints is not None:
            rec["points"] = points_of(m, keypoints[i], keypoints[j], img_sizes[i], img_sizes[j])
        out.append(rec)
    return out


def near_pairs(rows, mask=None):
    n = len(rows)
    return [(i, j) for i in range(n - 1) for j in range(i + 1, n) if rows[i] > 0 and rows[j] > 0 and (mask is None or mask[i][j])]
