"""The reference's features matcher (M = its 特征点匹配 demo): BestOf2NearestMatcher1 matcher(false, 0.3f, 6, 6); matcher(features,
pairwise_matches) (M:307-308) up to where M:158 returns, plus the point gather of M:164-179, on the GPU (isx_match_features).
The 2-nearest-neighbour search is exact (Hamming distance over 32-byte descriptors); the FLANN LSH index of M:241-250 is not reproduced.
float32 descriptors of 1 .. 128 columns (the CV_32F depth of M:237) take isx_match_features_f32: an exact L2 search in place of the KD-tree
index, distances carried as float32 bits (DESIGN.md §8 "Features matcher, float descriptors")."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import IsxMat, as_mat, check

# the tiling of the search kernel (ISX_MATCH_* of include/imagestitch_hip.h): queries per block, train rows per LDS tile, train rows per
# work item; the row limits are the width of the packed key distance << 22 | row
QUERY_BLOCK, TRAIN_TILE, TRAIN_CHUNK = 128, 128, 256
MAX_ROWS, MAX_TOTAL_ROWS = 1 << 20, 1 << 22
# the float entry (ISX_MATCH_F32_*): the same query block, chunk plan and row limits; train rows per LDS tile and floats a row at the most
F32_TRAIN_TILE, F32_MAX_COLS = 32, 128


def _is_device(a):
    return hasattr(a, "is_cuda") and bool(a.is_cuda)


def _allocator(dev):
    """alloc(rows, cols, dtype): an uninitialised CUDA tensor on the torch device `dev`, or a NumPy array where dev is None"""
    if dev is None:
        return lambda r, c, dt: np.empty((r, c), dt)
    import torch
    return lambda r, c, dt: torch.empty((r, c), dtype=getattr(torch, np.dtype(dt).name), device=dev)


def _synchronize(stream, device):
    """Wait for the stream, or for the whole device where the stream is None or a raw handle."""
    if hasattr(stream, "synchronize"):
        stream.synchronize()
    else:
        import torch
        torch.cuda.synchronize(int(device))


def _mat(a):
    """as_mat, and a mat without rows for an array / tensor of shape (0, cols): its strides are whatever its history left, its data is never read."""
    if a.shape[0] == 0:
        dt = str(a.dtype).replace("torch.", "")
        key = (dt, 1)
        if len(a.shape) != 2 or key not in _lib._NP_TYPES:
            raise _lib.IsxError(2, "unsupported dtype/shape %s %s" % (dt, tuple(a.shape)))
        es = np.dtype(dt).itemsize
        return IsxMat(None, 0, int(a.shape[1]), _lib._NP_TYPES[key], int(a.shape[1]) * es, (a.device.index or 0) if _is_device(a) else -1)
    return as_mat(a)


def _mats(seq):
    return (IsxMat * max(len(seq), 1))(*[_mat(a) for a in seq])


def _call(entry, descriptors, pairs, match_conf, matches, counts, keypoints, img_sizes, points, knn, device, stream):
    n, npairs = len(descriptors), len(pairs)
    pij = (C.c_int * max(2 * npairs, 1))(*[int(v) for p in pairs for v in p])
    sizes = None
    if img_sizes is not None:
        sizes = (C.c_int * max(2 * n, 1))(*[int(v) for s in img_sizes for v in s])
    info = (C.c_int * 2)()
    ptr = getattr(stream, "cuda_stream", stream)
    check(getattr(_lib.load(), entry)(
        n, _mats(descriptors), None if keypoints is None else _mats(keypoints), sizes, npairs, pij, float(match_conf), _mats(matches),
        None if points is None else _mats(points), C.byref(as_mat(counts)), None if knn is None else _mats(knn), info, int(device),
        C.c_void_p(ptr or 0)))
    return info[0], info[1]


def match_features(descriptors, pairs, match_conf, matches, counts, keypoints=None, img_sizes=None, points=None, knn=None, device=0, stream=None):
    """isx_match_features on caller-allocated outputs.  descriptors: n_i x 32 uint8 arrays / CUDA tensors; pairs: (from, to) with from < to;
    matches: per pair an int32 mat of at least (n_from + n_to) x 3; counts: an int32 mat of at least 1 x len(pairs); keypoints / img_sizes:
    n_i x 2 float32 mats and (width, height) per image; points: per pair a float32 mat of at least (n_from + n_to) x 4; knn: 2 per pair,
    int32, at least n_query x 4.  Returns (pairs searched, kernel launches)."""
    return _call("isx_match_features", descriptors, pairs, match_conf, matches, counts, keypoints, img_sizes, points, knn, device, stream)


def match_features_f32(descriptors, pairs, match_conf, matches, counts, keypoints=None, img_sizes=None, points=None, knn=None, device=0, stream=None):
    """isx_match_features_f32 on caller-allocated outputs: match_features for n_i x cols float32 descriptors, 1 <= cols <= 128, one cols a
    call.  Column 2 of matches and columns 1 and 3 of knn carry the bits of the float32 L2 distance (view them as float32)."""
    return _call("isx_match_features_f32", descriptors, pairs, match_conf, matches, counts, keypoints, img_sizes, points, knn, device, stream)


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def entry_for(descriptors):
    """match_features or match_features_f32 by the descriptors' dtype: uint8 / float32, the same for every image (else ISX_ERR_TYPE)."""
    kinds = {_dtype_name(d) for d in descriptors}
    if kinds == {"float32"}:
        return match_features_f32
    if len(kinds) > 1 and "float32" in kinds:
        raise _lib.IsxError(2, "match: descriptors of mixed dtypes %s" % sorted(kinds))
    return match_features


class MatchesInfo:
    """detail::MatchesInfo as far as M:158 and M:164-179 fill it: src_img_idx, dst_img_idx, matches as an (m, 3) int32 array of (queryIdx,
    trainIdx, distance), src_points / dst_points as (m, 2) float32 arrays (None without keypoints), knn as the pair (1->2, 2->1) of
    n_query x 4 arrays (idx0, dist0, idx1, dist1) when asked for.  With float32 descriptors the distance columns carry the bits of the float32
    L2 distance; `distances` gives DMatch::distance as float32 for either kind (that view, or the Hamming column converted).  BestOf2NearestMatcher (homography.py) fills the rest: H (3 x 3 float64,
    None when empty), inliers_mask (uint8, one per match; empty below num_matches_thresh1), num_inliers and confidence; FeaturesMatcher
    leaves them at None, None, 0 and 0."""

    def __init__(self, src_img_idx, dst_img_idx, matches, src_points=None, dst_points=None, knn=None, float_distances=False):
        self.src_img_idx, self.dst_img_idx, self.matches = src_img_idx, dst_img_idx, matches
        self.src_points, self.dst_points, self.knn = src_points, dst_points, knn
        self.float_distances = bool(float_distances)
        self.H, self.inliers_mask, self.num_inliers, self.confidence = None, None, 0, 0.0

    @property
    def distances(self):
        """DMatch::distance of every match, float32: the float32 view of column 2 (float descriptors) or the Hamming distance converted."""
        col = self.matches[:, 2]
        if _is_device(col):
            import torch
            return col.contiguous().view(torch.float32) if self.float_distances else col.to(torch.float32)
        col = np.ascontiguousarray(col, np.int32)
        return col.view(np.float32) if self.float_distances else col.astype(np.float32)

    def dual(self):
        """The entry of the pair (to, from), as the reference's matcher derives it from (from, to): swapped image indices and points,
        matches with queryIdx and trainIdx swapped, H.inv() by np.linalg.inv.  Host arithmetic: the inverse is not bit-pinned."""
        m = self.matches.cpu().numpy() if _is_device(self.matches) else np.array(self.matches)
        d = MatchesInfo(self.dst_img_idx, self.src_img_idx, m[:, [1, 0, 2]], self.dst_points, self.src_points,
                        None if self.knn is None else (self.knn[1], self.knn[0]), self.float_distances)
        d.H = None if self.H is None else np.linalg.inv(self.H)
        d.inliers_mask, d.num_inliers, d.confidence = self.inliers_mask, self.num_inliers, self.confidence
        return d


class FeaturesMatcher:
    """BestOf2NearestMatcher1(try_use_gpu, match_conf, ...) (M:146-152, M:307) with the exact search OpenCV's own GpuMatcher runs."""

    def __init__(self, match_conf=0.3, device=0, stream=None):
        self.match_conf, self.device, self.stream = float(match_conf), device, stream
        self.last_info = None
        self.last_outputs = None      # of the last match(): pairs, counts; a subclass adds its mats (cameras.py reads them where they lie)

    @staticmethod
    def near_pairs(rows, mask=None):
        """M:126-135: i < j, both images with features, and mask[i, j] where a mask is given."""
        n = len(rows)
        if mask is not None:
            mask = np.asarray(mask)
            if mask.shape != (n, n):
                raise _lib.IsxError(1, "match: the mask is not %d x %d" % (n, n))
        return [(i, j) for i in range(n - 1) for j in range(i + 1, n) if rows[i] > 0 and rows[j] > 0 and (mask is None or mask[i, j])]

    def match(self, descriptors, keypoints=None, img_sizes=None, mask=None, knn=False):
        """matcher(features, pairwise_matches, mask) (M:123-144): one MatchesInfo per near pair, in the order of M:132-135.  descriptors:
        n_i x 32 uint8 NumPy arrays or CUDA tensors, or n_i x cols float32 ones (the L2 entry; mixed dtypes raise ISX_ERR_TYPE); keypoints: n_i x 2 float32 (pt.x, pt.y) with img_sizes = (width, height) per image.
        With CUDA descriptors the outputs are computed into CUDA tensors and returned as such."""
        rows = [int(d.shape[0]) for d in descriptors]
        entry = entry_for(descriptors)
        pairs = self.near_pairs(rows, mask)
        self.last_outputs = {"pairs": pairs}
        if not pairs:
            self.last_info = (0, 0)
            return []
        on_device = any(_is_device(d) for d in descriptors)
        alloc = _allocator("cuda:%d" % int(self.device) if on_device else None)
        cap = [rows[i] + rows[j] for i, j in pairs]
        m_all, counts = alloc(sum(cap), 3, np.int32), alloc(1, len(pairs), np.int32)
        p_all = alloc(sum(cap), 4, np.float32) if keypoints is not None else None
        at = np.concatenate([[0], np.cumsum(cap)])
        ms = [m_all[at[k]:at[k + 1]] for k in range(len(pairs))]
        ps = [p_all[at[k]:at[k + 1]] for k in range(len(pairs))] if p_all is not None else None
        ks = [alloc(rows[p[d]], 4, np.int32) for p in pairs for d in range(2)] if knn else None
        self.last_info = entry(descriptors, pairs, self.match_conf, ms, counts, keypoints, img_sizes, ps, ks, self.device, self.stream)
        self.last_outputs.update(counts=counts, matches=ms, keypoints=keypoints)      # where the later stages read them (adjuster.py)
        post = self._post_match(alloc, cap, ps, counts)
        if on_device:
            _synchronize(self.stream, self.device)
            cnt = counts.cpu().numpy()[0]
        else:
            cnt = counts[0]
        fill = post() if post is not None else None
        out = []
        for k, (i, j) in enumerate(pairs):
            c = int(cnt[k])
            pts = ps[k][:c] if ps is not None else None
            out.append(MatchesInfo(i, j, ms[k][:c], None if pts is None else pts[:, 0:2], None if pts is None else pts[:, 2:4],
                                   (ks[2 * k], ks[2 * k + 1]) if knn else None, entry is match_features_f32))
            if fill is not None:
                fill(out[-1], k, c)
        return out

    def _post_match(self, alloc, cap, points, counts):
        """What a subclass enqueues behind the matcher on the same mats, before the read-back: None, or a callable that - once the stream
        has been synchronised - returns fill(info, k, count)."""
        return None

    __call__ = match

    @staticmethod
    def release():
        """Return the scratch the matcher keeps per calling thread between calls (isx_match_release)."""
        check(_lib.load().isx_match_release())
