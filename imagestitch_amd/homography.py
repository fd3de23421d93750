"""The second half of the reference's BestOf2NearestMatcher::match (R = its 计算单应性矩阵 demo, R:836-909): findHomography(RANSAC), the inlier
mask, num_inliers, confidence and the second run on the inliers, on the GPU (isx_find_homography, DESIGN.md §8 "Homography").  The
Levenberg-Marquardt polish of R:672 is opt-in (refine=True: isx_find_homography_lm, four more stats columns); cv::eigen, cv::RNG,
haveCollinearPoints and cvRound - and, for the polish, OpenCV's mulTransposed, gemm, norm, dot, solve and invert - are restated, so parity
with OpenCV is not pinned (tests/helpers/homography_np.py and homography_lm_np.py are the specification)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import as_mat, check
from .matcher import FeaturesMatcher, _is_device, _mats

# stats columns and status bits (ISX_HOMOGRAPHY_* of include/imagestitch_hip.h); hypotheses per chunk of the kernel
STATUS, NUM_INLIERS, ITERS1, WIN1, ITERS2, WIN2, ATTEMPTS = range(7)
LM_RET1, LM_NFJ1, LM_RET2, LM_NFJ2 = 8, 9, 10, 11       # refine only: run()'s return value and nfJ of the LM polish, per pass
ST_H, ST_PASS2, ST_PASS2_FAILED, ST_CLAMPED, ST_DEGENERATE = 1, 2, 4, 8, 16
CHUNK = 64


def find_homography(points, counts, H, inlier_masks, stats, conf, reproj_thresh=3.0, max_iters=2000, confidence=0.995, num_matches_thresh1=6,
                    num_matches_thresh2=6, device=0, stream=None, refine=False, lm_max_iters=10):
    """isx_find_homography - with refine, isx_find_homography_lm: the LM polish of R:672 with lm_max_iters (1 .. 1000) iterations at the
    most, and stats of at least len(points) x 12 - on caller-allocated outputs.  points: per pair the matcher's float32 mat (rows x >= 4); counts: its int32 mat of
    at least 1 x len(points), read on the device when it lives there; H: float64, at least 3 len(points) x 3; inlier_masks: per pair uint8,
    at least count x 1; stats: int32, at least len(points) x 8; conf: float64, at least 1 x len(points).  NumPy arrays or CUDA tensors.
    Returns (pairs processed, kernel launches)."""
    npairs = len(points)
    if len(inlier_masks) != npairs:
        raise _lib.IsxError(1, "find_homography: points and inlier_masks differ in length")
    info = (C.c_int * 2)()
    ptr = getattr(stream, "cuda_stream", stream)
    head = (npairs, _mats(points), C.byref(as_mat(counts)), float(reproj_thresh), int(max_iters), float(confidence), int(num_matches_thresh1),
            int(num_matches_thresh2))
    tail = (C.byref(as_mat(H)), _mats(inlier_masks), C.byref(as_mat(stats)), C.byref(as_mat(conf)), info, int(device), C.c_void_p(ptr or 0))
    if refine:
        check(_lib.load().isx_find_homography_lm(*head, int(lm_max_iters), *tail))
    else:
        check(_lib.load().isx_find_homography(*head, *tail))
    return info[0], info[1]


def release():
    """Return the scratch isx_find_homography keeps per calling thread between calls (isx_homography_release)."""
    check(_lib.load().isx_homography_release())


class BestOf2NearestMatcher(FeaturesMatcher):
    """BestOf2NearestMatcher1(try_use_gpu, match_conf, num_matches_thresh1, num_matches_thresh2) (R:781-782, R:830-911): FeaturesMatcher's
    matches, then H (3 x 3 float64, None when empty), inliers_mask, num_inliers and confidence of every pair.  match() needs keypoints.
    refine: H is polished by Levenberg-Marquardt as at R:672 (lm_max_iters: 10 there) and MatchesInfo.stats has 12 columns."""

    def __init__(self, match_conf=0.3, num_matches_thresh1=6, num_matches_thresh2=6, device=0, stream=None, reproj_thresh=3.0, max_iters=2000,
                 confidence=0.995, refine=False, lm_max_iters=10):
        super().__init__(match_conf, device, stream)
        self.refine, self.lm_max_iters = bool(refine), int(lm_max_iters)
        self.num_matches_thresh1, self.num_matches_thresh2 = int(num_matches_thresh1), int(num_matches_thresh2)
        self.reproj_thresh, self.max_iters, self.confidence = float(reproj_thresh), int(max_iters), float(confidence)
        self.last_homography_info = None

    def match(self, descriptors, keypoints=None, img_sizes=None, mask=None, knn=False):
        """matcher(features, pairwise_matches, mask) with R:830-911 per near pair.  With CUDA descriptors both entries run on device mats, the
        second reading the first's points and counts where they lie; the one read-back follows both."""
        if keypoints is None or img_sizes is None:
            raise _lib.IsxError(1, "BestOf2NearestMatcher: the homography needs keypoints and img_sizes")
        return super().match(descriptors, keypoints, img_sizes, mask, knn)

    __call__ = match

    def _post_match(self, alloc, cap, points, counts):
        n = len(points)
        H, stats, conf = alloc(3 * n, 3, np.float64), alloc(n, 12 if self.refine else 8, np.int32), alloc(1, n, np.float64)
        m_all = alloc(max(sum(cap), 1), 1, np.uint8)
        at = np.concatenate([[0], np.cumsum(cap)])
        masks = [m_all[at[k]:at[k + 1]] for k in range(n)]
        self.last_homography_info = find_homography(points, counts, H, masks, stats, conf, self.reproj_thresh, self.max_iters, self.confidence,
                                                    self.num_matches_thresh1, self.num_matches_thresh2, self.device, self.stream, self.refine,
                                                    self.lm_max_iters)
        self.last_outputs.update(H=H, stats=stats, conf=conf, masks=masks)      # where the next stages read them (cameras.py, adjuster.py)

        def read_back():
            Hh, sh, ch = (a.cpu().numpy() if _is_device(a) else a for a in (H, stats, conf))

            def fill(info, k, count):
                st = int(sh[k, STATUS])
                info.H = Hh[3 * k:3 * k + 3].copy() if st & ST_H else None
                info.num_inliers, info.confidence = int(sh[k, NUM_INLIERS]), float(ch[0, k])
                info.inliers_mask = masks[k][:count if count >= self.num_matches_thresh1 else 0, 0]      # R:836 returns before the mask exists
                info.status, info.stats = st, sh[k].copy()
            return fill
        return read_back

    @staticmethod
    def release():
        """Return the scratch both stages keep per calling thread (isx_match_release, isx_homography_release)."""
        check(_lib.load().isx_match_release())
        check(_lib.load().isx_homography_release())
