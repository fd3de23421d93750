"""NumPy model of OpenCV 3.4.2's VoronoiSeamFinder (PairwiseSeamFinder::run + VoronoiSeamFinder::findInPair), the specification of
isx_voronoi_seam_find (DESIGN.md §8 "Voronoi seam finder").  OpenCV parity is unpinned, as for the rest of the blend half: OpenCV is not
installed where this was written; the distance transform is the oracle's orc_distance_transform_l1, the restatement of
distanceTransform(DIST_L1, 3) that FeatherBlender's weight maps are already checked against.

    find(sizes, corners, masks): for i < j (outer i, inner j) with a non-empty overlapRoi, on the masks as the earlier pairs left them:
        1. submask_k: (roi.h + 2 gap) x (roi.w + 2 gap), gap = 10: the window of mask k around the roi, 0 outside tile k
        2. collision = (submask1 != 0) & (submask2 != 0); unique_k = submask_k with the collision cells set to 0
        3. dist_k = distanceTransform(unique_k == 0, DIST_L1, 3): the source is 255 where unique_k is 0, so dist_k is the city-block
           distance to the nearest cell only tile k covers - or INIT_DIST0 / 65536 + the distance to the border ring where none is near
        4. seam = dist1 < dist2, as floats
        5. over the roi: where seam, mask2 = 0, elsewhere mask1 = 0 (ties and "no unique cell at all" fall to the else)
Pixels are never read.  Test infrastructure: product code imports neither this nor the oracle."""
import numpy as np

GAP = 10


def overlap_roi(tl1, tl2, sz1, sz2):
    """cv::detail::overlapRoi: (x, y, w, h) or None.  sz = (width, height)."""
    x_tl, y_tl = max(tl1[0], tl2[0]), max(tl1[1], tl2[1])
    x_br, y_br = min(tl1[0] + sz1[0], tl2[0] + sz2[0]), min(tl1[1] + sz1[1], tl2[1] + sz2[1])
    if x_tl < x_br and y_tl < y_br:
        return x_tl, y_tl, x_br - x_tl, y_br - y_tl
    return None


def submask(mask, tl, roi):
    """Step 1: the window of a tile's mask over the roi and its gap, zero outside the tile."""
    x0, y0, w, h = roi
    hp, wp = h + 2 * GAP, w + 2 * GAP
    out = np.zeros((hp, wp), np.uint8)
    oy, ox = y0 - tl[1] - GAP, x0 - tl[0] - GAP          # tile coordinates of the submask's (0, 0)
    ys, xs = max(0, -oy), max(0, -ox)
    ye, xe = min(hp, mask.shape[0] - oy), min(wp, mask.shape[1] - ox)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = mask[oy + ys:oy + ye, ox + xs:ox + xe]
    return out


def unique_cells(sub1, sub2):
    """Step 2."""
    collision = (sub1 != 0) & (sub2 != 0)
    u1, u2 = sub1.copy(), sub2.copy()
    u1[collision] = 0
    u2[collision] = 0
    return u1, u2


def dist_to_unique(unique):
    """Step 3, through the oracle's distance transform (float32)."""
    from oracle import capi
    return capi.distance_transform_l1(np.where(unique == 0, 255, 0).astype(np.uint8))


def find_in_pair(mask1, mask2, tl1, tl2, roi):
    """Steps 1-5 for one pair; edits mask1 / mask2 in place and returns seam over the roi (bool, roi.h x roi.w)."""
    u1, u2 = unique_cells(submask(mask1, tl1, roi), submask(mask2, tl2, roi))
    seam = (dist_to_unique(u1) < dist_to_unique(u2))[GAP:-GAP, GAP:-GAP]
    x0, y0, w, h = roi
    v1 = mask1[y0 - tl1[1]:y0 - tl1[1] + h, x0 - tl1[0]:x0 - tl1[0] + w]
    v2 = mask2[y0 - tl2[1]:y0 - tl2[1] + h, x0 - tl2[0]:x0 - tl2[0] + w]
    v2[seam] = 0
    v1[~seam] = 0
    return seam


def find(sizes, corners, masks):
    """PairwiseSeamFinder::run: sizes = (width, height) per image; masks (uint8 arrays of those sizes) are edited in place."""
    n = len(masks)
    assert len(sizes) == n and len(corners) == n
    for k in range(n):
        assert masks[k].shape == (sizes[k][1], sizes[k][0]) and masks[k].dtype == np.uint8
    if n < 2:
        return masks
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = overlap_roi(corners[i], corners[j], sizes[i], sizes[j])
            if roi is not None:
                find_in_pair(masks[i], masks[j], corners[i], corners[j], roi)
    return masks
