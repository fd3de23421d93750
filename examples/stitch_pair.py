#!/usr/bin/env python3
"""The reference demo's post-registration stage on one pair of images, every step on the GPU through imagestitch_amd
(needs an MI355X):

    python examples/stitch_pair.py [left.bmp right.bmp] [--register [--small] [--features orb|surf|sift]] [--focal F] [--yaw RAD] [--warper cylindrical|spherical|plane] [--blend feather|multiband] [--seam-megapix M] [--out pano.bmp | pano.jpg]

By default registration is replaced by a known rig: two cameras
with focal length F rotated by -/+ yaw about the vertical axis.  Without input files a synthetic pair is generated.
With --register nothing is supplied from outside: OrbFeaturesFinder (F:948-1017), BestOf2NearestMatcher (M:307-308, R:830-911) and
HomographyBasedEstimator (C:246-284) take the two images to the cameras the warp uses, from image files to pano.bmp.

Steps = the reference's main(): warp image + mask (W:223-233), gain apply with given gains (W:241-244) - or, with
--estimate-gains, the compensator's feed on the warped tiles (W:238-240) and its apply (W:241-244): --compensator gain is the
GainCompensator the demos create, gain_blocks the BlocksGainCompensator of createDefault(GAIN_BLOCKS) -, convertTo(CV_32F) +
DP seam finder (S:87-1093, --seam-cost color_grad: DpSeamFinder::COLOR_GRAD W:255; --seam graphcut: W's own GraphCutSeamFinder, W:257-264, with --seam-cost color_grad its COST_COLOR_GRAD, W:258; --seam voronoi: the VoronoiSeamFinder S constructs, S:1180), dilate 20x20 & warped mask (W:286-301), FeatherBlender 0.1 (W:278-313) or the
multi-band blender (W:271-273), imwrite (W:315).  --seam-megapix M finds the seams at reduced scale the way OpenCV's stitching_detailed
does: resize, small warp, finder, then dilate 3x3 + resize + AND per tile at compose time (isx.resize, isx.dilate_resize_and)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import imagestitch_amd as isx  # noqa: E402
from imagestitch_amd import synth  # noqa: E402


BUILT_IN_HESS_THRESH = 100.0
BUILT_IN_CONTRAST_THRESHOLD = 0.02


def register_views(small=False):
    """The two views --register takes without input files: overlapping crops of one synthetic scene, 1280 x 720 out of 1600 x 720 - or,
    small, 480 x 270 out of 600 x 270; three quarters of each crop lie in the other."""
    h, w, shift = (270, 480, 120) if small else (720, 1280, 320)
    wide = synth.make_tile(h, w + shift, 0)
    return [np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, shift:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="*")
    ap.add_argument("--register", action="store_true",
                    help="find ORB features, match them and estimate the cameras on the GPU instead of assuming the rig of --focal and --yaw")
    ap.add_argument("--small", action="store_true",
                    help="with --register and no input files: crops of 480 x 270 instead of 1280 x 720 (a quick run)")
    ap.add_argument("--features", default="orb", choices=["orb", "surf", "sift"],
                    help="with --register: OrbFeaturesFinder (32-byte descriptors, Hamming), SurfFeaturesFinder (64 floats, L2) or "
                         "SiftFeaturesFinder (128 floats, L2)")
    ap.add_argument("--contrast-threshold", type=float, default=None,
                    help="with --features sift: SiftFeaturesFinder's contrast_threshold; default 0.04, or 0.02 on the built-in views, whose smooth "
                         "synthetic scene leaves 15 keypoints a view at 0.04")
    ap.add_argument("--hess-thresh", type=float, default=None,
                    help="with --features surf: SurfFeaturesFinder's hess_thresh; default 300, or 100 on the built-in views, whose smooth synthetic "
                         "scene has no Hessian response above 200")
    ap.add_argument("--focal", type=float, default=None)
    ap.add_argument("--yaw", type=float, default=0.18)
    ap.add_argument("--warper", default="cylindrical", choices=["cylindrical", "spherical", "plane", "fisheye", "stereographic"],
                    help="the warper list of the reference's demos (B:91-95): cv::PlaneWarper, cv::CylindricalWarper (the one they run), cv::SphericalWarper, "
                         "cv::FisheyeWarper, cv::StereographicWarper")
    ap.add_argument("--blend", default="feather", choices=["feather", "multiband"])
    ap.add_argument("--gains", type=float, nargs=2, default=[1.0, 1.0])
    ap.add_argument("--estimate-gains", action="store_true",
                    help="estimate the gains from the warped tiles as the reference does (GainCompensator feed, then apply; W:238-244) "
                         "instead of taking --gains")
    ap.add_argument("--compensator", default="gain", choices=["gain", "gain_blocks"],
                    help="with --estimate-gains: ExposureCompensator::createDefault(GAIN), one gain per tile, or (GAIN_BLOCKS), one per 32 x 32 "
                         "block, applied as a smoothed gain map (W:238)")
    ap.add_argument("--seam", default="dp", choices=["dp", "graphcut", "voronoi"],
                    help="dp: the DP seam finder on a copy of the warped masks (S:1192); graphcut: W's own GraphCutSeamFinder(COST_COLOR) (or COST_COLOR_GRAD with --seam-cost color_grad), "
                         "which edits the warped masks while masks_seam stays their unedited copy (W:247-264); voronoi: the VoronoiSeamFinder of "
                         "S:1180 on masks_seam (S:1192), masks only")
    ap.add_argument("--seam-cost", default="color", choices=["color", "color_grad"],
                    help="--seam dp: the finder's cost function, DpSeamFinder::COLOR (W:253) or DpSeamFinder::COLOR_GRAD (W:255, S:1183); "
                         "--seam graphcut: GraphCutSeamFinder::COST_COLOR (W:257) or COST_COLOR_GRAD (W:258)")
    ap.add_argument("--seam-megapix", type=float, default=0.0,
                    help="find the seams at reduced scale, as OpenCV's stitching_detailed does (its default: 0.1): the sources are resized by "
                         "seam_scale = min(1, sqrt(M * 1e6 / (W * H))) (isx.resize), warped with K and the warper's scale times seam_scale, the finder "
                         "runs on the small tiles, and dilate_resize_and(small seam mask, full warped mask, 3, 3) replaces the 20 x 20 dilate.  "
                         "0 (the default): off, the seams are found at full size")
    ap.add_argument("--out", default="pano.bmp")
    ap.add_argument("--separate", action="store_true",
                    help="gain apply and mask preparation as passes of their own (isx_gain_apply, isx_mask_dilate_and) instead of folded into the warp's "
                         "store (isx_warper_set_gain) and into the feed (isx_blender_feed_dilated): same panorama, two passes per tile more")
    a = ap.parse_args()
    if a.images:
        imgs = [isx.imread(p) for p in a.images[:2]]                       # W:166
    elif a.register:                                                        # two views of one scene: overlapping crops
        imgs = register_views(a.small)
    else:
        imgs = [synth.make_tile(720, 1280, i) for i in range(2)]
    H, W = imgs[0].shape[:2]
    if a.register:
        hess = a.hess_thresh if a.hess_thresh is not None else (300.0 if a.images else BUILT_IN_HESS_THRESH)
        finder = isx.SurfFeaturesFinder(hess_thresh=hess) if a.features == "surf" else isx.OrbFeaturesFinder()       # B:36-37: the line the demos comment out
        if a.features == "sift":                                            # cv::Stitcher's other finder; stitching_detailed --features sift
            contrast = a.contrast_threshold if a.contrast_threshold is not None else (0.04 if a.images else BUILT_IN_CONTRAST_THRESHOLD)
            finder = isx.SiftFeaturesFinder(contrast_threshold=contrast)
        features = finder.find(imgs)                                        # F:1034-1040: finder(img, features)
        matcher = isx.BestOf2NearestMatcher(match_conf=0.3)                 # M:307
        info = matcher.match([f.descriptors for f in features], [f.keypoints for f in features], [f.img_size for f in features])   # M:308
        if not info or info[0].H is None:
            sys.exit("registration failed: %s keypoints, %d matches" % ([int(f.keypoints.shape[0]) for f in features], info[0].matches.shape[0] if info else 0))
        cameras = isx.HomographyBasedEstimator()([f.img_size for f in features], matcher)      # C:246-284
        F = float(np.median([c.focal for c in cameras]))                    # W:207-216: the warper's scale is the median focal
        Kl, Rs = [c.K32 for c in cameras], [c.R32 for c in cameras]
        print("registered: keypoints %s, %d matches, %d inliers, focals %s" % ([int(f.keypoints.shape[0]) for f in features], info[0].matches.shape[0],
                                                                             info[0].num_inliers, ["%.1f" % c.focal for c in cameras]))
    else:
        F = a.focal or 1.1 * W
        K, Rs = synth.camera_pair(W, H, F, yaw=a.yaw)
        Kl = [K, K]
    creator = {"cylindrical": isx.CylindricalWarper, "spherical": isx.SphericalWarper, "plane": isx.PlaneWarper, "fisheye": isx.FisheyeWarper,
               "stereographic": isx.StereographicWarper}[a.warper]          # B:91-95
    warper = creator().create(F)                                            # W:217-222
    corners, warped, wmasks = [], [], []
    for i in range(2):
        if a.estimate_gains:                                                # the gains are not known before the warp: apply comes after feed
            c, wi, wm = warper.warp_with_mask(imgs[i], Kl[i], Rs[i])           # W:229, W:232
        elif a.separate:
            c, wi, wm = warper.warp_with_mask(imgs[i], Kl[i], Rs[i])           # W:229, W:232
            isx.gain_apply(wi, a.gains[i])                                  # W:241-244
        else:                                                               # W:241-244 folded into the warp's store (gains known: a fixed rig)
            warper.set_gain(a.gains[i])
            c, wi, wm = warper.warp_with_mask(imgs[i], Kl[i], Rs[i])           # W:229, W:232
        corners.append(tuple(c)); warped.append(wi); wmasks.append(wm)
    if a.estimate_gains:
        compensator = isx.BlocksGainCompensator() if a.compensator == "gain_blocks" else isx.GainCompensator()   # W:238
        compensator.feed(corners, warped, wmasks)                           # W:240
        for i in range(2):
            compensator.apply(i, corners[i], warped[i], wmasks[i])          # W:241-244
        g = compensator.gains()
        if a.compensator == "gain_blocks":
            print("estimated gains of %d blocks: %.9f to %.9f" % (g.size, g.min(), g.max()))
        else:
            print("estimated gains", " ".join("%.9f" % v for v in g))
    def find(tiles, tile_corners, masks):                                  # the chosen finder, masks edited in place
        if a.seam == "graphcut":
            cost = isx.seam.COST_COLOR_GRAD if a.seam_cost == "color_grad" else isx.seam.COST_COLOR
            isx.GraphCutSeamFinder(cost).find([w.astype(np.float32) for w in tiles], tile_corners, masks)   # W:257 / W:258, W:261-264
        elif a.seam == "voronoi":
            isx.VoronoiSeamFinder().find(tiles, tile_corners, masks)        # S:1180, S:1192
        else:
            cost = isx.DP_COLOR_GRAD if a.seam_cost == "color_grad" else isx.DP_COLOR
            isx.DpSeamFinder(cost).find([w.astype(np.float32) for w in tiles], tile_corners, masks)   # W:253 / W:255, W:259-262

    if a.seam_megapix > 0:
        # OpenCV's stitching_detailed / Stitcher::composePanorama: the seams are found on sources resized to seam_megapix and warped with
        # K and the warper's scale multiplied by the same factor; the small seam masks come back to full size in the compose loop below
        seam_scale = min(1.0, float(np.sqrt(a.seam_megapix * 1e6 / (W * H))))
        small = [isx.resize(im, fx=seam_scale, fy=seam_scale) for im in imgs]
        Ks = [np.array(k, np.float32) for k in Kl]
        for k in Ks:
            for r, c in ((0, 0), (0, 2), (1, 1), (1, 2)):
                k[r, c] = np.float32(k[r, c] * np.float32(seam_scale))
        small_warper = creator().create(float(np.float32(F) * np.float32(seam_scale)))
        small_corners, small_warped, seam = [], [], []
        for i in range(2):
            c, wi, wm = small_warper.warp_with_mask(small[i], Ks[i], Rs[i])
            small_corners.append(tuple(c)); small_warped.append(wi); seam.append(wm)
        find(small_warped, small_corners, seam)
        print("seam scale %.4f: sources %d x %d, warped tiles %s" % (seam_scale, small[0].shape[1], small[0].shape[0], [(w.shape[1], w.shape[0]) for w in small_warped]))
    else:
        seam = [m.copy() for m in wmasks]                                   # W:247-249
        # graphcut, W:257-264 as written: find edits masks_warped, and the blender gets dilate(masks_seam) & masks_warped (W:286-301);
        # the S demo's finders edit masks_seam (S:1192)
        find(warped, corners, wmasks if a.seam == "graphcut" else seam)
    sizes = [(w.shape[1], w.shape[0]) for w in warped]
    if a.blend == "feather":
        blender = isx.FeatherBlender(False, 0.1)                            # W:278-280
    else:
        blender = isx.MultiBandBlender(False, 4, isx.PREC_I16)              # W:271-273
    blender.prepare(corners, sizes)                                         # W:281
    for i in range(2):
        if a.seam_megapix > 0:                                              # dilate(seam, Mat()); resize(.., mask_warped.size()); & mask_warped
            mk = isx.dilate_resize_and(seam[i], wmasks[i], 3, 3)
            blender.feed(warped[i].astype(np.int16), mk, corners[i])        # W:294, W:302
        elif a.separate:
            mk = isx.dilate_and(seam[i], 20, 20, other=wmasks[i])           # W:295-301
            blender.feed(warped[i].astype(np.int16), mk, corners[i])        # W:294, W:302
        else:                                                               # W:294-302 in one call
            blender.feed_dilated(warped[i].astype(np.int16), seam[i], wmasks[i], 20, 20, corners[i])
    result, result_mask = blender.blend(out_u8=True)                        # W:313 + the convertTo(CV_8U) of imwrite
    isx.imwrite(a.out, result)                                              # W:315
    print("corners", corners, "sizes", sizes, "->", a.out, result.shape, "covered %.1f %%" % (100.0 * (result_mask > 0).mean()))


if __name__ == "__main__":
    main()
