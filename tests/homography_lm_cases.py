"""Inputs of the tests of the Levenberg-Marquardt polish (isx_find_homography_lm): tests/homography_cases.py's point sets under the names
the polish's tests need - pass-1 inlier counts either side of the grouped norm's four and of the wave, data that fit exactly, an iteration
limit that is reached, noise that takes the invert branch and rejects a step, and every way LM does not run.  name -> (points, keyword
arguments of the call); tests/test_homography_lm_model.py asserts that the model reaches what the names say."""
import numpy as np

import homography_cases as cases


def translation(n, seed=3):
    """Integer-valued points under an integer translation, dst = src + (3, -2): the data fit exactly, LM stops by norm(r, NORM_INF)."""
    src = np.random.default_rng(seed).integers(-200, 200, (n, 2)).astype(np.float32)
    return np.ascontiguousarray(np.c_[src, src + np.float32([3, -2])], np.float32)


def named():
    base = cases.named()
    low = dict(num_matches_thresh1=5, num_matches_thresh2=5)
    c = {
        # every correspondence is an inlier: 2n mod 4 is 2, 0, 0, 2 for the grouped norm; 5 is the fewest rows LM accepts
        "inliers_5": (cases.exact(5, 5), low),
        "inliers_6": (cases.exact(6, 6), low),
        "inliers_8": (cases.exact(8, 8), low),
        "inliers_9": (cases.exact(9, 9), low),
        "inliers_63": base["n63_exact"],
        "inliers_64": base["n64_exact"],
        "inliers_65": base["n65_exact"],
        "translation_20": (translation(20), {}),
        "lm_iters_1": (base["n65_half_noisy"][0], dict(lm_max_iters=1)),
        "lm_iters_2": (base["n65_half_noisy"][0], dict(lm_max_iters=2)),
        "noise25_invert_reject": (cases.planted(7000, 30, 22, 2.5), dict(reproj_thresh=6.0)),
        "noise25_invert": (cases.planted(7001, 48, 36, 2.5), dict(reproj_thresh=6.0)),
        "thresh2_above_inliers": (base["n64_half_noisy"][0], dict(num_matches_thresh2=1000)),
        "half_noisy_300": base["n300_half_noisy"],
        "degenerate_det": base["degenerate_det"],
        "outliers_to_the_end": base["outliers_to_the_end"],
        # LM does not run
        "n4_thresh1_4": base["n4_thresh1_4"],
        "n5_below_thresh1": base["n5_below_thresh1"],
        "n3_thresh1_3": base["n3_thresh1_3"],
        "collinear_40": base["collinear_40"],
        "n0": base["n0"],
    }
    return c


NO_LM = ("n4_thresh1_4", "n5_below_thresh1", "n3_thresh1_3", "collinear_40", "n0")
