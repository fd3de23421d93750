"""The named cases of tests/test_gpu_bundle_reproj.py, the planted rigs of tests/test_bundle_reproj_model.py and the rigs of
tests/test_gpu_wave_correct.py: bundle_cases.make (planted rotations and one focal, exact projections rounded to float32 keypoints, cameras
that come in turned and with their focal scaled) plus what BundleAdjusterReproj refines beyond BundleAdjusterRay - the cameras come in with
their principal point moved by `off_pp` pixels and their aspect scaled by 1 + `off_aspect`, alternating in sign from camera to camera.  A case
is bundle_cases' dict with refine_flags added; planted: (focal, rotations, ppx, ppy, aspect)."""
import numpy as np

import bundle_cases as bc
from bundle_cases import EST_ASSERT, TILE, WIDE, all_pairs, join, ring, ring_pairs  # noqa: F401

REFINE_ALL = 31


def plant(c, off_pp=(6.0, -4.0), off_aspect=0.01, refine_flags=REFINE_ALL):
    """The offsets of ppx, ppy and aspect on cameras_in (in place); returns c."""
    cams = c["cameras_in"]
    w, h = c["sizes"][0]
    for i in range(cams.shape[0]):
        sg = 1.0 if i % 2 == 0 else -1.0
        cams[i, 1] = 1.0 + sg * off_aspect
        cams[i, 2] += sg * off_pp[0]
        cams[i, 3] -= sg * off_pp[1]
    c["refine_flags"] = refine_flags
    c["planted"] = c["planted"] + (w * 0.5, h * 0.5, 1.0)
    return c


def make(n, pairs, seed, refine_flags=REFINE_ALL, off_pp=(6.0, -4.0), off_aspect=0.01, **kw):
    return plant(bc.make(n, pairs, seed, **kw), off_pp, off_aspect, refine_flags)


def chain(n):
    return [(i, i + 1) for i in range(n - 1)]


def chain_64():
    """448 unknowns: every row of the block's Cholesky.  The model's outputs are recorded in tests/golden/bundle_reproj_chain64.npz."""
    return make(64, chain(64), 15, inliers=4, outliers=0.2, max_iter=1, center=31)


def named():
    out = {}
    out["two_images_8_inliers"] = make(2, [(0, 1)], 1, inliers=8)                                   # 14 unknowns, 16 rows
    for it in (1, 2, 3):
        out["max_iter_%d" % it] = make(3, all_pairs(3), 2, inliers=12, max_iter=it)
    out["conf_equal_thresh_is_excluded"] = make(3, all_pairs(3), 3, inliers=10, conf=[2.0, 1.0, 1.5], max_iter=4)
    out["tiles_5"] = make(5, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 4), (3, 4)], 4, inliers=[TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5, 2 * TILE], max_iter=2)
    out["camera_without_edge"] = make(4, all_pairs(4), 5, inliers=9, conf=[2.0, 2.0, 0.5, 2.0, 0.25, 1.0], max_iter=5)
    out["rig_without_edge"] = make(3, all_pairs(3), 6, inliers=7, conf=[1.0, 0.0, 0.9])
    c = make(3, all_pairs(3), 7, inliers=7)
    c["est_rig_stats"][0, 0] |= EST_ASSERT
    out["estimator_assert_bit"] = c
    c = make(3, all_pairs(3), 8, inliers=7, max_iter=5)
    c["cameras_in"][1, 0] = np.nan
    out["nan_focal_in"] = c
    c = make(3, all_pairs(3), 9, inliers=10, max_iter=3)
    c["counts"][0, 1] = c["matches"][1].shape[0] + 5
    c["counts"][0, 2] = -3
    out["count_above_rows"] = c
    c = make(3, all_pairs(3), 10, inliers=10, max_iter=3)
    c["matches"][0][2, 0] = c["keypoints"][0].shape[0]
    c["matches"][0][4, 1] = -1
    out["index_outside_keypoints"] = c
    c = make(3, all_pairs(3), 11, inliers=10, max_iter=3)
    c["cameras_in"][2, 4:13] = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 1.0]]).ravel()
    out["singular_R_in"] = c
    c = make(3, all_pairs(3), 12, inliers=10, max_iter=3, center=1)
    c["pairs"], c["matches"], c["masks"] = c["pairs"][::-1], c["matches"][::-1], c["masks"][::-1]
    c["counts"], c["conf"], c["stats"] = c["counts"][:, ::-1].copy(), c["conf"][:, ::-1].copy(), c["stats"][::-1].copy()
    out["pairs_in_another_order"] = c
    out["chain_37"] = make(37, chain(37), 17, inliers=3, outliers=0.2, max_iter=2, center=18)      # 259 unknowns: the first size past 256 rows / four waves
    out["tiles_past_a_block"] = make(33, all_pairs(33), 16, inliers=1, outliers=0.0, max_iter=2)   # 528 tiles: the norm's second chunk of 512
    out["natural_end_2"] = make(2, [(0, 1)], 13, inliers=10, max_iter=1000)
    out["natural_end_3"] = make(3, all_pairs(3), 14, inliers=8, max_iter=1000)
    for flags in (0, 1, 31):                                                                        # one rig: rotations only, with the focal, everything
        out["refine_flags_%d" % flags] = make(3, all_pairs(3), 18, inliers=12, max_iter=4, refine_flags=flags)
    # z driven to 0: a focal of exactly 0 makes K singular, Mat::inv() gives nine zeros, H of the camera's edges is zero and every match of
    # theirs divides 0 by 0 - NaN residuals, NaN sums, a NaN trace rule under which every pivot drops: the step is 0, both |err| are NaN
    c = make(3, all_pairs(3), 19, inliers=6, max_iter=3)
    c["cameras_in"][0, 0] = 0.0
    out["z_zero"] = c
    out.update(bc.wide(make))                                                                       # the rigs that go round (Reproj: 112 unknowns for 16 cameras)
    return out


# ---- rigs of rotations for the wave correction -----------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def cameras_of(Rs, focal=900.0, size=(1280, 960)):
    cams = np.zeros((len(Rs), 16))
    for i, R in enumerate(Rs):
        cams[i, 0:4] = [focal + i, 1.0 + 0.001 * i, size[0] * 0.5 + i, size[1] * 0.5 - i]
        cams[i, 4:13] = np.asarray(R, np.float64).ravel()
        cams[i, 13:16] = [0.25 * i, -0.5, 1.0]                # t is copied, whatever it holds
    return cams


def pan_about_tilted_axis(n, tilt_deg=12.0, roll_deg=5.0, step_deg=9.0, wobble=0.0, seed=0):
    """n cameras that pan about one axis, tilted from the y axis: what a hand-held sweep gives, and what waveCorrect straightens.  wobble:
    a random turn of that many degrees on each camera."""
    rng = np.random.default_rng(seed)
    T = _rot([1, 0, 0], tilt_deg) @ _rot([0, 0, 1], roll_deg)
    Rs = []
    for i in range(n):
        R = T @ _rot([0, 1, 0], step_deg * (i - (n - 1) / 2))
        if wobble:
            R = _rot(rng.normal(size=3), wobble) @ R
        Rs.append(R)
    return Rs


def wave_rigs():
    """name -> cameras (n x 16 float64) of one rig."""
    out = {}
    out["one_image"] = cameras_of(pan_about_tilted_axis(1))
    out["pan_2"] = cameras_of(pan_about_tilted_axis(2, wobble=1.0, seed=1))
    out["pan_3"] = cameras_of(pan_about_tilted_axis(3, wobble=0.5, seed=2))
    out["pan_5_planted"] = cameras_of(pan_about_tilted_axis(5))
    out["pan_64"] = cameras_of(pan_about_tilted_axis(64, step_deg=5.0, wobble=1.0, seed=3))
    # upside down: the cameras' x axes point against rg0, conf < 0 and both rows are negated
    out["flip"] = cameras_of([_rot([0, 0, 1], 180.0) @ R for R in pan_about_tilted_axis(4, wobble=0.5, seed=4)])
    # degenerate: every column 2 sums to zero, rg0 = rg1 x 0 = 0
    out["degenerate"] = cameras_of([np.eye(3), np.diag([1.0, -1.0, -1.0])])
    return out
