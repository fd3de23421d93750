"""The named cases of tests/test_gpu_bundle.py, the planted rigs of tests/test_bundle_model.py and the building blocks of tools/fuzz_bundle.py:
synthetic inputs of isx_bundle_adjust_ray.  No matcher, RANSAC or estimator run: a rig has planted rotations and one focal, a match is the
exact projection of a random ray into both images rounded to float32 keypoints, and the cameras that come in are the planted ones turned by
`off_deg` about a random axis, their focal scaled by 1 + `off_focal` and their R scaled as a homography divided by h22 leaves it.  A case is
a dict: sizes ((width, height) per image), keypoints (per image n_i x 2 float32), pairs ((from, to), from < to, global indices), matches (per
pair rows x 3 int32: queryIdx, trainIdx, distance), masks (per pair rows x 1 uint8), counts (1 x pairs int32), stats (pairs x 8 int32), conf
(1 x pairs float64), est_rig_stats (rigs x 8 int32, the estimator's), cameras_in (n x 16 float64), rig_first (None or the image offsets),
conf_thresh, max_iter; planted: (focal, rotations)."""
import numpy as np

from estimator_cases import all_pairs, planted_rotations, rotation  # noqa: F401

ST_H = 1
EST_ASSERT = 2
TILE = 64


def _axis_turn(rng, deg):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


MAX_AXES_DEG = 80.0                            # a pair further apart shares too little view: the inlier loop of make would not end


def ring(n, step_deg, jitter=0.03, seed=0):
    """Planted rotations of a panorama that goes round: camera i has yaw i * step_deg, and all three angles move by up to `jitter` rad
    (seeded).  jitter = 0: the exact yaws, camera 0 the identity."""
    rng = np.random.default_rng([seed, n])
    out = []
    for i in range(n):
        j = rng.uniform(-jitter, jitter, 3) if jitter else np.zeros(3)
        out.append(rotation(np.deg2rad(i * step_deg) + j[0], j[1], j[2]))
    return out


def axes_apart_deg(Ri, Rj):
    """The angle between the optical axes R (0, 0, 1) of two planted cameras."""
    return float(np.rad2deg(np.arccos(np.clip(Ri[:, 2] @ Rj[:, 2], -1.0, 1.0))))


def ring_pairs(rotations, steps=(1,)):
    """The pairs (i, j), i < j, that lie `steps` cameras apart round the ring (the closing pairs included where the ring closes: where their
    axes are less than MAX_AXES_DEG apart), in index order."""
    n = len(rotations)
    out = set()
    for i in range(n):
        for s in steps:
            a, b = sorted((i, (i + s) % n))
            if a != b and axes_apart_deg(rotations[a], rotations[b]) < MAX_AXES_DEG:
                out.add((a, b))
    return sorted(out)


def make(n, pairs, seed, inliers=40, outliers=0.25, focal=900.0, off_deg=1.0, off_focal=0.05, conf=None, center=0, r_scale=1.02, max_iter=30,
         conf_thresh=1.0, size=(1280, 960), rotations=None):
    """One rig.  inliers: an int or one per pair; outliers: the share of mask-0 matches interleaved; conf: per pair (default 2.0); rotations:
    the planted rotations (default: planted_rotations, yaw, pitch and roll of 0.1 to 0.3 rad) - every pair's axes less than MAX_AXES_DEG
    apart."""
    rng = np.random.default_rng(seed)
    if rotations is None:
        Rs = planted_rotations(n, rng)
    else:
        Rs = [np.array(R, np.float64) for R in rotations]
        assert len(Rs) == n and all(axes_apart_deg(Rs[i], Rs[j]) < MAX_AXES_DEG for i, j in pairs), "a pair that shares no view"
    Rs = [Rs[center].T @ R for R in Rs]                       # the centre's R is the identity, as the adjuster leaves it
    sizes = [size] * n
    w, h = size
    K = np.array([[focal, 0, w * 0.5], [0, focal, h * 0.5], [0, 0, 1.0]])
    Ki = np.linalg.inv(K)
    kps = [[] for _ in range(n)]
    inl = [inliers] * len(pairs) if np.isscalar(inliers) else list(inliers)
    matches, masks = [], []
    for k, (i, j) in enumerate(pairs):
        rows, mk = [], []
        while sum(mk) < inl[k]:
            if rng.random() < outliers:
                pi, pj, good = rng.uniform(0, [w, h]), rng.uniform(0, [w, h]), 0
            else:
                pi = rng.uniform([0, 0], [w, h])
                d = Rs[i] @ Ki @ np.array([pi[0], pi[1], 1.0])  # the ray of calcError: R K^-1 p
                q = K @ Rs[j].T @ d
                if q[2] <= 0:
                    continue
                pj, good = q[:2] / q[2], 1
            kps[i].append(pi)
            kps[j].append(pj)
            rows.append((len(kps[i]) - 1, len(kps[j]) - 1, int(rng.integers(0, 60))))
            mk.append(good)
        matches.append(np.array(rows, np.int32).reshape(-1, 3))
        masks.append(np.array(mk, np.uint8).reshape(-1, 1))
    keypoints = [np.array(k, np.float32).reshape(-1, 2) for k in kps]
    cams = np.zeros((n, 16))
    for i in range(n):
        cams[i, 0:4] = [focal * (1 + off_focal * (1 if i % 2 == 0 else -1)), 1.0, w * 0.5, h * 0.5]
        cams[i, 4:13] = ((_axis_turn(rng, off_deg) @ Rs[i]) * r_scale ** (i % 3)).ravel()
    stats = np.zeros((len(pairs), 8), np.int32)
    stats[:, 0] = ST_H
    stats[:, 1] = [int(m.sum()) for m in masks]
    est = np.array([[1, 2 * len(pairs), center, -1, n - 1, n, 1, 1]], np.int32)
    return dict(sizes=sizes, keypoints=keypoints, pairs=list(pairs), matches=matches, masks=masks,
                counts=np.array([[len(m) for m in matches]], np.int32).reshape(1, -1), stats=stats,
                conf=np.array([[2.0] * len(pairs) if conf is None else conf], np.float64).reshape(1, -1), est_rig_stats=est, cameras_in=cams, rig_first=None,
                conf_thresh=conf_thresh, max_iter=max_iter, planted=(focal, Rs))


def join(rigs):
    """Several one-rig cases as the rigs of one call (conf_thresh and max_iter of the first)."""
    out = dict(sizes=[], keypoints=[], pairs=[], matches=[], masks=[], rig_first=[0], conf_thresh=rigs[0]["conf_thresh"], max_iter=rigs[0]["max_iter"])
    for r in rigs:
        a = out["rig_first"][-1]
        out["sizes"] += r["sizes"]
        out["keypoints"] += r["keypoints"]
        out["pairs"] += [(i + a, j + a) for i, j in r["pairs"]]
        out["matches"] += r["matches"]
        out["masks"] += r["masks"]
        out["rig_first"].append(a + len(r["sizes"]))
    out["counts"] = np.concatenate([r["counts"] for r in rigs], 1)
    out["conf"] = np.concatenate([r["conf"] for r in rigs], 1)
    out["stats"] = np.concatenate([r["stats"] for r in rigs])
    out["est_rig_stats"] = np.concatenate([r["est_rig_stats"] for r in rigs])
    out["cameras_in"] = np.concatenate([r["cameras_in"] for r in rigs])
    return out


def named():
    out = {}
    out["two_images_8_inliers"] = make(2, [(0, 1)], 1, inliers=8)                                   # 8 parameters, 24 rows
    for it in (1, 2, 3):
        out["max_iter_%d" % it] = make(3, all_pairs(3), 2, inliers=12, max_iter=it)
    out["conf_equal_thresh_is_excluded"] = make(3, all_pairs(3), 3, inliers=10, conf=[2.0, 1.0, 1.5], max_iter=4)      # the test is >
    # one fewer, exactly, one more inlier than the tile of the accumulation, and past two tiles; zeros interleaved in every mask
    out["tiles_5"] = make(5, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 4), (3, 4)], 4, inliers=[TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5, 2 * TILE], max_iter=2)
    out["camera_without_edge"] = make(4, all_pairs(4), 5, inliers=9, conf=[2.0, 2.0, 0.5, 2.0, 0.25, 1.0], max_iter=5)    # camera 3: no pair above 1
    out["rig_without_edge"] = make(3, all_pairs(3), 6, inliers=7, conf=[1.0, 0.0, 0.9])
    c = make(3, all_pairs(3), 7, inliers=7)
    c["est_rig_stats"][0, 0] |= EST_ASSERT
    out["estimator_assert_bit"] = c
    c = make(3, all_pairs(3), 8, inliers=7, max_iter=5)
    c["cameras_in"][1, 0] = np.nan
    out["nan_focal_in"] = c
    c = make(3, all_pairs(3), 9, inliers=10, max_iter=3)
    c["counts"][0, 1] = c["matches"][1].shape[0] + 5                                               # clamped to the mat's rows
    c["counts"][0, 2] = -3                                                                          # a negative count is 0
    out["count_above_rows"] = c
    c = make(3, all_pairs(3), 10, inliers=10, max_iter=3)
    c["matches"][0][2, 0] = c["keypoints"][0].shape[0]                                              # indices outside the keypoints: not inliers
    c["matches"][0][4, 1] = -1
    out["index_outside_keypoints"] = c
    c = make(3, all_pairs(3), 11, inliers=10, max_iter=3)
    c["cameras_in"][2, 4:13] = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 1.0]]).ravel()      # a singular R: the identity
    out["singular_R_in"] = c
    c = make(3, all_pairs(3), 12, inliers=10, max_iter=3, center=1)
    c["pairs"], c["matches"], c["masks"] = c["pairs"][::-1], c["matches"][::-1], c["masks"][::-1]   # the caller's order is not index order
    c["counts"], c["conf"], c["stats"] = c["counts"][:, ::-1].copy(), c["conf"][:, ::-1].copy(), c["stats"][::-1].copy()
    out["pairs_in_another_order"] = c
    out["chain_64"] = make(64, [(i, i + 1) for i in range(63)], 15, inliers=4, outliers=0.2, max_iter=3, center=31)      # 256 parameters: a thread each
    out["tiles_past_a_block"] = make(24, all_pairs(24), 16, inliers=1, outliers=0.0, max_iter=2)      # 276 tiles: the norm's second chunk of 256
    out["natural_end_2"] = make(2, [(0, 1)], 13, inliers=10, max_iter=1000)
    out["natural_end_3"] = make(3, all_pairs(3), 14, inliers=8, max_iter=1000)
    out.update(wide(make))
    return out


WIDE = ("ring_8x45_center_0", "ring_8x45_center_4", "ring_8x45_exact_half_turn", "ring_6x60_center_0", "arc_5x50_natural_end", "reflection_R_in",
        "ring_16x22p5_two_steps")


def wide(make):
    """The rigs that go round (tests/test_bundle_model.py counts the branches of bundle_math.hpp that these take and no narrow rig does):
    rotation vectors up to half a turn, so every branch of acos, quadrants 1 and 2 of sin / cos, the half turn of cvRodrigues2 and the
    det < 0 of the polar factor.  make: this module's, or bundle_reproj_cases'.  12 inliers an edge."""
    out = {}
    r8 = ring(8, 45.0, seed=21)
    out["ring_8x45_center_0"] = make(8, ring_pairs(r8), 31, inliers=12, max_iter=4, rotations=r8)       # the chain and the closing pair (0, 7)
    out["ring_8x45_center_4"] = make(8, ring_pairs(r8), 32, inliers=12, max_iter=3, center=4, rotations=r8)      # camera 0: half a turn from the centre
    e8 = ring(8, 45.0, jitter=0.0)
    out["ring_8x45_exact_half_turn"] = make(8, ring_pairs(e8), 33, inliers=12, max_iter=3, off_deg=0.0, r_scale=1.0, rotations=e8)      # camera 4: rotation(pi, 0, 0)
    r6 = ring(6, 60.0, seed=22)
    out["ring_6x60_center_0"] = make(6, ring_pairs(r6), 34, inliers=12, max_iter=4, rotations=r6)
    a5 = ring(5, 50.0, seed=23)
    out["arc_5x50_natural_end"] = make(5, ring_pairs(a5), 35, inliers=12, max_iter=1000, rotations=a5)   # 200 degrees: the ring does not close
    c = make(3, all_pairs(3), 36, inliers=12, max_iter=3)
    c["cameras_in"][1, 4:13] = (c["cameras_in"][1, 4:13].reshape(3, 3) @ np.diag([1.0, 1.0, -1.0])).ravel()      # det < 0: the polar factor is negated
    out["reflection_R_in"] = c
    r16 = ring(16, 22.5, seed=24)
    out["ring_16x22p5_two_steps"] = make(16, ring_pairs(r16, (1, 2)), 37, inliers=12, max_iter=2, rotations=r16)      # Ray: 64 unknowns, one wave of rows
    return out
