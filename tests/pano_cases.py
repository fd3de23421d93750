"""A planted rotating rig rendered by plain float64 NumPy, and the measures that hold the chain from pixels to panorama to it
(tests/test_pano_model.py on the NumPy models, tests/test_gpu_pano_chain.py on the GPU classes).  Nothing here was written from a model of
ours: a view is the texture of orb_cases.scene read as a cylinder (TEX_SCALE pixels a radian) through the ray R K^-1 (x, y, 1), and a
measure projects with formulas written out here.

Conventions of the ground truth (cv::detail's, which the chain claims to recover): a pixel (x, y) of view i looks along the world ray
R_i K_i^-1 (x, y, 1), K = [[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]]; x to the right, y down, z forward; a positive yaw turns the view to
the right.  Recovered rotations are defined up to one common rotation (the centre's), so every measure is relative: a pair's relative
rotation, the distance of two projections of one world ray.

The measurement (python tests/pano_cases.py prints it; the NumPy models and the CPU oracle only, no GPU) is recorded at the end of this
file:

  rig3(): texture scene(420, 760, 31, channels=3), three 320 x 240 views, focal 300, yaw -12 / 0 / +12 degrees, pitch and roll up to 0.02 rad.
    keypoints 450 / 440 / 457; pairs (0,1) (0,2) (1,2): matches 151 / 103 / 226, inliers 131 / 82 / 209, confidence 2.46 / 2.11 / 2.76
                          focal error   rotation error   misregistration, worst pair and kind: mean / max
    estimator             23.5          0.48 deg         0.36 / 1.46 px
    BundleAdjusterRay      2.3          0.16 deg         0.15 / 0.42 px
    BundleAdjusterReproj   7.6          0.72 deg         0.17 / 0.51 px   (it also moves aspect to 1.036 and ppx by up to 3.6 px)
    At the 14 degrees first tried the reprojection adjuster's largest misregistration was 1.5 px, its doubled bound past 2 px; 12 degrees is
    the more overlap that keeps every adjuster's doubled bound below 2 px.
  rig3_plus_2(): rig3() and two one-channel views of scene(420, 760, 47), yaw -5 / +5 degrees: keypoints 475 / 462, 232 matches, 217 inliers,
    confidence 2.80; the six pairs across the rigs reach a confidence of 0.41 at the most without the mask.
  Every bound a test asserts on these is BOUND_FACTOR (2) x the measured value of the model chain: the margin tests/test_gpu_orb_chain.py
  takes for a change in match order moving RANSAC's draw.  The GPU chain is bit-equal to the models and gets no margin of its own.
  Composition (oracle steps on the model chain's wave-corrected Ray cameras): overlap agreement 2.5 gray levels, ground-truth error 6.4 - 6.8
  against 3.1 - 3.6 with the planted cameras (two bilinear passes over a noisy texture).  With BundleAdjusterReproj's cameras the error is
  11.5: its aspect of 1.036 stretches the whole panorama against the texture while the views still agree with each other (0.17 px), so
  2 gt_planted + overlap (8.8) is asked of the Ray adjuster's cameras, the adjuster the reference's demos run, and REPROJ_CASE is held to
  its own recorded figures."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import orb_cases  # noqa: E402

TEX_H, TEX_W, TEX_SCALE = 420, 760, 400.0
VIEW_W, VIEW_H, FOCAL = 320, 240, 300.0
KINDS = ("cylindrical", "spherical", "plane")
STAGES = ("est", "ray", "reproj", "wave_ray", "wave_reproj")
GRID_STEP, INSIDE_PX, ERODE_PX, BOUND_FACTOR = 12, 8, 8, 2.0
CONTROL_FLOOR_PX = 20.0                   # a floor, not a measurement: the planted yaw step alone is about 60 px of panorama


# ---- the planted rig ------------------------------------------------------------------------------------------------------------------
def rotation(yaw, pitch=0.0, roll=0.0):
    """R = Ry(yaw) Rx(pitch) Rz(roll), float64: the view's axes in the world's."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def k_of(focal, size, aspect=1.0, ppx=None, ppy=None):
    w, h = size
    return np.array([[focal, 0.0, 0.5 * w if ppx is None else ppx], [0.0, focal * aspect, 0.5 * h if ppy is None else ppy], [0.0, 0.0, 1.0]])


def lookup(texture, rays):
    """The cylindrical texture along world rays (... x 3): bilinear in float64.  Returns (values ... [x channels] float64, inside ...)."""
    tex = np.asarray(texture, np.float64)
    th, tw = tex.shape[:2]
    X, Y, Z = rays[..., 0], rays[..., 1], rays[..., 2]
    u = 0.5 * (tw - 1) + TEX_SCALE * np.arctan2(X, Z)
    v = 0.5 * (th - 1) + TEX_SCALE * Y / np.sqrt(X * X + Z * Z)
    inside = (u >= 0) & (u <= tw - 1) & (v >= 0) & (v <= th - 1)
    uc, vc = np.clip(u, 0, tw - 1), np.clip(v, 0, th - 1)
    x0, y0 = np.minimum(np.floor(uc).astype(np.int64), tw - 2), np.minimum(np.floor(vc).astype(np.int64), th - 2)
    fx, fy = uc - x0, vc - y0
    if tex.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    val = (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy
    return val, inside


def render(texture, size, focal, R):
    """The view of size (width, height) and focal `focal` turned by R: uint8, 1 or 3 channels as the texture.  Every ray lands inside the
    texture (asserted), so no border rule enters the ground truth."""
    w, h = size
    xx, yy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    p = np.stack([xx, yy, np.ones_like(xx)], -1)
    rays = p @ (np.asarray(R, np.float64) @ np.linalg.inv(k_of(focal, size))).T
    val, inside = lookup(texture, rays)
    assert inside.all(), "render: a ray leaves the texture"
    return np.ascontiguousarray(np.rint(val).astype(np.uint8))


def _rig(seed, angles, channels=1):
    tex = orb_cases.scene(TEX_H, TEX_W, seed, channels)
    Rs = [rotation(np.deg2rad(y), p, r) for y, p, r in angles]
    size = (VIEW_W, VIEW_H)
    return dict(texture=tex, views=[render(tex, size, FOCAL, R) for R in Rs], sizes=[size] * len(Rs), focal=FOCAL, Rs=Rs, rigs=None, mask=None,
                textures=[tex] * len(Rs))


RIG3_ANGLES = ((-12.0, 0.02, -0.015), (0.0, -0.01, 0.02), (12.0, 0.015, 0.01))      # yaw in degrees, pitch and roll in radians
RIG2_ANGLES = ((-5.0, -0.015, 0.01), (5.0, 0.02, -0.02))


@functools.lru_cache(maxsize=None)
def rig3():
    """Three 3-channel views 12 degrees apart (14 leaves an adjuster's largest misregistration above 1 px, see the header).  A dict: texture,
    views, sizes, focal, Rs (planted), rigs, mask.  Shared, never written to."""
    return _rig(31, RIG3_ANGLES, 3)


@functools.lru_cache(maxsize=None)
def rig3_plus_2():
    """rig3() and a two-view rig of another texture (one channel, 10 degrees apart) in one list: rigs = [3, 2] and the 5 x 5 matcher mask
    that keeps pairs inside a rig."""
    a, b = rig3(), _rig(47, RIG2_ANGLES)
    mask = np.zeros((5, 5), np.uint8)
    mask[0:3, 0:3] = 1
    mask[3:5, 3:5] = 1
    return dict(views=a["views"] + b["views"], sizes=a["sizes"] + b["sizes"], focal=FOCAL, Rs=a["Rs"] + b["Rs"], rigs=[3, 2], mask=mask,
                textures=a["textures"] + b["textures"], parts=(a, b))


def part(rig, r):
    """(first image, one past the last) of rig r of a joined rig."""
    first = np.concatenate([[0], np.cumsum(rig["rigs"])])
    return int(first[r]), int(first[r + 1])


# ---- the NumPy models in order -----------------------------------------------------------------------------------------------------------
ORB_KW = dict(grid=(1, 1), n_features=500)
MATCH_CONF = 0.3
_ORB = {}


def orb_of(view):
    """orb_np.find of one view, once a process (keyed by the pixels)."""
    from helpers import orb_np
    key = (view.shape, view.tobytes())
    if key not in _ORB:
        _ORB[key] = orb_np.find(view, orb_np.Params(**ORB_KW))
    return _ORB[key]


def model_chain(views, mask=None, rigs=None, swap_pair=None, centred=True, swap_matches=None):
    """orb_np.find -> match_np.match_model -> homography_np.find_homography_np -> estimator_np.estimate -> bundle_np.adjust and
    bundle_reproj_np.adjust -> bundle_reproj_np.wave_correct of each, at the classes' defaults.  Returns every intermediate a hand-off
    carries: sizes, feats, keypoints, descriptors, pairs, recs (the matcher's dicts), counts, points, hom (the homography's dicts), H, masks,
    stats, conf, and per stage of STAGES the model's tuple (cameras, kr32, ...).
    The negative controls: swap_pair = k feeds pair k's points to the homography with from and to exchanged; centred = False feeds
    keypoints as they are, without `pt - size / 2`; swap_matches = k feeds pair k's matches to the adjusters with queryIdx and trainIdx
    exchanged (the adjusters gather from keypoints and matches, not from the points: they undo a wrong start from the estimator)."""
    from helpers import bundle_np, bundle_reproj_np, estimator_np, homography_np, match_np
    feats = [orb_of(v) for v in views]
    sizes = [(int(v.shape[1]), int(v.shape[0])) for v in views]
    kps, descs = [f.keypoints for f in feats], [f.descriptors for f in feats]
    pairs = match_np.near_pairs([f.count for f in feats], mask)
    recs = match_np.match_model(descs, pairs, MATCH_CONF, kps, sizes if centred else [(0, 0)] * len(views))
    points = [r["points"] for r in recs]
    if swap_pair is not None:
        points = [p[:, [2, 3, 0, 1]].copy() if k == swap_pair else p for k, p in enumerate(points)]
    hom = [homography_np.find_homography_np(p) for p in points]
    n = len(pairs)
    counts = np.array([[r["count"] for r in recs]], np.int32)
    H = np.concatenate([h["H"] for h in hom]).reshape(3 * n, 3)
    stats = np.stack([h["stats"] for h in hom]).astype(np.int32)
    conf = np.array([[h["conf"] for h in hom]], np.float64)
    masks = [np.zeros((r["count"], 1), np.uint8) if h["mask"] is None else np.asarray(h["mask"], np.uint8).reshape(-1, 1) for r, h in zip(recs, hom)]
    first = None if rigs is None else [int(v) for v in np.concatenate([[0], np.cumsum(rigs)])]
    out = dict(sizes=sizes, feats=feats, keypoints=kps, descriptors=descs, pairs=pairs, recs=recs, counts=counts, points=points, hom=hom, H=H,
               masks=masks, stats=stats, conf=conf, rig_first=first)
    out["est"] = estimator_np.estimate(sizes, pairs, H, stats, first)
    ms = [r["matches"][:, [1, 0, 2]].copy() if k == swap_matches else r["matches"] for k, r in enumerate(recs)]
    args = (sizes, kps, pairs, ms, masks, counts, conf, out["est"][3], out["est"][0], first)
    out["ray"] = bundle_np.adjust(*args)
    out["reproj"] = bundle_reproj_np.adjust(*args)
    out["wave_ray"] = bundle_reproj_np.wave_correct(out["ray"][0], first, bundle_reproj_np.WAVE_HORIZ)
    out["wave_reproj"] = bundle_reproj_np.wave_correct(out["reproj"][0], first, bundle_reproj_np.WAVE_HORIZ)
    return out


@functools.lru_cache(maxsize=None)
def chain3():
    """model_chain of rig3(): shared, never written to."""
    return model_chain(rig3()["views"])


@functools.lru_cache(maxsize=None)
def chain3_plus_2():
    """model_chain of rig3_plus_2() with its mask and rigs.  Asserts first that without the mask every pair across the rigs has a
    confidence below 1: the mask is what keeps the rigs apart, not a lucky texture."""
    from helpers import homography_np, match_np
    rig = rig3_plus_2()
    feats = [orb_of(v) for v in rig["views"]]
    cross = [(i, j) for i in range(3) for j in range(3, 5)]
    recs = match_np.match_model([f.descriptors for f in feats], cross, MATCH_CONF, [f.keypoints for f in feats], rig["sizes"])
    cross_conf = [homography_np.find_homography_np(r["points"])["conf"] for r in recs]
    assert max(cross_conf) < 1.0, cross_conf
    out = model_chain(rig["views"], rig["mask"], rig["rigs"])
    out["cross_conf"] = cross_conf
    return out


# ---- the measures ---------------------------------------------------------------------------------------------------------------------------
def polar(R):
    """The rotation nearest R (u vt of its SVD, by np.linalg.svd in float64)."""
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64).reshape(3, 3))
    Q = u @ vt
    return -Q if np.linalg.det(Q) < 0 else Q


def cam_k(c):
    """CameraParams::K() of a camera row (focal, aspect, ppx, ppy, R[9], t[3])."""
    return k_of(c[0], (0, 0), c[1], c[2], c[3])


def cam_r(c):
    return np.asarray(c[4:13], np.float64).reshape(3, 3)


def rays_of(K, R, pts):
    """R K^-1 (x, y, 1) of points (m x 2), float64."""
    p = np.concatenate([np.asarray(pts, np.float64).reshape(-1, 2), np.ones((len(pts), 1))], 1)
    return p @ (np.asarray(R, np.float64).reshape(3, 3) @ np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))).T


def ray_angle(a, b):
    """The angle between rays, row by row: atan2(|a x b|, a . b)."""
    return np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum(1)), (a * b).sum(1))


def project(kind, scale, K, R, pts):
    """RotationWarper::warpPoint written out in float64 for points (m x 2): the ray R K^-1 (x, y, 1) to the panorama (u, v)."""
    r = rays_of(K, R, pts)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    if kind == "cylindrical":
        return np.stack([scale * np.arctan2(x, z), scale * y / np.sqrt(x * x + z * z)], 1)
    if kind == "spherical":
        return np.stack([scale * np.arctan2(x, z), scale * (np.pi - np.arccos(y / np.sqrt(x * x + y * y + z * z)))], 1)
    assert kind == "plane", kind
    return np.stack([scale * x / z, scale * y / z], 1)


def unproject(kind, scale, uv):
    """The ray of the panorama point (u, v) in the recovered world frame (... x 2 -> ... x 3): project's inverse."""
    u, v = np.asarray(uv[..., 0], np.float64) / scale, np.asarray(uv[..., 1], np.float64) / scale
    if kind == "cylindrical":
        return np.stack([np.sin(u), v, np.cos(u)], -1)
    if kind == "spherical":
        s = np.sin(np.pi - v)
        return np.stack([s * np.sin(u), np.cos(np.pi - v), s * np.cos(u)], -1)
    assert kind == "plane", kind
    return np.stack([u, v, np.ones_like(u)], -1)


def grid_pairs(planted, i, j):
    """The GRID_STEP grid of pixels p_i of view i whose planted ray falls at least INSIDE_PX inside view j, and where: (p_i, p_j)."""
    (wi, hi), (wj, hj) = planted["sizes"][i], planted["sizes"][j]
    xx, yy = np.meshgrid(np.arange(0.0, wi, GRID_STEP), np.arange(0.0, hi, GRID_STEP))
    pi = np.stack([xx.ravel(), yy.ravel()], 1)
    Ki, Kj = k_of(planted["focal"], (wi, hi)), k_of(planted["focal"], (wj, hj))
    ray = np.concatenate([pi, np.ones((len(pi), 1))], 1) @ (planted["Rs"][i] @ np.linalg.inv(Ki)).T
    q = ray @ (Kj @ planted["Rs"][j].T).T
    with np.errstate(all="ignore"):
        pj = q[:, :2] / q[:, 2:]
    keep = (q[:, 2] > 0) & (pj[:, 0] >= INSIDE_PX) & (pj[:, 0] <= wj - 1 - INSIDE_PX) & (pj[:, 1] >= INSIDE_PX) & (pj[:, 1] <= hj - 1 - INSIDE_PX)
    return pi[keep], pj[keep]


def all_pairs(planted, first=0, last=None):
    last = len(planted["Rs"]) if last is None else last
    return [(i, j) for i in range(first, last - 1) for j in range(i + 1, last)]


def misregistration(cameras, planted, kind, first=0, last=None):
    """For each pair (i, j) of the images first .. last - 1: (points, mean, max) of |project(i, p_i) - project(j, p_j)| over grid_pairs
    under the recovered `cameras` (n x 16 rows), in pixels of a panorama whose scale is the median recovered focal.  kind "angle" is the
    angle between the two rays times that scale: the one of these distances that a rotation common to all cameras leaves as it is (a
    panorama's own distances stretch away from its centre, so turning the rig changes them a little)."""
    cams = np.asarray(cameras, np.float64)
    last = len(cams) if last is None else last
    scale = float(np.median(cams[first:last, 0]))
    out = []
    for i, j in all_pairs(planted, first, last):
        pi, pj = grid_pairs(planted, i, j)
        if kind == "angle":
            d = scale * ray_angle(rays_of(cam_k(cams[i]), cam_r(cams[i]), pi), rays_of(cam_k(cams[j]), cam_r(cams[j]), pj))
        else:
            d = project(kind, scale, cam_k(cams[i]), cam_r(cams[i]), pi) - project(kind, scale, cam_k(cams[j]), cam_r(cams[j]), pj)
            d = np.sqrt((d * d).sum(1))
        out.append((len(d), float(d.mean()), float(d.max())))
    return out


def rotation_error_deg(cameras, planted, first=0, last=None):
    """Per pair, the angle in degrees between the recovered relative rotation polar(R_i)^T polar(R_j) and the planted R_i^T R_j."""
    cams = np.asarray(cameras, np.float64)
    last = len(cams) if last is None else last
    out = []
    for i, j in all_pairs(planted, first, last):
        rec = polar(cam_r(cams[i])).T @ polar(cam_r(cams[j]))
        D = rec.T @ (planted["Rs"][i].T @ planted["Rs"][j])
        out.append(float(np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0)))))
    return out


def focal_error(cameras, planted, first=0, last=None):
    """|recovered focal - planted| per camera."""
    cams = np.asarray(cameras, np.float64)
    last = len(cams) if last is None else last
    return [abs(float(cams[i, 0]) - planted["focal"]) for i in range(first, last)]


def measure(cameras, planted, first=0, last=None):
    """The worst of every measure over a rig: dict(focal, rot, mean_<kind>, max_<kind>)."""
    out = dict(focal=max(focal_error(cameras, planted, first, last)), rot=max(rotation_error_deg(cameras, planted, first, last)))
    for kind in KINDS + ("angle",):
        m = misregistration(cameras, planted, kind, first, last)
        out["mean_" + kind], out["max_" + kind] = max(v[1] for v in m), max(v[2] for v in m)
    return out


def within(got, measured):
    """Every figure of measure() at most BOUND_FACTOR x the recorded one; the list of those that are not."""
    return [(k, got[k], BOUND_FACTOR * measured[k]) for k in measured if not got[k] <= BOUND_FACTOR * measured[k]]


# ---- composition: the oracle's steps and the two figures ------------------------------------------------------------------------------------
# (kind, blend, the adjuster whose wave-corrected cameras compose): every kind with both blenders, both adjusters with every kind
COMPOSE_CASES = tuple((kind, blend, "ray") for kind in KINDS for blend in ("feather", "multiband"))
REPROJ_CASE = ("cylindrical", "feather", "reproj")


def planted_kr32(rig, first=0, last=None):
    """The planted cameras as the n x 18 float32 rows (K()[9], R[9]) a registration hands to the warper."""
    last = len(rig["Rs"]) if last is None else last
    return np.stack([np.concatenate([k_of(rig["focal"], rig["sizes"][i]).ravel(), rig["Rs"][i].ravel()]).astype(np.float32) for i in range(first, last)])


def oracle_warp(oracle, kind, scale, K, R, img):
    """(corner, warped image LINEAR / REFLECT, warped all-255 mask NEAREST / CONSTANT) by the oracle; the plane by tests/helpers/plane_np.py."""
    full = np.full(img.shape[:2], 255, np.uint8)
    if kind == "plane":
        from helpers import plane_np
        m = plane_np.from_rig(oracle, scale, K, R)
        c, wi, roi = m.warp(img, oracle.LINEAR, oracle.BORDER_REFLECT)
        _, wm, _ = m.warp(full, oracle.NEAREST, oracle.BORDER_CONSTANT, roi)
        return c, wi, wm
    k = {"cylindrical": oracle.CYL, "spherical": oracle.SPH}[kind]
    c, wi, _ = oracle.warp_u8(k, scale, K, R, img, oracle.LINEAR, oracle.BORDER_REFLECT)
    _, wm, _ = oracle.warp_u8(k, scale, K, R, full, oracle.NEAREST, oracle.BORDER_CONSTANT)
    return c, wi, wm


def compose_oracle(oracle, views, kr32, scale, kind, blend, gains=None):
    """The reference demo's post-registration stage on the oracle, step by step as tests/test_gpu_end_to_end.py chains it, for any number
    of tiles: warp image + mask with K32 / R32 of kr32, GainCompensator feed (tests/test_gain_model.py's feed_model; `gains` given: those
    instead) and apply, DP seam finder on copies of the masks, dilate 20 x 20 & warped mask, FeatherBlender 0.1 or MultiBandBlender(4 bands,
    I16).  Returns a dict of every step's outputs."""
    from oracle.dpseam_np import DpSeamFinder
    from test_gain_model import feed_model
    corners, warped, masks = [], [], []
    for v, row in zip(views, kr32):
        c, wi, wm = oracle_warp(oracle, kind, scale, row[0:9].reshape(3, 3), row[9:18].reshape(3, 3), v)
        corners.append(tuple(int(a) for a in c)); warped.append(wi); masks.append(wm)
    model = feed_model(corners, warped, masks)
    gains = model[5] if gains is None else gains
    applied = [oracle.gain_apply(w, float(g)) for w, g in zip(warped, gains)]
    seam = [m.copy() for m in masks]
    DpSeamFinder().find([a.astype(np.float32) for a in applied], corners, seam)
    sizes = [(a.shape[1], a.shape[0]) for a in applied]
    ob = oracle.Feather(0.1) if blend == "feather" else oracle.MultiBand(4, oracle.I16)
    ob.prepare(corners, sizes)
    fed = [oracle.dilate_rect(s, 20, 20) & m for s, m in zip(seam, masks)]
    for a, mk, c in zip(applied, fed, corners):
        ob.feed(a.astype(np.int16), mk, c)
    result, result_mask = ob.blend() if blend == "feather" else ob.blend(False)
    return dict(corners=corners, warped=warped, masks=masks, feed_model=model, gains=np.asarray(gains, np.float64), applied=applied, seam=seam,
                fed=fed, sizes=sizes, result=result, result_mask=result_mask, tl=(min(c[0] for c in corners), min(c[1] for c in corners)))


def gray(img):
    """The mean of the channels, float64."""
    return np.asarray(img, np.float64).mean(axis=2) if img.ndim == 3 else np.asarray(img, np.float64)


def overlap_agreement(corners, tiles, masks):
    """Per pair whose warped masks share a pixel: (i, j, pixels, mean |gray(tile_i) - gray(tile_j)| where both masks hold 255)."""
    out = []
    for i in range(len(tiles)):
        for j in range(i + 1, len(tiles)):
            x0, y0 = max(corners[i][0], corners[j][0]), max(corners[i][1], corners[j][1])
            x1 = min(corners[i][0] + tiles[i].shape[1], corners[j][0] + tiles[j].shape[1])
            y1 = min(corners[i][1] + tiles[i].shape[0], corners[j][1] + tiles[j].shape[0])
            if x0 >= x1 or y0 >= y1:
                continue
            sub = lambda a, k: a[y0 - corners[k][1]:y1 - corners[k][1], x0 - corners[k][0]:x1 - corners[k][0]]      # noqa: E731
            both = (sub(masks[i], i) == 255) & (sub(masks[j], j) == 255)
            if both.any():
                out.append((i, j, int(both.sum()), float(np.abs(gray(sub(tiles[i], i)) - gray(sub(tiles[j], j)))[both].mean())))
    return out


def erode(mask, r):
    """The mask eroded by a (2 r + 1)-square, pixels outside the mat counting as 0: boolean."""
    m = np.pad(np.asarray(mask) > 0, r)
    h, w = mask.shape
    rows = np.logical_and.reduce([m[:, r + d:r + d + w] for d in range(-r, r + 1)])
    return np.logical_and.reduce([rows[r + d:r + d + h] for d in range(-r, r + 1)])


def ground_truth_error(result, result_mask, tl, kind, scale, G, texture):
    """The panorama against the texture rendered directly into the panorama's frame: a pixel (col, row) is the panorama point
    (tl.x + col, tl.y + row), its ray unproject(...) in the recovered frame, G times that in the planted one.  Over the pixels of the
    result mask eroded by ERODE_PX - the only ones dropped -: (the mean absolute gray error, the share of the mask's pixels kept)."""
    h, w = result_mask.shape
    keep = erode(result_mask, ERODE_PX)
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64) + tl[0], np.arange(h, dtype=np.float64) + tl[1])
    rays = unproject(kind, scale, np.stack([uu, vv], -1)) @ np.asarray(G, np.float64).T
    val, inside = lookup(texture, rays)
    assert inside[keep].all(), "ground truth: a ray of the panorama leaves the texture"
    err = np.abs(gray(result) - gray(val))[keep]
    return float(err.mean()), float(keep.sum()) / float((np.asarray(result_mask) > 0).sum())


def alignment(rig, cameras, centre):
    """G = R_planted[c] polar(R_rec[c])^T: the recovered world frame in the planted one, fixed at the estimator's centre c."""
    return rig["Rs"][centre] @ polar(cam_r(np.asarray(cameras, np.float64)[centre])).T


def compose_figures(oracle, rig, c, kind, blend, adjuster):
    """The oracle composition of rig3-like `rig` from the model chain c's wave-corrected cameras of `adjuster`, and once from the planted
    cameras: dict(overlap, gt, share, gt_planted, run) - `run` the compose_oracle dict of the recovered cameras."""
    cams, kr32 = c["wave_" + adjuster][0], c["wave_" + adjuster][1]
    scale = float(np.median(cams[:, 0]))
    run = compose_oracle(oracle, rig["views"], kr32, scale, kind, blend)
    centre = int(c["est"][3][0, 2])
    gt, share = ground_truth_error(run["result"], run["result_mask"], run["tl"], kind, scale, alignment(rig, cams, centre), rig["texture"])
    overlap = max(v[3] for v in overlap_agreement(run["corners"], run["applied"], run["masks"]))
    ref = compose_oracle(oracle, rig["views"], planted_kr32(rig), rig["focal"], kind, blend)
    gt_planted, _ = ground_truth_error(ref["result"], ref["result_mask"], ref["tl"], kind, rig["focal"], np.eye(3), rig["texture"])
    return dict(overlap=overlap, gt=gt, share=share, gt_planted=gt_planted, run=run, scale=scale)


# ---- recorded ----------------------------------------------------------------------------------------------------------------------------
# python tests/pano_cases.py prints these literals.  RECORDED (rig3_plus_2(): its first three images and pairs are rig3()'s) is held exactly;
# MEASURED is measure() of the model chain per stage, every bound BOUND_FACTOR x its entry; COMPOSED is compose_figures() on the CPU oracle
# per case: the bound on `overlap` and `gt` is COMPOSE_FACTOR x the entry, and gt must stay below 2 gt_planted + overlap.
COMPOSE_FACTOR, MIN_SHARE = 1.5, 0.8
RECORDED = dict(keypoints=[450, 440, 457, 475, 462], pairs=[(0, 1), (0, 2), (1, 2), (3, 4)], matches=[151, 103, 226, 232], inliers=[131, 82, 209, 217],
                conf=[2.4577861163227017, 2.107969151670951, 2.757255936675462, 2.79639175257732])
MEASURED = {
    'rig3': {
        'est': {'focal': 23.5071, 'rot': 0.4759, 'mean_cylindrical': 0.3275, 'max_cylindrical': 1.1349, 'mean_spherical': 0.3178, 'max_spherical': 1.0533, 'mean_plane': 0.3582, 'max_plane': 1.4587, 'mean_angle': 0.314, 'max_angle': 1.0343},
        'ray': {'focal': 2.3329, 'rot': 0.1579, 'mean_cylindrical': 0.1379, 'max_cylindrical': 0.3272, 'mean_spherical': 0.1345, 'max_spherical': 0.3053, 'mean_plane': 0.1462, 'max_plane': 0.4183, 'mean_angle': 0.1331, 'max_angle': 0.2972},
        'reproj': {'focal': 7.6388, 'rot': 0.715, 'mean_cylindrical': 0.1566, 'max_cylindrical': 0.4252, 'mean_spherical': 0.1526, 'max_spherical': 0.4196, 'mean_plane': 0.1666, 'max_plane': 0.5135, 'mean_angle': 0.1514, 'max_angle': 0.4079},
        'wave_ray': {'focal': 2.3329, 'rot': 0.1579, 'mean_cylindrical': 0.1385, 'max_cylindrical': 0.316, 'mean_spherical': 0.1348, 'max_spherical': 0.302, 'mean_plane': 0.1466, 'max_plane': 0.3948, 'mean_angle': 0.1331, 'max_angle': 0.2972},
        'wave_reproj': {'focal': 7.6388, 'rot': 0.715, 'mean_cylindrical': 0.1574, 'max_cylindrical': 0.4369, 'mean_spherical': 0.1525, 'max_spherical': 0.4274, 'mean_plane': 0.1683, 'max_plane': 0.5483, 'mean_angle': 0.1514, 'max_angle': 0.4079},
    },
    'rig2': {
        'est': {'focal': 38.4632, 'rot': 0.1549, 'mean_cylindrical': 0.2865, 'max_cylindrical': 0.766, 'mean_spherical': 0.2663, 'max_spherical': 0.6821, 'mean_plane': 0.3004, 'max_plane': 0.8012, 'mean_angle': 0.2661, 'max_angle': 0.682},
        'ray': {'focal': 3.9223, 'rot': 0.1224, 'mean_cylindrical': 0.102, 'max_cylindrical': 0.333, 'mean_spherical': 0.0997, 'max_spherical': 0.3051, 'mean_plane': 0.1077, 'max_plane': 0.3512, 'mean_angle': 0.0986, 'max_angle': 0.3041},
        'reproj': {'focal': 25.4209, 'rot': 0.6873, 'mean_cylindrical': 0.1904, 'max_cylindrical': 0.6918, 'mean_spherical': 0.1817, 'max_spherical': 0.6509, 'mean_plane': 0.2042, 'max_plane': 0.7687, 'mean_angle': 0.1795, 'max_angle': 0.634},
        'wave_ray': {'focal': 3.9223, 'rot': 0.1224, 'mean_cylindrical': 0.1024, 'max_cylindrical': 0.3117, 'mean_spherical': 0.1003, 'max_spherical': 0.3043, 'mean_plane': 0.1079, 'max_plane': 0.3346, 'mean_angle': 0.0986, 'max_angle': 0.3041},
        'wave_reproj': {'focal': 25.4209, 'rot': 0.6873, 'mean_cylindrical': 0.1961, 'max_cylindrical': 0.6496, 'mean_spherical': 0.1828, 'max_spherical': 0.638, 'mean_plane': 0.2107, 'max_plane': 0.7328, 'mean_angle': 0.1795, 'max_angle': 0.634},
    },
}
COMPOSED = {
    ('cylindrical', 'feather', 'ray'): {'overlap': 2.5067, 'gt': 6.4067, 'gt_planted': 3.1449, 'share': 0.8943},
    ('cylindrical', 'multiband', 'ray'): {'overlap': 2.5067, 'gt': 6.5037, 'gt_planted': 3.6183, 'share': 0.8943},
    ('spherical', 'feather', 'ray'): {'overlap': 2.5077, 'gt': 6.4099, 'gt_planted': 3.149, 'share': 0.891},
    ('spherical', 'multiband', 'ray'): {'overlap': 2.5077, 'gt': 6.5045, 'gt_planted': 3.6266, 'share': 0.891},
    ('plane', 'feather', 'ray'): {'overlap': 2.5238, 'gt': 6.7585, 'gt_planted': 3.1264, 'share': 0.9027},
    ('plane', 'multiband', 'ray'): {'overlap': 2.5238, 'gt': 6.805, 'gt_planted': 3.638, 'share': 0.9027},
    ('cylindrical', 'feather', 'reproj'): {'overlap': 2.6276, 'gt': 11.4533, 'gt_planted': 3.1449, 'share': 0.8913},
}


def main():
    """Print RECORDED, MEASURED and COMPOSED as the literals above: NumPy models and the CPU oracle only."""
    c, rig, c5, rig5 = chain3(), rig3(), chain3_plus_2(), rig3_plus_2()
    print("RECORDED = dict(keypoints=%r, pairs=%r, matches=%r, inliers=%r,\n                conf=%r)" % (
        [f.count for f in c5["feats"]], c5["pairs"], c5["counts"][0].tolist(), c5["stats"][:, 1].tolist(), [float(v) for v in c5["conf"][0]]))
    print("cross-rig conf", c5["cross_conf"])
    print("MEASURED = {")
    for name, cams, r, a, b in (("rig3", c, rig, 0, 3), ("rig2", c5, rig5, 3, 5)):
        print("    %r: {" % name)
        for s in STAGES:
            print("        %r: %r," % (s, {k: round(v, 4) for k, v in measure(cams[s][0], r, a, b).items()}))
        print("    },")
    print("}")
    from oracle import capi
    capi.lib()
    print("COMPOSED = {")
    for case in COMPOSE_CASES + (REPROJ_CASE,):
        f = compose_figures(capi, rig, c, *case)
        print("    %r: %r," % (case, {k: round(f[k], 4) for k in ("overlap", "gt", "gt_planted", "share")}))
    print("}")


if __name__ == "__main__":
    main()
