"""Images for the SURF finder's tests (tests/test_surf_model.py, tests/test_gpu_surf.py, tools/fuzz_surf.py): plain NumPy, deterministic,
and the model's answer to each, computed once a process."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import pano_cases  # noqa: E402
from helpers import surf_np as M  # noqa: E402


def blobs(h, w, seed, sigmas, count, noise=3.0, ground=110.0, centres=None):
    """`count` isotropic Gaussian blobs of either contrast, sigma drawn from `sigmas`, on a flat ground with a little noise: uint8 h x w"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), ground)
    for k in range(count):
        cy, cx = (rng.uniform(0, h), rng.uniform(0, w)) if centres is None else centres[k]
        s = float(sigmas[int(rng.integers(0, len(sigmas)))])
        amp = float(rng.choice((-1.0, 1.0))) * rng.uniform(50, 100)
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    img += rng.normal(0, noise, (h, w)) if noise else 0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def blob1(contrast=80.0, sigma=4.0, side=96):
    """one blob of sigma 4 on pixel (48, 48) of a flat 96 x 96 ground (between four pixels its maximum would be a four-way tie, which the strict
    test of the 26 neighbours rejects)"""
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    c = float(side // 2)
    return np.clip(np.rint(110.0 + contrast * np.exp(-((yy - c) ** 2 + (xx - c) ** 2) / (2 * sigma * sigma))), 0, 255).astype(np.uint8)


def rig_view(i=0, channels=3):
    v = pano_cases.rig3()["views"][i]
    if channels == 3:
        return v
    if channels == 1:
        return M.gray(v)
    return np.ascontiguousarray(np.concatenate([v, np.full(v.shape[:2] + (1,), 200 + i, np.uint8)], axis=2))


def large_blobs():
    """480 x 400 (rows x cols), blobs of sigma 10 - 28: sizes in the top octave, the long-window path"""
    return blobs(480, 400, 5, (10, 14, 20, 28), 14, noise=1.5)


def border_blobs():
    """blobs whose centres lie 11 px inside each border of a 150 x 170 image - the nearest a maximum of the 15-filter can lie is 10 - and a
    few inside: the descriptor window and the orientation disc of the outer ones leave the image"""
    h, w = 150, 170
    centres = [(11, x) for x in (30, 75, 120)] + [(h - 12, x) for x in (40, 90, 140)] + [(y, 11) for y in (40, 90)] + [(y, w - 12) for y in (50, 100)] + \
              [(60, 70), (85, 110)]
    return blobs(h, w, 9, (2.5,), len(centres), noise=1.0, centres=centres)


CASES = {
    # name: (image, Params keywords)
    "rig-bgr": (lambda: rig_view(0, 3), {}),
    "rig-gray": (lambda: rig_view(1, 1), {}),
    "rig-bgra": (lambda: rig_view(2, 4), {}),
    "side-1": (lambda: blobs(1, 1, 1, (2,), 1), {}),
    "side-8": (lambda: blobs(8, 8, 2, (2,), 2), {}),
    "side-9": (lambda: blobs(9, 9, 3, (2,), 2), {}),
    "side-14": (lambda: blobs(14, 14, 4, (2,), 3), {}),
    "side-15": (lambda: blobs(15, 15, 5, (2,), 3), {}),
    "side-39": (lambda: blobs(39, 39, 6, (2, 3), 8), dict(hess_thresh=50.0)),
    "side-40": (lambda: blobs(40, 40, 7, (2, 3), 8), dict(hess_thresh=50.0)),
    "strip-33x200": (lambda: blobs(33, 200, 8, (2, 3), 14), dict(hess_thresh=50.0)),
    "strip-200x33": (lambda: blobs(200, 33, 8, (2, 3), 14), dict(hess_thresh=50.0)),
    "large-blobs": (large_blobs, {}),
    "large-blobs-4-octaves": (large_blobs, dict(num_octaves=4)),
    "border": (border_blobs, dict(hess_thresh=100.0)),
    "octaves-1": (lambda: rig_view(0, 1), dict(num_octaves=1)),
    "octaves-4": (lambda: rig_view(0, 1), dict(num_octaves=4)),
    "layers-1": (lambda: rig_view(1, 1), dict(num_layers=1)),
    "layers-4-octaves-1": (lambda: rig_view(1, 1), dict(num_layers=4, num_octaves=1)),
    "thresh-huge": (lambda: rig_view(0, 1), dict(hess_thresh=1e30)),
    "thresh-0": (lambda: blobs(72, 88, 11, (2, 3, 5), 12, noise=2.0), dict(hess_thresh=0.0)),
    "flat": (lambda: np.full((64, 80), 90, np.uint8), dict(hess_thresh=0.0)),
}


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name][0]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want(name, cap=None):
    """the model's answer (a dict of read-only arrays), computed once"""
    r = M.find(image(name), M.Params(**CASES[name][1]), cap)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the planted rig through the SURF model chain ------------------------------------------------------------------------------------------
MATCH_CONF = 0.3                # BestOf2NearestMatcher's default
_FEATS = {}


def surf_of(view, hess_thresh=300.0):
    """surf_np.find of one view at the class defaults (and the given threshold), once a process (keyed by the pixels)."""
    key = (view.shape, view.tobytes(), float(hess_thresh))
    if key not in _FEATS:
        _FEATS[key] = M.find(view, M.Params(hess_thresh=hess_thresh))
    return _FEATS[key]


def model_chain(views, centred=True, hess_thresh=300.0):
    """pano_cases.model_chain with three stages replaced: surf_np.find -> match_f32_np.match_model -> homography_np.find_homography_np, then
    estimator_np.estimate -> bundle_np.adjust as there.  centred = False is the negative control: keypoints fed as pt, not pt - size / 2."""
    from helpers import bundle_np, estimator_np, homography_np, match_f32_np, match_np
    feats = [surf_of(v, hess_thresh) for v in views]
    sizes = [(int(v.shape[1]), int(v.shape[0])) for v in views]
    kps, descs = [f["keypoints"] for f in feats], [f["descriptors"] for f in feats]
    pairs = match_np.near_pairs([f["count"] for f in feats])
    recs = match_f32_np.match_model(descs, pairs, MATCH_CONF, kps, sizes if centred else [(0, 0)] * len(views))
    points = [r["points"] for r in recs]
    hom = [homography_np.find_homography_np(p) for p in points]
    n = len(pairs)
    counts = np.array([[r["count"] for r in recs]], np.int32)
    H = np.concatenate([h["H"] for h in hom]).reshape(3 * n, 3)
    stats = np.stack([h["stats"] for h in hom]).astype(np.int32)
    conf = np.array([[h["conf"] for h in hom]], np.float64)
    masks = [np.zeros((r["count"], 1), np.uint8) if h["mask"] is None else np.asarray(h["mask"], np.uint8).reshape(-1, 1) for r, h in zip(recs, hom)]
    out = dict(sizes=sizes, feats=feats, keypoints=kps, descriptors=descs, pairs=pairs, recs=recs, counts=counts, points=points, hom=hom, H=H, masks=masks,
               stats=stats, conf=conf)
    out["est"] = estimator_np.estimate(sizes, pairs, H, stats, None)
    out["ray"] = bundle_np.adjust(sizes, kps, pairs, [r["matches"] for r in recs], masks, counts, conf, out["est"][3], out["est"][0], None)
    return out


@functools.lru_cache(maxsize=None)
def chain3():
    """model_chain of pano_cases.rig3(): shared, never written to."""
    return model_chain(pano_cases.rig3()["views"])
