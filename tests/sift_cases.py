"""Images for the SIFT finder's tests (tests/test_sift_model.py, tests/test_gpu_sift.py, tools/fuzz_sift.py): plain NumPy, deterministic,
and the model's answer to each, computed once a process."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import pano_cases  # noqa: E402
from helpers import sift_np as M  # noqa: E402


def noise(h, w, seed, smooth=0):
    """uniform noise, box-smoothed `smooth` times: uint8 h x w"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 255, (h, w))
    for _ in range(smooth):
        p = np.pad(img, 1, mode="edge")
        img = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + p[1:-1, 1:-1]) / 5.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def blob(s_b, side=96, centre=(47.75, 47.75), contrast=80.0, ground=110.0, s_y=None):
    """one Gaussian blob of standard deviation s_b (s_y down the rows, where given) on a flat field.  The centre sits on a pixel of the
    doubled image, (2 x + 0.5, 2 y + 0.5) = (96, 96), which every octave of the test keeps (96 = 4 * 24); between pixels the extremum would be
    a tie of four."""
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    sy = s_b if s_y is None else s_y
    g = np.exp(-((yy - centre[1]) ** 2 / (2 * sy * sy) + (xx - centre[0]) ** 2 / (2 * s_b * s_b)))
    return np.clip(np.rint(ground + contrast * g), 0, 255).astype(np.uint8)


# standard deviations that put the extremum in layers 1, 2, 3 of octaves -1, 0 and 1 (found with the model; tests/test_sift_model.py asserts it)
BLOBS = {(-1, 1): 1.1, (-1, 2): 1.4, (-1, 3): 1.8, (0, 1): 2.25, (0, 2): 2.8, (0, 3): 3.6, (1, 1): 4.5, (1, 2): 5.6, (1, 3): 7.2}


def edge_blob_top():
    """a blob whose extremum sits at r = 5 of octave -1: source row 2.25 (doubled row 5)"""
    return blob(1.4, side=48, centre=(23.75, 2.25))


def edge_blob_bottom():
    """a blob whose extremum sits at r = rows - 6 of octave -1: 48 rows double to 96, row 90 is source row 44.75"""
    return blob(1.4, side=48, centre=(23.75, 44.75))


def two_lobes():
    """an elongated blob: gradients point at its long axis from both sides, two orientation peaks half a turn apart"""
    return blob(2.0, s_y=4.5)


def straight_edge():
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    return np.clip(np.rint(110 + 80 / (1 + np.exp(-(xx - 31.75)))), 0, 255).astype(np.uint8)


def rig_view(i=0, channels=3):
    v = pano_cases.rig3()["views"][i]
    if channels == 3:
        return v
    if channels == 1:
        return M.gray(v)
    return np.ascontiguousarray(np.concatenate([v, np.full(v.shape[:2] + (1,), 200 + i, np.uint8)], axis=2))


DUP_CASE = (16, 1, 2)               # (side, seed, smoothing) of the smallest noise image in which two starting pixels end on one point

CASES = {
    # name: (image, Params keywords)
    "rig-bgr": (lambda: rig_view(0, 3), {}),
    "rig-gray": (lambda: rig_view(1, 1), {}),
    "rig-bgra": (lambda: rig_view(2, 4), {}),
    "side-1": (lambda: noise(1, 1, 1), dict(contrast_threshold=0.0)),
    "side-5": (lambda: noise(5, 5, 2), dict(contrast_threshold=0.0)),
    "side-6": (lambda: noise(6, 6, 3), dict(contrast_threshold=0.0)),
    "side-7": (lambda: noise(7, 7, 4), dict(contrast_threshold=0.0)),
    "strip-6x200": (lambda: noise(6, 200, 5, 1), dict(contrast_threshold=0.0)),
    "strip-200x6": (lambda: noise(200, 6, 6, 1), dict(contrast_threshold=0.0)),
    "odd-33x47": (lambda: noise(33, 47, 7, 2), dict(contrast_threshold=0.01)),
    "two-lobes": (two_lobes, {}),
    "edge-blob-top": (edge_blob_top, {}),
    "edge-blob-bottom": (edge_blob_bottom, {}),
    "straight-edge": (straight_edge, dict(contrast_threshold=0.0)),
    "contrast-0": (lambda: noise(40, 56, 8, 2), dict(contrast_threshold=0.0)),
    "contrast-huge": (lambda: rig_view(0, 1), dict(contrast_threshold=1e30)),
    "edge-1e-3": (lambda: noise(40, 56, 8, 2), dict(contrast_threshold=0.0, edge_threshold=1e-3)),
    "edge-1e6": (lambda: noise(40, 56, 8, 2), dict(contrast_threshold=0.0, edge_threshold=1e6)),
    "nfeatures-1": (lambda: rig_view(1, 1), dict(nfeatures=1)),
    "duplicates": (lambda: noise(DUP_CASE[0], DUP_CASE[0], DUP_CASE[1], DUP_CASE[2]), dict(contrast_threshold=0.0)),
    "flat": (lambda: np.full((64, 80), 90, np.uint8), dict(contrast_threshold=0.0)),
}
for _k, _s in BLOBS.items():
    CASES["blob-%d-%d" % _k] = ((lambda s=_s: blob(s)), {})
CASES["blob-dark"] = (lambda: blob(2.8, contrast=-80.0), {})


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name][0]()
    img.setflags(write=False)
    return img


def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def want(name, cap=None, nfeatures=None):
    """the model's answer (a dict of read-only arrays), computed once"""
    kw = dict(CASES[name][1])
    if nfeatures is not None:
        kw["nfeatures"] = nfeatures
    return _frozen(M.find(image(name), M.Params(**kw), cap))


@functools.lru_cache(maxsize=None)
def traced(name):
    """(answer, trace) of a case"""
    t = {}
    r = _frozen(M.find(image(name), M.Params(**CASES[name][1]), None, t))
    return r, t


# ---- the planted rig through the SIFT model chain ------------------------------------------------------------------------------------------
MATCH_CONF = 0.3                # BestOf2NearestMatcher's default, as the SURF chain has it
RIG_CONTRAST = 0.04             # the class default
_FEATS = {}


def sift_of(view, contrast_threshold=RIG_CONTRAST):
    """sift_np.find of one view at the class defaults (and the given threshold), once a process (keyed by the pixels)."""
    key = (view.shape, view.tobytes(), float(contrast_threshold))
    if key not in _FEATS:
        _FEATS[key] = _frozen(M.find(view, M.Params(contrast_threshold=contrast_threshold)))
    return _FEATS[key]


def model_chain(views, centred=True, contrast_threshold=RIG_CONTRAST):
    """pano_cases.model_chain with three stages replaced: sift_np.find -> match_f32_np.match_model -> homography_np.find_homography_np, then
    estimator_np.estimate -> bundle_np.adjust as there.  centred = False is the negative control: keypoints fed as pt, not pt - size / 2."""
    from helpers import bundle_np, estimator_np, homography_np, match_f32_np, match_np
    feats = [sift_of(v, contrast_threshold) for v in views]
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


# ---- more candidates than ISX_SIFT_MAX_CANDIDATES ------------------------------------------------------------------------------------------
# the smallest lattice (in whole periods) that passes the limit at contrast_threshold 0: 32868 candidates on 810 x 810, 32442 on 805 x 805
DROPPED_SIDE, DROPPED_STEP = 810, 5


def dots(side, seed=1, period=5, s=1.1):
    """a lattice of small blobs of either contrast, one every `period` pixels: about one candidate a blob at contrast_threshold 0, far denser
    than white noise, which stays below the limit up to ISX_SIFT_MAX_PIXELS (1347 candidates on 700 x 700)"""
    rng = np.random.default_rng(seed)
    n = side // period
    centres = np.arange(n) * period + period / 2.0 - 0.25
    amp = rng.uniform(40, 100, (n, n)) * rng.choice((-1.0, 1.0), (n, n))
    g = np.exp(-((np.arange(side)[:, None] - centres[None, :]) ** 2) / (2 * s * s))
    return np.clip(np.rint(110 + g @ amp @ g.T), 0, 255).astype(np.uint8)
