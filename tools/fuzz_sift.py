"""Randomised parity of the SIFT finder (isx_sift_find) against its NumPy model (tests/helpers/sift_np.py): count, status, keypoints, meta
and descriptors with np.array_equal, and rows from the count on untouched.

    python tools/fuzz_sift.py --seconds 120 --seed 20261221 [--out profiles/fuzz_sift_120s.json]

The generator (no GPU needed: tests/test_sift_fuzz_generator.py checks it).  case(seed, cls) draws one of CLASSES, each sitting on a
constant of the algorithm or of the kernels:
    tiles         a side whose double is a multiple of the blur kernels' 64 x 4 tile, one pixel less or one more, the other side free
    octaves       a side at which an octave appears: the integer octave rule's steps (3, 6, 12, 23, 46 and 91 source pixels) and the
                  11-pixel rule's (an octave 10 or 11 wide), one less or one more
    border        small blobs whose centres lie 2 .. 4 px inside a border: the extremum sits on the first or last searched rows and columns
                  and the orientation and descriptor windows leave the image
    cap           a scene of many blobs; cap is 1, count - 1, count or count + 1 (the model's count), or nfeatures is
    params        1, 3 or 4 channels, contrast_threshold from {0, 0.01, 0.04, 0.2, 1e30}, edge_threshold from {1e-3, 2, 10, 1e6}, nfeatures 0, 1 or 5
Layouts: host or device mats, the image dense or at an odd byte offset with an odd pitch, the outputs dense or with padded rows."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from helpers import sift_np as M  # noqa: E402

CLASSES = ("tiles", "octaves", "border", "cap", "params")
CONTRASTS = (0.0, 0.01, 0.04, 0.2, 1e30)
EDGES = (1e-3, 2.0, 10.0, 1e6)
SENTINEL = -7777.0
MAX_SIDE = 120                # of a generated image: the model takes a fraction of a second
TILE_SIDES = (32, 64, 96)     # their doubles are multiples of the 64-wide tile; every side's double is a multiple of the 4-high one
# the sides at which the octave count steps (2 side >= 2^c sqrt 2) and at which an octave is 11 wide (2 side >> k == 11)
OCTAVE_SIDES = (3, 6, 12, 23, 46, 91, 11, 22, 44, 88)


def scene(rng, h, w, centres, sigmas, noise):
    """Gaussian blobs of either contrast on a flat ground, a little noise: uint8 h x w"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), float(rng.integers(90, 140)))
    for (cy, cx), s in zip(centres, sigmas):
        amp = float(rng.choice((-1.0, 1.0))) * rng.uniform(40, 90)
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
    if noise:
        img += rng.normal(0, noise, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def case(seed, cls=None):
    """One case: dict(cls, image, params (keywords of sift_np.Params), cap_rule, layout_seed, and what the class planted)."""
    rng = np.random.default_rng(seed)
    cls = cls or CLASSES[int(rng.integers(len(CLASSES)))]
    params, cap_rule, extra, channels = dict(contrast_threshold=float(rng.choice((0.01, 0.04)))), "room", {}, 1
    if cls in ("tiles", "octaves"):
        table = TILE_SIDES if cls == "tiles" else OCTAVE_SIDES
        side = max(int(table[int(rng.integers(len(table)))]) + int(rng.integers(-1, 2)), 1)
        other = int(rng.integers(max(6, side // 2), MAX_SIDE + 1))
        h, w = (side, other) if rng.random() < 0.5 else (other, side)
        n = int(rng.integers(3, 12))
        centres = [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(n)]
        sigmas = [float(rng.choice((1.2, 1.8, 2.5, 3.5, 5.0))) for _ in range(n)]
        extra = dict(side=side)
        params["contrast_threshold"] = float(rng.choice((0.0, 0.01)))
    elif cls == "border":
        h, w = int(rng.integers(30, 101)), int(rng.integers(30, 101))
        centres = []
        for _ in range(int(rng.integers(4, 10))):
            d, along = float(rng.integers(2, 5)) + 0.25, rng.random()
            centres.append([(d, along * w), (h - 1 - d, along * w), (along * h, d), (along * h, w - 1 - d)][int(rng.integers(4))])
        sigmas = [float(rng.choice((1.2, 1.5)))] * len(centres)
        extra = dict(centres=centres)
        params["contrast_threshold"] = 0.01
    elif cls == "cap":
        h, w = int(rng.integers(60, 121)), int(rng.integers(60, 121))
        n = int(rng.integers(10, 25))
        centres = [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(n)]
        sigmas = [float(rng.choice((1.5, 2.5, 4.0))) for _ in range(n)]
        cap_rule = ("one", "count-1", "count", "count+1", "nf-1", "nf+1")[int(rng.integers(6))]
    else:
        h, w = int(rng.integers(20, 121)), int(rng.integers(20, 121))
        n = int(rng.integers(4, 14))
        centres = [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(n)]
        sigmas = [float(rng.choice((1.5, 2.5, 5.0, 8.0))) for _ in range(n)]
        channels = int(rng.choice((1, 3, 4)))
        params = dict(contrast_threshold=float(CONTRASTS[int(rng.integers(len(CONTRASTS)))]), edge_threshold=float(EDGES[int(rng.integers(len(EDGES)))]),
                      nfeatures=int(rng.choice((0, 1, 5))))
    img = scene(rng, h, w, centres, sigmas, float(rng.choice((0.0, 1.0, 2.5))))
    if channels > 1:
        img = np.stack([np.clip(img.astype(np.int64) + int(rng.integers(-20, 21)), 0, 255).astype(np.uint8) for _ in range(channels)], axis=2)
    return dict(cls=cls, image=np.ascontiguousarray(img), params=params, cap_rule=cap_rule, layout_seed=int(rng.integers(1 << 30)), **extra)


def cap_of(rule, count):
    return {"room": count + 3, "one": 1, "count-1": max(count - 1, 1), "count": max(count, 1), "count+1": count + 1, "nf-1": count + 3, "nf+1": count + 3}[rule]


def expected(c):
    """(cap, nfeatures, the model's answer under them)"""
    full = M.find(c["image"], M.Params(**c["params"]))
    cap = cap_of(c["cap_rule"], full["count"])
    nf = c["params"].get("nfeatures", 0)
    if c["cap_rule"] in ("nf-1", "nf+1"):
        nf = max(full["count"] + (-1 if c["cap_rule"] == "nf-1" else 1), 1)
        full = M.find(c["image"], M.Params(**dict(c["params"], nfeatures=nf)))
    n = min(cap, full["count"])
    return cap, nf, dict(count=n, status=full["status"] | (M.STATUS_TRUNCATED if full["count"] > cap else 0), keypoints=full["keypoints"][:n], meta=full["meta"][:n],
                         descriptors=full["descriptors"][:n])


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
def _place_image(rng, img, device, strided):
    import torch
    h, w = img.shape[:2]
    cn = 1 if img.ndim == 2 else img.shape[2]
    if not strided:
        return torch.from_numpy(img.copy()).cuda() if device else img.copy()
    pitch = w * cn + int(rng.choice((1, 3, 8)))
    raw = np.full(1 + h * pitch + 8, 0xA5, np.uint8)
    shape, strides = ((h, w), (pitch, 1)) if img.ndim == 2 else ((h, w, cn), (pitch, cn, 1))
    view = np.lib.stride_tricks.as_strided(raw[1:], shape, strides)
    view[...] = img
    if device:
        return torch.as_strided(torch.from_numpy(raw).cuda(), shape, strides, 1)
    return view


def run_case(c, rng=None):
    """Runs one case through the library in a random layout and compares with the model.  Returns a list of differences (empty: equal)."""
    import torch
    from fuzz_match import _place
    from imagestitch_amd import features
    rng = rng or np.random.default_rng(c["layout_seed"])
    cap, nf, want = expected(c)
    device = bool(rng.random() < 0.6)
    image = _place_image(rng, c["image"], device, bool(rng.random() < 0.5))
    outs = [_place(rng, np.full((cap + int(rng.integers(0, 3)), cols), SENTINEL, np.float32), device, bool(rng.random() < 0.5)) for cols in (2, 5, 128)]
    k = int(rng.integers(3))
    outs[k] = _place(rng, np.full((cap, (2, 5, 128)[k]), SENTINEL, np.float32), device, bool(rng.random() < 0.5))      # the smallest row count is the cap
    cs = _place(rng, np.full((1, 2), -7777, np.int32), device, False)
    q = features.sift_default_params()
    q.nfeatures, q.contrast_threshold, q.edge_threshold = nf, c["params"]["contrast_threshold"], c["params"].get("edge_threshold", 10.0)
    stream = torch.cuda.current_stream()
    features.sift_find(image, q, outs[0][0], outs[1][0], outs[2][0], cs[0], 0, stream)
    stream.synchronize()
    got_cs = cs[1]()[0]
    bad = []
    if int(got_cs[0]) != want["count"] or int(got_cs[1]) != want["status"]:
        return ["count %d status %d, the model %d and %d" % (got_cs[0], got_cs[1], want["count"], want["status"])]
    n = want["count"]
    for (mat, back), name in zip(outs, ("keypoints", "meta", "descriptors")):
        got = back()
        if not np.array_equal(got[:n], want[name]):
            bad.append("%s differ in %d rows of %d" % (name, int((got[:n] != want[name]).any(axis=1).sum()), n))
        if not (got[n:] == SENTINEL).all():
            bad.append("%s: rows from the count on were written" % name)
    return bad


def scheduled(seed, n):
    """(case seed, class) of a soak's n-th case: the classes in turn."""
    return int(seed) * 1000003 + n, CLASSES[n % len(CLASSES)]


def run(seconds, seed, verbose=False, progress_path=None):
    """Draws cases (the classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    per, failing, n, keypoints, told = {c: 0 for c in CLASSES}, [], 0, 0, t0
    while time.time() - t0 < seconds:
        if progress_path and time.time() - told >= 30.0:
            told = time.time()
            with open(progress_path, "w") as f:
                json.dump(dict(seconds=round(told - t0, 1), cases=n, mismatches=len(failing)), f)
        s, cls = scheduled(seed, n)
        c = case(s, cls)
        bad = run_case(c)
        per[cls] += 1
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=cls, shape=list(c["image"].shape), params=c["params"], differences=bad[:4]))
            if verbose:
                print("MISMATCH", s, cls, c["image"].shape, c["params"], bad[:4], flush=True)
    return dict(tool="fuzz_sift", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, mismatches=len(failing), per_class=per, failing_seeds=failing[:20],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261221)
    ap.add_argument("--out", default=None)
    ap.add_argument("--progress", default=None)
    a = ap.parse_args()
    out = run(a.seconds, a.seed, verbose=True, progress_path=a.progress)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(1 if out["mismatches"] else 0)


if __name__ == "__main__":
    main()
