#!/usr/bin/env python3
"""Fuzz isx_orb_find against its specification, tests/helpers/orb_np.py.

    python tools/fuzz_orb.py --seconds 60 [--seed N] [--out profiles/x.json]

A class fixes what the image holds - blobs under noise (corners of every strength), pure noise (more corners than any cut keeps), a periodic
grid of identical dots (ties at both cuts, with and without room), periodic squares (plateaus for the non-max suppression) and a flat image
(nothing).  The seed draws the rest: 40 to 330 pixels a side, 1, 3 or 4 channels, a grid of 1 to 3 cells a side, 0 to 600 features, 1 to 8
levels, the scale factor (2.0 takes the 2 x 2 area rule), the FAST threshold, host / device / strided mats and - one case in three - a
pattern of the caller's.  Every case is compared with the model (count, status, keypoints, meta, descriptors: bits; the rows from count on
untouched); none is skipped.  Prints one JSON line; exit status 1 on a mismatch.

    python tools/fuzz_orb.py --family limits ...

draws from the builders of the limit cases (tests/orb_cases.py) instead: 700 to 1920 features on one or two levels over noise or identical dots
(more than one pass of the final cut's 1024 candidates), strips 64 to 72 pixels high under grids of up to 1024 layers (keypoints in layers
past 256), and images of 1 to 70 pixels a side, down to cells of one pixel.  The default family is what it was, seed for seed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
from helpers import orb_np as om  # noqa: E402

CLASSES = ("blobs", "noise", "dots", "squares", "flat")
LAYOUTS = ("host", "device", "strided")
SCALES = (1.3, 1.2, 2.0, 1.5, 1.05)
SENTINEL = 91
LIMIT_KINDS = ("passes", "layers", "sides")


def make_case(seed, cls=None):
    """The case of `seed`; cls: what the image holds (default: the classes in turn)."""
    rng = np.random.default_rng(seed)
    cls = CLASSES[seed % len(CLASSES)] if cls is None else cls
    lo = 40 if rng.random() < 0.2 else 120              # one image in five may be too small for any keypoint
    h, w = int(rng.integers(lo, 331)), int(rng.integers(lo, 331))
    if seed % 7 == 0:
        w = int(rng.choice([63, 64, 65, 127, 128, 129, 255, 256, 257]))       # either side of a wave's and a block's pixels
    channels = int(rng.choice([1, 3, 4]))
    if cls == "blobs":
        img = cases.scene(h, w, seed, 1)
    elif cls == "noise":
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif cls == "dots":
        img = cases.dots(h, w, period=int(rng.choice([7, 8, 11])), count=[None, 30, 100, 300][int(rng.integers(0, 4))], lo=int(rng.integers(0, 100)),
                         hi=int(rng.integers(130, 256)))
    elif cls == "squares":
        img = cases.squares(h, w, period=int(rng.choice([12, 16, 21])), side=int(rng.integers(3, 9)))
    else:
        img = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    if channels > 1:
        img = np.ascontiguousarray(np.stack([img] + [np.clip(img.astype(np.int64) + rng.integers(-9, 10, (h, w)), 0, 255).astype(np.uint8) for _ in range(channels - 1)], 2))
    grid = (int(rng.integers(1, 4)), int(rng.integers(1, 4))) if rng.random() < 0.4 else (1, 1)
    params = om.Params(grid=(min(grid[0], w), min(grid[1], h)), n_features=int(rng.choice([0, 7, 60, 200, 600, 600])), scale_factor=float(rng.choice(SCALES)),
                       nlevels=int(rng.integers(1, om.MAX_LEVELS + 1)), fast_threshold=int(rng.choice([20, 20, 20, 5, 60, 1, 254])))
    pattern = None
    if seed % 3 == 1:
        pattern = rng.integers(-om.HALF_PATCH, om.HALF_PATCH + 1, (512, 2)).astype(np.int32)
    layout = LAYOUTS[(seed // len(CLASSES) + seed) % 3]
    return dict(seed=seed, cls=cls, image=img, params=params, pattern=pattern, layout=layout)


def make_limit_case(seed, kind=None):
    """The case of `seed` in the limits family; kind: one of LIMIT_KINDS (default: in turn)."""
    rng = np.random.default_rng(seed)
    kind = LIMIT_KINDS[seed % len(LIMIT_KINDS)] if kind is None else kind
    channels = int(rng.choice([1, 1, 3, 4]))
    if kind == "passes":
        if rng.random() < 0.5:
            side = int(rng.integers(200, 281))
            img, threshold = cases.noise(side, side, seed), int(rng.choice([1, 20]))
        else:
            img, threshold = cases.dots(400, 400, period=6, count=[None, 1100, 1300, 2100][int(rng.integers(0, 4))]), 20
        params = om.Params(grid=(1, 1), n_features=int(rng.integers(700, 1921)), scale_factor=float(rng.choice([1.2, 1.3])), nlevels=int(rng.integers(1, 3)),
                           fast_threshold=threshold)
    elif kind == "layers":
        nlevels = int(rng.choice([8, 8, 4]))
        cells = int(rng.integers(33, om.MAX_LAYERS // nlevels + 1)) if rng.random() < 0.4 else int(rng.integers(33, 48))
        h, w = int(rng.integers(64, 73)), min(cells * int(rng.integers(64, 73)) + int(rng.integers(0, cells)), om.MAX_SIDE)      # cells of two widths
        img = cases.noise(h, w, seed)
        params = om.Params(grid=(cells, 1), n_features=cells * int(rng.choice([10, 40])), scale_factor=float(rng.choice([1.05, 1.05, 1.3])), nlevels=nlevels,
                           fast_threshold=int(rng.choice([5, 20])))
    else:
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        if rng.random() < 0.25:
            h, w = [(h, 200), (200, w)][int(rng.integers(0, 2))]
        img = [cases.dots_from(h, w, period=int(rng.choice([4, 8]))), cases.noise(h, w, seed), cases.flat(h, w, int(rng.integers(0, 256)))][int(rng.integers(0, 3))]
        grid = (int(rng.integers(1, min(w, 5) + 1)), int(rng.integers(1, min(h, 3) + 1))) if rng.random() < 0.5 else (1, 1)
        params = om.Params(grid=grid, n_features=int(rng.choice([0, 10, 100, 1500])), scale_factor=float(rng.choice(SCALES)), nlevels=int(rng.integers(1, om.MAX_LEVELS + 1)),
                           fast_threshold=int(rng.choice([20, 5, 1])))
    if channels > 1:
        img = np.ascontiguousarray(np.stack([img] + [np.clip(img.astype(np.int64) + rng.integers(-9, 10, img.shape), 0, 255).astype(np.uint8) for _ in range(channels - 1)], 2))
    pattern = rng.integers(-om.HALF_PATCH, om.HALF_PATCH + 1, (512, 2)).astype(np.int32) if seed % 4 == 1 else None
    return dict(seed=seed, cls=kind, image=img, params=params, pattern=pattern, layout=LAYOUTS[(seed // len(LIMIT_KINDS) + seed) % 3])


FAMILIES = {"default": (make_case, CLASSES), "limits": (make_limit_case, LIMIT_KINDS)}


def place(a, layout, sentinel=None):
    """The array as the mat of `layout`: a NumPy array, a CUDA tensor, or a CUDA tensor view of a wider one (a longer step)."""
    a = np.ascontiguousarray(a)
    if sentinel is not None:
        a = np.full(a.shape, sentinel, a.dtype)
    if layout == "host":
        return a.copy()
    import torch
    if layout == "device":
        return torch.from_numpy(a.copy()).cuda()
    wide = torch.zeros((a.shape[0], a.shape[1] + 3) + a.shape[2:], dtype=getattr(torch, a.dtype.name), device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, :a.shape[1]]


def library_params(p):
    from imagestitch_amd import features
    q = features.default_params()
    q.grid_width, q.grid_height, q.n_features, q.scale_factor, q.nlevels, q.fast_threshold = p.grid[0], p.grid[1], p.n_features, p.scale_factor, p.nlevels, p.fast_threshold
    return q


def run_library(c, layout=None, stream=None):
    """isx_orb_find on the case's mats in `layout`: (keypoints, meta, descriptors, count_status) as NumPy arrays, whole mats"""
    import torch
    from imagestitch_amd import features
    layout = layout or c["layout"]
    q = library_params(c["params"])
    cap = max(features.capacity(q), 1)
    outs = [place(np.zeros((cap, 2), np.float32), layout, SENTINEL), place(np.zeros((cap, 4), np.float32), layout, SENTINEL),
            place(np.zeros((cap, 32), np.uint8), layout, SENTINEL), place(np.zeros((1, 2), np.int32), layout, SENTINEL)]
    pattern = None if c["pattern"] is None else place(c["pattern"], "host" if layout == "host" else "device")
    features.orb_find(place(c["image"], layout), q, *outs, pattern, 0, stream)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else o for o in outs)


def run_case(c):
    """The differences between the library and the model on one case (an empty list: none)."""
    want = om.find(c["image"], c["params"], c["pattern"])
    kp, meta, desc, cs = run_library(c)
    n = int(cs[0, 0])
    if (n, int(cs[0, 1])) != (want.count, want.status):
        return ["count_status %s, the model %s" % ((n, int(cs[0, 1])), (want.count, want.status))]
    bad = [name for name, g, w in (("keypoints", kp, want.keypoints), ("meta", meta, want.meta), ("descriptors", desc, want.descriptors))
           if not np.array_equal(g[:n].view(np.uint8), np.ascontiguousarray(w).view(np.uint8).reshape(g[:n].view(np.uint8).shape))]
    if not ((kp[n:] == SENTINEL).all() and (meta[n:] == SENTINEL).all() and (desc[n:] == SENTINEL).all()):
        bad.append("rows from count on were written")
    return bad


def run(seconds, seed, verbose=False, family="default"):
    """Draws cases of `family` (its classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    make, classes = FAMILIES[family]
    per, failing, n = {c: 0 for c in classes}, [], 0
    while time.time() - t0 < seconds:
        s = int(seed) * 1000 + n
        c = make(s)
        bad = run_case(c)
        per[c["cls"]] += 1
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=c["cls"], layout=c["layout"], differences=bad))
            if verbose:
                print("MISMATCH", s, c["cls"], c["layout"], bad, flush=True)
    return dict(tool="fuzz_orb", family=family, seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, mismatches=len(failing), per_class=per, failing_seeds=failing[:20],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=None)
    ap.add_argument("--family", choices=sorted(FAMILIES), default="default")
    a = ap.parse_args()
    out = run(a.seconds, a.seed, verbose=True, family=a.family)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(1 if out["mismatches"] else 0)


if __name__ == "__main__":
    main()
