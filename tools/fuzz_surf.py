"""Randomised parity of the SURF finder (isx_surf_find) against its NumPy model (tests/helpers/surf_np.py): count, status, keypoints, meta
and descriptors with np.array_equal, and rows from the count on untouched.

    python tools/fuzz_surf.py --seconds 120 --seed 20261201 [--out profiles/fuzz_surf_120s.json]

The generator (no GPU needed: tests/test_surf_fuzz_generator.py checks it).  case(seed, cls) draws one of CLASSES, each sitting on a
constant of the algorithm:
    layer_edges   one side at a layer's filter size (9 + 6 l) << o, one less or one more - the layer appears or does not -, the other free
    border        blobs whose centres lie 10 .. 14 px inside a border: descriptor windows and orientation discs leave the image
    scales        blobs from sigma 1.5 (sizes near 9) to the sigma of the largest layer of the drawn octaves, on an image that holds it
    cap           a scene of many blobs; cap is 1, count - 1, count or count + 1 (the model's count)
    params        1, 3 or 4 channels, num_octaves 1 .. 4, num_layers 1 .. 4, hess_thresh from {0, 50, 300, 2000, 1e30}
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

from helpers import surf_np as M  # noqa: E402

CLASSES = ("layer_edges", "border", "scales", "cap", "params")
THRESHOLDS = (0.0, 50.0, 300.0, 2000.0, 1e30)
SENTINEL = -7777.0
MAX_SIDE = 200                # of a generated image: the model takes a fraction of a second


def layer_sizes(num_octaves, num_layers):
    return sorted({M.layer_size(o, l) for o in range(num_octaves) for l in range(num_layers + 2)})


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
    """One case: dict(cls, image, params (keywords of surf_np.Params), cap_rule, layout_seed, and what the class planted)."""
    rng = np.random.default_rng(seed)
    cls = cls or CLASSES[int(rng.integers(len(CLASSES)))]
    params, cap_rule, extra, channels = dict(hess_thresh=float(rng.choice((50.0, 300.0)))), "room", {}, 1
    if cls == "layer_edges":
        params.update(num_octaves=int(rng.integers(1, 4)), num_layers=int(rng.integers(1, 5)))
        sizes = [s for s in layer_sizes(params["num_octaves"], params["num_layers"]) if s + 1 <= MAX_SIDE]
        side = int(sizes[int(rng.integers(len(sizes)))]) + int(rng.integers(-1, 2))
        other = int(rng.integers(max(9, side // 2), MAX_SIDE + 1))
        h, w = (side, other) if rng.random() < 0.5 else (other, side)
        n = int(rng.integers(3, 12))
        centres = [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(n)]
        sigmas = [float(rng.choice((2.5, 3.5, 5.0, 7.0))) for _ in range(n)]
        extra = dict(side=side, sizes=sizes)
    elif cls == "border":
        h, w = int(rng.integers(60, 161)), int(rng.integers(60, 161))
        centres = []
        for _ in range(int(rng.integers(4, 10))):
            d, along = float(rng.integers(10, 15)), rng.random()
            centres.append([(d, along * w), (h - 1 - d, along * w), (along * h, d), (along * h, w - 1 - d)][int(rng.integers(4))])
        sigmas = [2.5] * len(centres)
        extra = dict(centres=centres)
        params["hess_thresh"] = 50.0
    elif cls == "scales":
        params.update(num_octaves=int(rng.integers(2, 4)), num_layers=4)
        top = M.layer_size(params["num_octaves"] - 1, 5)
        h, w = int(rng.integers(top + 4, MAX_SIDE + 1)), int(rng.integers(top + 4, MAX_SIDE + 1))
        big = top * 1.2 / 9.0 * 0.8                      # the sigma whose blob peaks near the last middle layer
        sigmas = [1.5, 1.8, 2.2, big, big * 0.7, big * 0.5] + [float(rng.uniform(2, big)) for _ in range(3)]
        centres = [(rng.uniform(0.25 * h, 0.75 * h), rng.uniform(0.25 * w, 0.75 * w)) for _ in sigmas]
        extra = dict(top=top, sigmas=sigmas)
        params["hess_thresh"] = 50.0
    elif cls == "cap":
        h, w = int(rng.integers(80, 141)), int(rng.integers(80, 141))
        n = int(rng.integers(10, 25))
        centres = [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(n)]
        sigmas = [float(rng.choice((2.5, 3.0, 4.0))) for _ in range(n)]
        cap_rule = ("one", "count-1", "count", "count+1")[int(rng.integers(4))]
    else:
        h, w = int(rng.integers(30, 141)), int(rng.integers(30, 141))
        n = int(rng.integers(4, 14))
        centres = [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(n)]
        sigmas = [float(rng.choice((2.5, 3.5, 5.0, 8.0))) for _ in range(n)]
        channels = int(rng.choice((1, 3, 4)))
        params = dict(hess_thresh=float(THRESHOLDS[int(rng.integers(len(THRESHOLDS)))]), num_octaves=int(rng.integers(1, 5)), num_layers=int(rng.integers(1, 5)))
    img = scene(rng, h, w, centres, sigmas, float(rng.choice((0.0, 1.0, 2.5))))
    if channels > 1:
        img = np.stack([np.clip(img.astype(np.int64) + int(rng.integers(-20, 21)), 0, 255).astype(np.uint8) for _ in range(channels)], axis=2)
    return dict(cls=cls, image=np.ascontiguousarray(img), params=params, cap_rule=cap_rule, layout_seed=int(rng.integers(1 << 30)), **extra)


def cap_of(rule, count):
    return {"room": count + 3, "one": 1, "count-1": max(count - 1, 1), "count": max(count, 1), "count+1": count + 1}[rule]


def expected(c):
    """(cap, the model's answer under that cap)"""
    full = M.find(c["image"], M.Params(**c["params"]))
    cap = cap_of(c["cap_rule"], full["count"])
    n = min(cap, full["count"])
    return cap, dict(count=n, status=full["status"] | (M.STATUS_TRUNCATED if full["count"] > cap else 0), keypoints=full["keypoints"][:n], meta=full["meta"][:n],
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
    cap, want = expected(c)
    device = bool(rng.random() < 0.6)
    image = _place_image(rng, c["image"], device, bool(rng.random() < 0.5))
    outs = [_place(rng, np.full((cap + int(rng.integers(0, 3)), cols), SENTINEL, np.float32), device, bool(rng.random() < 0.5)) for cols in (2, 5, 64)]
    k = int(rng.integers(3))
    outs[k] = _place(rng, np.full((cap, (2, 5, 64)[k]), SENTINEL, np.float32), device, bool(rng.random() < 0.5))      # the smallest row count is the cap
    cs = _place(rng, np.full((1, 2), -7777, np.int32), device, False)
    q = features.surf_default_params()
    q.hess_thresh = c["params"]["hess_thresh"]
    q.num_octaves = q.num_octaves_descr = c["params"].get("num_octaves", 3)
    q.num_layers = q.num_layers_descr = c["params"].get("num_layers", 4)
    stream = torch.cuda.current_stream()
    features.surf_find(image, q, outs[0][0], outs[1][0], outs[2][0], cs[0], 0, stream)
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
    return dict(tool="fuzz_surf", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, mismatches=len(failing), per_class=per, failing_seeds=failing[:20],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261201)
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
