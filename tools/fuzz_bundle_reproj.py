#!/usr/bin/env python3
"""Fuzz isx_bundle_adjust_reproj against its specification, tests/helpers/bundle_reproj_np.py.

    python tools/fuzz_bundle_reproj.py --seconds 60 [--seed N] [--out profiles/x.json]

The cases are tools/fuzz_bundle.py's (its classes of 2, 3, 5 and 9 images in the first rig, one to three rigs a call, its edge densities,
inliers around the tile of the accumulation, confidences either side of conf_thresh, max_iter, layouts and planted faults: a NaN focal, a
singular R, a count above its mat's rows, an index outside the keypoints, the estimator's assert bit) with what BundleAdjusterReproj adds drawn
on top: every camera comes in with ppx and ppy moved by up to 12 pixels and its aspect scaled by up to 2 %, and refine_flags is random -
everything, nothing, the focal alone or any of the 32 values.  Every fourth case is fuzz_bundle.make_wide_case's, a rig that goes round, with
the same drawn on top (counted as `wide`).  Every case is compared with the model (cameras, kr32, rig_stats, rig_err:
bits, NaNs by position); none is skipped.  The model in Python sets the pace.  Prints one JSON line; exit status 1 on a mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_bundle as fz  # noqa: E402
from fuzz_estimator import place, same  # noqa: E402
from helpers import bundle_reproj_np as rp  # noqa: E402

CLASSES, LAYOUTS, NAMES = fz.CLASSES, fz.LAYOUTS, fz.NAMES


def _plant(c, seed):
    """The ppx / ppy / aspect offsets and the refine_flags of `seed` on a case of fuzz_bundle (in place)."""
    rng = np.random.default_rng([seed, 7])
    cams = c["cameras_in"]
    n = cams.shape[0]
    scale = float(rng.choice([0.0, 0.25, 1.0]))
    cams[:, 1] = 1.0 + scale * rng.uniform(-0.02, 0.02, n)
    cams[:, 2] += scale * rng.uniform(-12, 12, n)
    cams[:, 3] += scale * rng.uniform(-12, 12, n)
    c["refine_flags"] = int(rng.choice([31, 0, 1, int(rng.integers(32))], p=[0.4, 0.1, 0.1, 0.4]))
    if c["max_iter"] == 1000:
        c["max_iter"] = 40                                   # the natural end of seven parameters a camera is slower in the model
    return c


def make_case(seed, cls=None):
    """fuzz_bundle.make_case(seed) with planted ppx / ppy / aspect offsets on cameras_in and a refine_flags."""
    return _plant(fz.make_case(seed, cls), seed)


def make_wide_case(seed):
    """fuzz_bundle.make_wide_case(seed), a rig that goes round, with the same offsets and refine_flags drawn on top."""
    return _plant(fz.make_wide_case(seed), seed)


def run_model(c):
    return rp.adjust(c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"], c["conf"], c["est_rig_stats"], c["cameras_in"],
                     c["rig_first"], c["conf_thresh"], c["max_iter"], refine_flags=c.get("refine_flags", rp.REFINE_ALL))


def run_library(c, layout=None, stream=None):
    """isx_bundle_adjust_reproj on the case's mats in `layout`.  Returns ((cameras, kr32, rig_stats, rig_err) as NumPy arrays, info)."""
    import torch
    from imagestitch_amd import adjuster as adj
    layout = layout or c.get("layout", "device")
    n = len(c["sizes"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    row = "host" if layout == "host" else "device"            # a 1 x n mat has no step to widen
    kps = [place(k, layout) for k in c["keypoints"]]
    ms = [place(m, layout) for m in c["matches"]]
    mk = [place(m, layout) for m in c["masks"]]
    counts, conf = place(c["counts"], row), place(c["conf"], row)
    stats, est, cin = place(c["stats"], layout), place(c["est_rig_stats"], layout), place(c["cameras_in"], layout)
    outs = [place(np.zeros((n, 16)), layout, -7777.25), place(np.zeros((n, 18), np.float32), layout, -7777.25),
            place(np.zeros((nrigs, 8), np.int32), layout, -7777), place(np.zeros((nrigs, 2)), layout, -7777.25)]
    info = adj.bundle_adjust_reproj(c["sizes"], kps, c["pairs"], ms, mk, counts, stats, conf, est, cin, *outs, rig_first=c["rig_first"],
                                    conf_thresh=c["conf_thresh"], max_iter=c["max_iter"], refine_flags=c.get("refine_flags", rp.REFINE_ALL),
                                    stream=stream)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else o for o in outs), info


def run_case(c):
    """The differences between the library and the model on one case (an empty list: none)."""
    want = run_model(c)
    got, info = run_library(c)
    bad = [name for name, g, w in zip(NAMES, got, want) if not same(g, w)]
    if info[1] != 1:
        bad.append("launches %d" % info[1])
    return bad


def run(seconds, seed, verbose=False):
    """Draws cases (the classes in turn; every fourth a rig that goes round, counted as `wide`) for `seconds` and compares the library with
    the model.  Returns a summary dict."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    per, failing, n, rigs, faults, flags = {c: 0 for c in CLASSES}, [], 0, 0, 0, {}
    wide = {c: 0 for c in fz.WIDE_CLASSES}
    while time.time() - t0 < seconds:
        is_wide = n % fz.WIDE_EVERY == fz.WIDE_EVERY - 1
        s = int(seed) * 1000 + (sum(wide.values()) if is_wide else sum(per.values()))      # make_case's seeds run on as without the wide share
        c = make_wide_case(s) if is_wide else make_case(s)
        bad = run_case(c)
        (wide if is_wide else per)[c["cls"]] += 1
        rigs += 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
        faults += 1 if c["fault"] else 0
        flags[c["refine_flags"]] = flags.get(c["refine_flags"], 0) + 1
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=c["cls"], layout=c["layout"], refine_flags=c["refine_flags"], differences=bad))
            if verbose:
                print("MISMATCH", s, c["cls"], c["layout"], c["refine_flags"], bad, flush=True)
    return dict(tool="fuzz_bundle_reproj", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, rigs=rigs, planted_faults=faults,
                mismatches=len(failing), wide=sum(wide.values()), per_class=per,
                per_wide_class=wide, refine_flags_seen=len(flags), failing_seeds=failing[:20], device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261203)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = run(a.seconds, a.seed, verbose=True)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(1 if out["mismatches"] else 0)


if __name__ == "__main__":
    main()
