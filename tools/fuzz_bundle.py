#!/usr/bin/env python3
"""Fuzz isx_bundle_adjust_ray against its specification, tests/helpers/bundle_np.py.

    python tools/fuzz_bundle.py --seconds 60 [--seed N] [--out profiles/x.json]

A class fixes the size of a call's first rig - 2, 3, 5 and 9 images - and the seed draws the rest: one to three rigs a call, the edge density
from a chain to the complete graph, inliers per edge around the tile of the accumulation (1 .. 2 * TILE + 2), the share of mask-0 matches,
confidences either side of conf_thresh (some exactly on it), max_iter 1 .. 6 (one case in eight runs to its natural end), how far off the
cameras start, host / device / strided mats, and - one case in six - a fault: a NaN focal, a singular R, a count above its mat's rows, an
index outside the keypoints, the estimator's assert bit.  Every fourth case is instead a rig that goes round (make_wide_case: a ring or an arc
with rotation vectors up to half a turn, no fault; counted as `wide`).  Every case is compared with the model (cameras, kr32, rig_stats, rig_err: bits,
NaNs by position); none is skipped.  The model in Python sets the pace.  Prints one JSON line; exit status 1 on a mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundle_cases as cases  # noqa: E402
from fuzz_estimator import place, same  # noqa: E402
from helpers import bundle_np as bm  # noqa: E402

CLASSES = (2, 3, 5, 9)                          # images of the first rig
LAYOUTS = ("host", "device", "strided")
NAMES = ("cameras", "kr32", "rig_stats", "rig_err")
_SMALL = (2, 3, 4)                              # images of the other rigs


def _rig(rng, n, density, max_iter, fault, rotations=None, pairs=None):
    """rotations, pairs: planted rotations and the pairs that share a view (make_wide_case); None: a narrow rig, pairs drawn by density."""
    if pairs is None:
        pairs = [p for p in cases.all_pairs(n) if p[1] == p[0] + 1 or rng.random() < density]
    inl = [int(rng.choice([1, 3, 9, cases.TILE - 1, cases.TILE, cases.TILE + 1, 2 * cases.TILE + 2], p=[0.1, 0.2, 0.4, 0.075, 0.075, 0.075, 0.075]))
           for _ in pairs]
    conf = [float(rng.choice([2.0, 1.5, 1.0, 0.5, 0.0], p=[0.5, 0.25, 0.1, 0.1, 0.05])) for _ in pairs]
    planted = {} if rotations is None else dict(rotations=rotations)      # a narrow rig is made by the call it always was
    c = cases.make(n, pairs, int(rng.integers(1 << 30)), inliers=inl, outliers=float(rng.choice([0.0, 0.3])), focal=float(rng.uniform(400, 2500)),
                   off_deg=float(rng.choice([0.0, 0.5, 3.0])), off_focal=float(rng.choice([0.0, 0.02, 0.1])), conf=conf, center=int(rng.integers(n)),
                   max_iter=max_iter, **planted)
    if fault == 1:
        c["cameras_in"][int(rng.integers(n)), 0] = np.nan
    elif fault == 2:
        c["cameras_in"][int(rng.integers(n)), 4:13] = 0.0
    elif fault == 3:
        c["counts"][0, int(rng.integers(len(pairs)))] += 7
    elif fault == 4:
        k = int(rng.integers(len(pairs)))
        c["matches"][k][0, int(rng.integers(2))] = int(rng.choice([-1, 1 << 20]))
    elif fault == 5:
        c["est_rig_stats"][0, 0] |= cases.EST_ASSERT
    return c


def make_case(seed, cls=None):
    """The case of `seed`; cls: the images of the first rig (default: the classes in turn)."""
    rng = np.random.default_rng(seed)
    n0 = CLASSES[seed % len(CLASSES)] if cls is None else cls
    nrigs = 1 + seed % 3
    layout = LAYOUTS[(seed // len(CLASSES) + seed) % 3]
    max_iter = 1000 if seed % 8 == 5 and n0 <= 3 else int(rng.integers(1, 7))
    fault = int(rng.integers(1, 6)) if seed % 6 == 2 else 0
    density = float(rng.choice([0.0, 0.4, 1.0]))
    ns = [n0] + [int(rng.choice(_SMALL)) for _ in range(nrigs - 1)]
    rigs = [_rig(rng, n, density, max_iter, fault if r == 0 else 0) for r, n in enumerate(ns)]
    c = cases.join(rigs)
    if nrigs == 1 and seed % 2:
        c["rig_first"] = None
    c.update(layout=layout, fault=fault, cls=n0, seed=seed)
    return c


WIDE_CLASSES = ("ring", "arc")
WIDE_EVERY = 4                                  # run() draws every fourth case from make_wide_case


def make_wide_case(seed):
    """A rig that goes round (bundle_cases.ring): a closed ring of 6 to 9 cameras, or an arc of 3 to 9 with a step of 20 to 60 degrees, a
    random centre, a jitter of 0, 0.01 or 0.03 rad, pairs one step apart or one and two (those whose axes are less than 80 degrees apart),
    make_case's draws of inliers, confidences, start offsets, layout and max_iter, no fault; every other case has a narrow second rig.  Such
    rigs take the branches of bundle_math.hpp that make_case's never reach (tests/test_bundle_model.py)."""
    rng = np.random.default_rng([seed, 11])
    cls = WIDE_CLASSES[int(rng.integers(2))]
    if cls == "ring":
        n = int(rng.integers(6, 10))
        step = 360.0 / n
    else:
        step = float(rng.uniform(20.0, 60.0))
        n = int(rng.integers(3, min(9, int(300.0 / step)) + 1))
    rotations = cases.ring(n, step, jitter=float(rng.choice([0.0, 0.01, 0.03])), seed=int(rng.integers(1 << 30)))
    steps = (1, 2) if rng.random() < 0.5 else (1,)
    layout = LAYOUTS[int(rng.integers(3))]
    max_iter = 1000 if n <= 3 and rng.random() < 0.25 else int(rng.integers(1, 7))
    rigs = [_rig(rng, n, 0.0, max_iter, 0, rotations, cases.ring_pairs(rotations, steps))]
    if rng.random() < 0.5:
        rigs.append(_rig(rng, int(rng.choice(_SMALL)), float(rng.choice([0.0, 1.0])), max_iter, 0))
    c = cases.join(rigs)
    if len(rigs) == 1 and rng.random() < 0.5:
        c["rig_first"] = None
    c.update(layout=layout, fault=0, cls=cls, seed=seed, wide=True, step_deg=step, steps=steps, rotations=rotations)
    return c


def run_model(c):
    return bm.adjust(c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"], c["conf"], c["est_rig_stats"], c["cameras_in"],
                     c["rig_first"], c["conf_thresh"], c["max_iter"])


def run_library(c, layout=None, stream=None):
    """isx_bundle_adjust_ray on the case's mats in `layout`.  Returns ((cameras, kr32, rig_stats, rig_err) as NumPy arrays, info)."""
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
    info = adj.bundle_adjust_ray(c["sizes"], kps, c["pairs"], ms, mk, counts, stats, conf, est, cin, *outs, rig_first=c["rig_first"],
                                 conf_thresh=c["conf_thresh"], max_iter=c["max_iter"], stream=stream)
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
    per, failing, n, rigs, faults = {c: 0 for c in CLASSES}, [], 0, 0, 0
    wide = {c: 0 for c in WIDE_CLASSES}
    while time.time() - t0 < seconds:
        is_wide = n % WIDE_EVERY == WIDE_EVERY - 1
        s = int(seed) * 1000 + (sum(wide.values()) if is_wide else sum(per.values()))      # make_case's seeds run on as without the wide share
        c = make_wide_case(s) if is_wide else make_case(s)
        bad = run_case(c)
        (wide if is_wide else per)[c["cls"]] += 1
        rigs += 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
        faults += 1 if c["fault"] else 0
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=c["cls"], layout=c["layout"], differences=bad))
            if verbose:
                print("MISMATCH", s, c["cls"], c["layout"], bad, flush=True)
    return dict(tool="fuzz_bundle", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, rigs=rigs, planted_faults=faults, mismatches=len(failing),
                wide=sum(wide.values()), per_class=per, per_wide_class=wide, failing_seeds=failing[:20], device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261020)
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
