#!/usr/bin/env python3
"""Fuzz isx_estimate_cameras against its specification, tests/helpers/estimator_np.py.

    python tools/fuzz_estimator.py --seconds 60 [--seed N] [--out profiles/x.json]

A class fixes the size of a call's first rig on the kernel's constants - 2 and 3 images (the smallest), 8 and 9, 16 and 17 (81 and 289
ordered pairs: either side of a wave and of the 256-thread block), 63 and 64 (both LDS sorts at full size).  The seed draws the rest: one
to five rigs a call, the edge density from a bare tree to the complete graph, the share of tied weights, the share of pairs without H,
host / device / strided mats, estimated or given focals, and - one case in five - homographies that are exactly singular.  Every case is
compared with the model (cameras, kr32, tree, rig_stats: bits, NaNs by position); none is skipped.  Prints one JSON line; exit status 1 on a
mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import estimator_cases as cases  # noqa: E402
from helpers import estimator_np as em  # noqa: E402

CLASSES = (2, 3, 8, 9, 16, 17, 63, 64)          # images of the first rig
LAYOUTS = ("host", "device", "strided")
_SMALL = (2, 3, 4, 5, 8, 9)                     # images of the other rigs


def _rig(rng, n, density, tie_share, no_h_share, singular):
    order = rng.permutation(n)
    tree = {tuple(sorted((int(order[k]), int(order[rng.integers(0, k)])))) for k in range(1, n)}      # a random spanning tree
    pairs = [p for p in cases.all_pairs(n) if p in tree or rng.random() < density]
    c = cases.make(n, pairs, int(rng.integers(1 << 30)), focal=float(rng.uniform(300, 3000)), generic=bool(rng.random() < 0.3))
    w = c["stats"][:, 1]
    tied = rng.random(len(pairs)) < tie_share
    w[tied] = rng.choice([30, 60], int(tied.sum()))
    for k in np.where(rng.random(len(pairs)) < no_h_share)[0]:
        c["stats"][k, 0], c["stats"][k, 1], c["H"][k] = 0, 0, 0.0
    c["stats"][:, 0] |= (rng.integers(0, 2, len(pairs)) * 2).astype(np.int32) * (c["stats"][:, 0] & 1)      # other status bits do not matter
    if singular:
        for k in np.where((rng.random(len(pairs)) < 0.3) & (c["stats"][:, 0] & 1 == 1))[0]:
            a, b = rng.integers(-3, 4, 3).astype(np.float64), rng.integers(-3, 4, 3).astype(np.float64)
            c["H"][k] = np.array([a, 2.0 * a, b]) if rng.random() < 0.7 else np.zeros((3, 3))              # two proportional rows: det exactly 0
    return c


def make_case(seed, cls=None):
    """The case of `seed`; cls: the images of the first rig (default: the classes in turn)."""
    rng = np.random.default_rng(seed)
    n0 = CLASSES[seed % len(CLASSES)] if cls is None else cls
    nrigs = 1 + seed % 5
    layout = LAYOUTS[(seed // len(CLASSES) + seed) % 3]
    singular = seed % 5 == 3
    density, tie_share, no_h_share = rng.choice([0.0, 0.3, 1.0]), rng.choice([0.0, 0.5, 1.0]), rng.choice([0.0, 0.0, 0.2, 0.6])
    ns = [n0] + [int(rng.choice(_SMALL)) for _ in range(nrigs - 1)]
    rigs = [_rig(rng, n, density, tie_share, no_h_share, singular) for n in ns]
    given = bool(rng.random() < 0.3)
    for r in rigs:
        m = len(r["sizes"])
        r["focals_in"] = np.stack([rng.uniform(300, 3000, m), rng.uniform(0.9, 1.1, m), rng.uniform(100, 900, m), rng.uniform(100, 900, m)], 1) if given else None
    c = cases.join(rigs)
    if nrigs == 1 and seed % 2:
        c["rig_first"] = None
    c.update(layout=layout, singular=int(singular), cls=n0, seed=seed)
    return c


def same(got, want):
    """Bits, NaNs by position (their payloads are the hardware's)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ng, nw = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(ng, nw) and np.array_equal(got.view(u)[~ng], want.view(u)[~nw]))


def place(a, layout, sentinel=None):
    """The array as the mat of `layout`: a NumPy array, a CUDA tensor, or a CUDA tensor view with two more columns a row (a wider step).
    sentinel: fill an output with it instead."""
    a = np.ascontiguousarray(a)
    if sentinel is not None:
        a = np.full(a.shape, sentinel, a.dtype)
    if layout == "host":
        return a.copy()
    import torch
    if layout == "device" or a.shape[0] == 0:
        return torch.from_numpy(a.copy()).cuda()
    wide = torch.zeros((a.shape[0], a.shape[1] + 2), dtype=getattr(torch, a.dtype.name), device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, :a.shape[1]]


def run_library(c, layout=None, stream=None):
    """isx_estimate_cameras on the case's mats in `layout`.  Returns ((cameras, kr32, tree, rig_stats) as NumPy arrays, info)."""
    import torch
    from imagestitch_amd import cameras as cam
    layout = layout or c.get("layout", "device")
    n, npairs = len(c["sizes"]), len(c["pairs"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    H = place(np.asarray(c["H"], np.float64).reshape(3 * npairs, 3), layout)
    stats = place(c["stats"], layout)
    conf = place(np.zeros((1, max(npairs, 1))), "host" if layout == "host" else "device")
    fin = None if c["focals_in"] is None else place(c["focals_in"], layout)
    outs = [place(np.zeros((n, 16)), layout, -7777.25), place(np.zeros((n, 18), np.float32), layout, -7777.25),
            place(np.zeros((n, 2), np.int32), layout, -7777), place(np.zeros((nrigs, 8), np.int32), layout, -7777)]
    info = cam.estimate_cameras(c["sizes"], c["pairs"], H, stats, conf, *outs, rig_first=c["rig_first"], focals_in=fin, stream=stream)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else o for o in outs), info


def run_case(c):
    """The differences between the library and the model on one case (an empty list: none)."""
    want = em.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"], c["focals_in"])
    got, info = run_library(c)
    bad = [name for name, g, w in zip(("cameras", "kr32", "tree", "rig_stats"), got, want) if not same(g, w)]
    if info[1] != 1:
        bad.append("launches %d" % info[1])
    return bad


def run(seconds, seed, verbose=False):
    """Draws cases (the classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    per, failing, n, rigs = {c: 0 for c in CLASSES}, [], 0, 0
    while time.time() - t0 < seconds:
        s = int(seed) * 1000 + n
        c = make_case(s)
        bad = run_case(c)
        per[c["cls"]] += 1
        rigs += 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=c["cls"], layout=c["layout"], differences=bad))
            if verbose:
                print("MISMATCH", s, c["cls"], c["layout"], bad, flush=True)
    return dict(tool="fuzz_estimator", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, rigs=rigs, mismatches=len(failing), per_class=per,
                failing_seeds=failing[:20], device=torch.cuda.get_device_name(0))


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
