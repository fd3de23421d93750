"""Times isx_estimate_cameras, apart from bench.py.  No time is an acceptance criterion: the stage is small and latency-bound.

  launch to launch   one rig of 2, 8 and 64 images (complete graphs) and 64 rigs of 8 in one call, on device mats: HIP events around
                     --chain calls enqueued back to back, divided by their number; --repeats such windows after --warmup calls.
  to host cameras    8 images x --rows rows through the matcher once; then, timed on the host clock and ending with the cameras in host
                     memory: isx_find_homography on the matcher's device mats followed by (a) isx_estimate_cameras on the device mats and
                     one read-back of cameras and kr32, or (b) a read-back of H, stats and conf and the model's host arithmetic
                     (tests/helpers/estimator_np.py - Python scalars: the comparison the project has today, not a tuned host port).
                     The homography launch alone (with a synchronise) is timed too, for what both paths share.

Every figure is a median with the minimum and maximum of its repeats.  Writes --out (profiles/estimator_time.json) and prints it."""
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
import torch  # noqa: E402

import estimator_cases as cases  # noqa: E402
import time_homography as th  # noqa: E402
from helpers import estimator_np as em  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from imagestitch_amd import cameras as cam  # noqa: E402
from imagestitch_amd import homography, matcher  # noqa: E402


def spread(ts):
    return dict(median=round(float(np.median(ts)), 4), min=round(float(min(ts)), 4), max=round(float(max(ts)), 4), repeats=len(ts))


def launch_to_launch(c, a):
    """Milliseconds a call, between HIP events around a.chain chained calls on device mats."""
    n, npairs = len(c["sizes"]), len(c["pairs"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    dev = dict(device="cuda")
    H = torch.from_numpy(np.ascontiguousarray(c["H"]).reshape(3 * npairs, 3)).cuda()
    stats, conf = torch.from_numpy(c["stats"]).cuda(), torch.zeros((1, npairs), dtype=torch.float64, **dev)
    outs = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
            torch.empty((n, 2), dtype=torch.int32, **dev), torch.empty((nrigs, 8), dtype=torch.int32, **dev))
    st = torch.cuda.current_stream()

    def call():
        return cam.estimate_cameras(c["sizes"], c["pairs"], H, stats, conf, *outs, rig_first=c["rig_first"], stream=st)
    for _ in range(a.warmup):
        info = call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.chain):
            call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / a.chain)
    # the kernel alone: the library's own profiler (start / stop events on the launch), in calls of their own
    lib = _lib.load()
    _lib.check(lib.isx_profile_reset())
    _lib.check(lib.isx_profile_enable(1))
    for _ in range(a.repeats * 5):
        call()
    torch.cuda.synchronize()
    prof = _lib.profile_entries().get("estimator_rigs", {})
    _lib.check(lib.isx_profile_enable(0))
    kernel_us = round(1e3 * prof["ms"] / prof["launches"], 2) if prof.get("launches") else None
    return dict(images=n, rigs=nrigs, pairs=npairs, launches=info[1], ms_per_call=spread(ts), kernel_us_mean=kernel_us)


def host_clock(fn, a):
    ts = []
    for k in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts[a.warmup:])


def to_host_cameras(a):
    n = 8
    descs, kps, sizes = th.features(n, n, a.rows, a.shared)
    pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
    k = len(pairs)
    dev = dict(device="cuda")
    ms = [torch.empty((2 * a.rows, 3), dtype=torch.int32, **dev) for _ in pairs]
    ps = [torch.empty((2 * a.rows, 4), dtype=torch.float32, **dev) for _ in pairs]
    masks = [torch.empty((2 * a.rows, 1), dtype=torch.uint8, **dev) for _ in pairs]
    cnt = torch.empty((1, k), dtype=torch.int32, **dev)
    H, stats, conf = torch.empty((3 * k, 3), dtype=torch.float64, **dev), torch.empty((k, 8), dtype=torch.int32, **dev), torch.empty((1, k), dtype=torch.float64, **dev)
    outs = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
            torch.empty((n, 2), dtype=torch.int32, **dev), torch.empty((1, 8), dtype=torch.int32, **dev))
    st = torch.cuda.current_stream()
    matcher.match_features(descs, pairs, 0.3, ms, cnt, kps, sizes, ps, stream=st)
    torch.cuda.synchronize()

    def homog():
        homography.find_homography(ps, cnt, H, masks, stats, conf, stream=st)

    def homog_only():
        homog()
        torch.cuda.synchronize()

    def through_the_entry():
        homog()
        cam.estimate_cameras(sizes, pairs, H, stats, conf, *outs, stream=st)
        return outs[0].cpu().numpy(), outs[1].cpu().numpy()          # .cpu() waits for the stream

    def through_the_host_model():
        homog()
        Hh, sh, _ = H.cpu().numpy(), stats.cpu().numpy(), conf.cpu().numpy()
        return em.estimate(sizes, pairs, Hh, sh)[:2]
    got, want = through_the_entry(), through_the_host_model()
    same = bool(np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))
    return dict(images=n, rows=a.rows, pairs=k, pairs_with_H=int((stats.cpu().numpy()[:, 0] & 1).sum()), same_bits_both_paths=same,
                homography_alone_ms=host_clock(homog_only, a), entry_ms=host_clock(through_the_entry, a),
                host_model_ms=host_clock(through_the_host_model, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--shared", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--chain", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimator_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_estimator needs a GPU"
    shapes = {"rig_of_2": cases.make(2, [(0, 1)], 1), "rig_of_8": cases.make(8, cases.all_pairs(8), 2), "rig_of_64": cases.make(64, cases.all_pairs(64), 3),
              "64_rigs_of_8": cases.join([cases.make(8, cases.all_pairs(8), 100 + r) for r in range(64)])}
    out = dict(tool="time_estimator", device=torch.cuda.get_device_name(0), chain=a.chain, warmup=a.warmup,
               launch_to_launch={k: launch_to_launch(c, a) for k, c in shapes.items()}, to_host_cameras=to_host_cameras(a))
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
