"""Times isx_bundle_adjust_ray, apart from bench.py.  No time is an acceptance criterion: the stage is latency-bound - one workgroup a rig runs
the whole Levenberg-Marquardt loop - and the iterations a rig takes set its time, so they are recorded beside it.

  launch to launch   one rig of 2, 8 and 64 images (complete graphs, --inliers inlier matches an edge, cameras started 1 degree and 5 % off)
                     and 64 rigs of 8 in one call, on device mats, run to their natural end (max_iter 1000): HIP events around --chain calls
                     enqueued back to back, divided by their number; --repeats such windows after --warmup calls.
  kernel             the library's own profiler (start / stop events on the launch), in calls of their own.

Every figure is a median with the minimum and maximum of its repeats.  Writes --out (profiles/bundle_time.json) and prints it.

  --adjuster reproj  times isx_bundle_adjust_reproj on the same four shapes (their cameras also start with ppx, ppy moved and the aspect
                     scaled, tests/bundle_reproj_cases.py) and, as the yardstick, isx_bundle_adjust_ray on them in the same run; --out
                     defaults to profiles/bundle_reproj_time.json.
  --wave             adds isx_wave_correct on the rotations of the same four shapes, timed the same way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bundle_cases as cases  # noqa: E402
import bundle_reproj_cases as rcases  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from imagestitch_amd import adjuster as adj  # noqa: E402
from time_estimator import spread  # noqa: E402


def _timed(call, a, kernel):
    """(info of a call, milliseconds a call in a.repeats windows of a.chain chained calls, the kernel's mean milliseconds)"""
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
    lib = _lib.load()
    _lib.check(lib.isx_profile_reset())
    _lib.check(lib.isx_profile_enable(1))
    for _ in range(a.repeats):
        call()
    torch.cuda.synchronize()
    prof = _lib.profile_entries().get(kernel, {})
    _lib.check(lib.isx_profile_enable(0))
    return info, ts, round(prof["ms"] / prof["launches"], 4) if prof.get("launches") else None


def wave(c, a):
    """isx_wave_correct on the case's cameras_in, device mats."""
    n = len(c["sizes"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    dev = dict(device="cuda")
    cin = torch.from_numpy(np.ascontiguousarray(c["cameras_in"])).cuda()
    outs = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev), torch.empty((nrigs, 2), dtype=torch.int32, **dev))
    st = torch.cuda.current_stream()
    info, ts, kernel_ms = _timed(lambda: adj.wave_correct(cin, *outs, rig_first=c["rig_first"], kind=adj.WAVE_CORRECT_HORIZ, stream=st), a, "wave_rigs")
    return dict(images=n, rigs=nrigs, launches=info[1], ms_per_call=spread(ts), kernel_ms_mean=kernel_ms,
                status_bits=int(np.bitwise_or.reduce(outs[2].cpu().numpy()[:, 0])))


def launch_to_launch(c, a, adjuster="ray"):
    """Milliseconds a call, between HIP events around a.chain chained calls on device mats."""
    n, npairs = len(c["sizes"]), len(c["pairs"])
    nrigs = 1 if c["rig_first"] is None else len(c["rig_first"]) - 1
    dev = dict(device="cuda")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    kps, ms, mk = [up(k) for k in c["keypoints"]], [up(m) for m in c["matches"]], [up(m) for m in c["masks"]]
    counts, stats, conf, est, cin = up(c["counts"]), up(c["stats"]), up(c["conf"]), up(c["est_rig_stats"]), up(c["cameras_in"])
    outs = (torch.empty((n, 16), dtype=torch.float64, **dev), torch.empty((n, 18), dtype=torch.float32, **dev),
            torch.empty((nrigs, 8), dtype=torch.int32, **dev), torch.empty((nrigs, 2), dtype=torch.float64, **dev))
    st = torch.cuda.current_stream()

    fn = adj.bundle_adjust_ray if adjuster == "ray" else adj.bundle_adjust_reproj

    def call():
        return fn(c["sizes"], kps, c["pairs"], ms, mk, counts, stats, conf, est, cin, *outs, rig_first=c["rig_first"],
                  conf_thresh=c["conf_thresh"], max_iter=c["max_iter"], stream=st)
    info, ts, kernel_ms = _timed(call, a, "bundle_rigs" if adjuster == "ray" else "bundle_reproj_rigs")
    rs, re = outs[2].cpu().numpy(), outs[3].cpu().numpy()
    return dict(images=n, rigs=nrigs, pairs=npairs, inlier_matches=int(rs[:, adj.RIG_MATCHES].sum()), launches=info[1], ms_per_call=spread(ts),
                kernel_ms_mean=kernel_ms, iterations=dict(min=int(rs[:, adj.RIG_ITERS].min()), max=int(rs[:, adj.RIG_ITERS].max())),
                error_evaluations=dict(min=int(rs[:, adj.RIG_ERR_EVALS].min()), max=int(rs[:, adj.RIG_ERR_EVALS].max())),
                status_bits=int(np.bitwise_or.reduce(rs[:, adj.RIG_STATUS])), first_err_max=float(re[:, 0].max()), last_err_max=float(re[:, 1].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inliers", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chain", type=int, default=4)
    ap.add_argument("--adjuster", choices=("ray", "reproj"), default="ray")
    ap.add_argument("--wave", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bundle_time.json" if a.adjuster == "ray" else "bundle_reproj_time.json")
    assert torch.cuda.is_available(), "time_bundle needs a GPU"
    make = cases.make if a.adjuster == "ray" else rcases.make
    mk = lambda n, seed: make(n, cases.all_pairs(n), seed, inliers=a.inliers, max_iter=1000, r_scale=1.0)      # noqa: E731
    shapes = {"rig_of_2": mk(2, 1), "rig_of_8": mk(8, 2), "rig_of_64": mk(64, 3), "64_rigs_of_8": cases.join([mk(8, 100 + r) for r in range(64)])}
    out = dict(tool="time_bundle", device=torch.cuda.get_device_name(0), chain=a.chain, warmup=a.warmup, inliers_per_edge=a.inliers,
               launch_to_launch={k: launch_to_launch(c, a) for k, c in shapes.items()})
    if a.adjuster == "reproj":
        out["adjuster"] = "reproj"
        out["launch_to_launch_reproj"] = {k: launch_to_launch(c, a, "reproj") for k, c in shapes.items()}
    if a.wave:
        out["wave_correct"] = {k: wave(c, a) for k, c in shapes.items()}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
