"""Times DpSeamFinder.find (isx_dp_seam_find_cost) with both cost functions, COLOR (S:71, the default) and COLOR_GRAD, on the two
workloads of tools/time_voronoi_seam.py (the reference's tiles; the config-2 4K pair converted to CV_32FC3): device-resident images and
masks, host clock around find + synchronise, median of --iters after warm-up, the two cost functions alternating --rounds times.  Then one
profiled find per cost function (the library's event profiler, a pass of its own): the time of every seam kernel, so that the COLOR_GRAD -
COLOR difference stands next to the gradient and cost launches that explain it.  One JSON line per workload.  On a tree without the cost
function argument (--color-only is implied) it times DpSeamFinder() alone, for a comparison of COLOR with the parent commit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from time_voronoi_seam import host_clock, workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--color-only", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    have_grad = hasattr(I, "DP_COLOR_GRAD") and not a.color_only
    for name, corners, imgs, masks in workloads():
        st = torch.cuda.current_stream()
        finders = {"color": I.DpSeamFinder(I.DP_COLOR, stream=st) if hasattr(I, "DP_COLOR") else I.DpSeamFinder(stream=st)}
        if have_grad:
            finders["color_grad"] = I.DpSeamFinder(I.DP_COLOR_GRAD, stream=st)
        out = dict(workload=name, tiles=[list(m.shape) for m in masks])
        cut = {}
        for r in range(a.rounds):
            for leg, f in finders.items():
                med, best, work = host_clock(lambda w: f.find(imgs, corners, w), masks, a.warmup if r == 0 else 1, a.iters)
                out.setdefault(leg + "_ms_median", []).append(med)
                out.setdefault(leg + "_ms_min", []).append(best)
                cut[leg] = work
        if have_grad:
            out["masks_differ"] = [int((x != y).sum()) for x, y in zip(cut["color"], cut["color_grad"])]
        if not a.no_profile:
            lib = _lib.load()
            for leg, f in finders.items():
                lib.isx_profile_enable(1)
                lib.isx_profile_reset()
                f.find(imgs, corners, [m.clone() for m in masks])
                torch.cuda.synchronize()
                ent = _lib.profile_entries()
                lib.isx_profile_enable(0)
                out[leg + "_kernels_ms"] = {k: [int(v["launches"]), round(v["ms"], 4)] for k, v in ent.items() if k.startswith("seam")}
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
