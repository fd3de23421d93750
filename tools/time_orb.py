"""Times OrbFeaturesFinder's entry (isx_orb_find) on device-resident images, apart from bench.py:
  tile      1101 x 1101, one channel (the size of the reference's src1.bmp), the F defaults: grid 3 x 1, 1500 features, 5 levels
  hd        1920 x 1080, three channels, the F defaults
  hd-1cell  the same on one cell
Blobs under seeded noise (tests/orb_cases.py); the cost follows the pixels, and the candidates up to their capacity.  Two clocks, since the
call never synchronises on device mats: the host clock around a call + a stream synchronise (median and minimum of --iters after --warmup)
and HIP events around --events calls enqueued back to back.  With --kernels the per-kernel times of the library's profiler follow.  One JSON
line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import orb_cases  # noqa: E402
from imagestitch_amd import _lib, features  # noqa: E402


def workloads():
    yield "tile", orb_cases.scene(1101, 1101, 1), (3, 1)
    yield "hd", orb_cases.scene(1080, 1920, 2, 3), (3, 1)
    yield "hd-1cell", orb_cases.scene(1080, 1920, 2, 3), (1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=50)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    st = torch.cuda.current_stream()
    for name, img, grid in workloads():
        q = features.default_params()
        q.grid_width, q.grid_height = grid
        cap = features.capacity(q)
        d_img = torch.from_numpy(img).cuda()
        outs = [torch.empty((cap, 2), dtype=torch.float32, device="cuda"), torch.empty((cap, 4), dtype=torch.float32, device="cuda"),
                torch.empty((cap, 32), dtype=torch.uint8, device="cuda"), torch.empty((1, 2), dtype=torch.int32, device="cuda")]
        ts = []
        for k in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            features.orb_find(d_img, q, *outs, None, 0, st)
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.events):
            features.orb_find(d_img, q, *outs, None, 0, st)
        e1.record()
        torch.cuda.synchronize()
        ev = e0.elapsed_time(e1) / a.events
        cs = outs[3].cpu().numpy()[0]
        rec = dict(workload=name, width=int(img.shape[1]), height=int(img.shape[0]), channels=1 if img.ndim == 2 else int(img.shape[2]), grid=list(grid),
                   keypoints=int(cs[0]), status=int(cs[1]), capacity=cap, ms_median=round(float(np.median(ts)), 4), ms_min=round(float(np.min(ts)), 4),
                   ms_events=round(ev, 4), mpix_per_s=round(img.shape[0] * img.shape[1] / ev / 1e3, 1), device=torch.cuda.get_device_name(0))
        if a.kernels:
            lib = _lib.load()
            _lib.check(lib.isx_profile_enable(1))
            _lib.check(lib.isx_profile_reset())
            for _ in range(5):
                features.orb_find(d_img, q, *outs, None, 0, st)
            torch.cuda.synchronize()
            rec["kernels_us"] = {k: round(v["ms"] / v["launches"] * 1e3, 2) for k, v in _lib.profile_entries().items() if k.startswith("orb_")}
            _lib.check(lib.isx_profile_enable(0))
        print(json.dumps(rec), flush=True)
    features.OrbFeaturesFinder.release()


if __name__ == "__main__":
    main()
