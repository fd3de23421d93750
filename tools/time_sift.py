"""Times SiftFeaturesFinder's entry (isx_sift_find) on device-resident images, apart from bench.py:
  work   960 x 640, three channels: 0.6 megapixels, the work_megapix of stitching_detailed
  4k     3840 x 2160, three channels
at the class defaults (contrast_threshold 0.04, edge_threshold 10, all features), cap 4096.  Blobs under seeded noise: one 240 x 320 tile of tests/orb_cases.py
repeated over the image, fresh noise on top.  Two clocks, since the
call never synchronises on device mats: the host clock around a call + a stream synchronise (median and minimum of --iters after --warmup)
and HIP events around --events calls enqueued back to back.  With --kernels the per-launch times of the library's profiler follow.  One JSON
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

CAP = 4096


def scene(h, w, seed):
    tile = orb_cases.scene(240, 320, seed, 3)
    img = np.tile(tile, (h // 240 + 1, w // 320 + 1, 1))[:h, :w].astype(np.int16)
    img += np.random.default_rng(seed).integers(-6, 7, img.shape, dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def workloads():
    yield "work", scene(640, 960, 1)
    yield "4k", scene(2160, 3840, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    st = torch.cuda.current_stream()
    for name, img in workloads():
        q = features.sift_default_params()
        d_img = torch.from_numpy(img).cuda()
        outs = [torch.empty((CAP, 2), dtype=torch.float32, device="cuda"), torch.empty((CAP, 5), dtype=torch.float32, device="cuda"),
                torch.empty((CAP, 128), dtype=torch.float32, device="cuda"), torch.empty((1, 2), dtype=torch.int32, device="cuda")]
        ts = []
        for k in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            features.sift_find(d_img, q, *outs, 0, st)
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.events):
            features.sift_find(d_img, q, *outs, 0, st)
        e1.record()
        torch.cuda.synchronize()
        ev = e0.elapsed_time(e1) / a.events
        cs = outs[3].cpu().numpy()[0]
        rec = dict(workload=name, width=int(img.shape[1]), height=int(img.shape[0]), channels=int(img.shape[2]), keypoints=int(cs[0]), status=int(cs[1]), cap=CAP,
                   ms_median=round(float(np.median(ts)), 4), ms_min=round(float(np.min(ts)), 4), ms_events=round(ev, 4),
                   mpix_per_s=round(img.shape[0] * img.shape[1] / ev / 1e3, 1), device=torch.cuda.get_device_name(0))
        if a.kernels:
            lib = _lib.load()
            _lib.check(lib.isx_profile_enable(1))
            _lib.check(lib.isx_profile_reset())
            for _ in range(3):
                features.sift_find(d_img, q, *outs, 0, st)
            torch.cuda.synchronize()
            rec["kernels_us"] = {k: round(v["ms"] / v["launches"] * 1e3, 2) for k, v in _lib.profile_entries().items() if k.startswith("sift_")}
            _lib.check(lib.isx_profile_enable(0))
        print(json.dumps(rec), flush=True)
    features.SiftFeaturesFinder.release()


if __name__ == "__main__":
    main()
