"""Times the float features matcher's entry (isx_match_features_f32) on device-resident descriptors, apart from bench.py:
  pair2k   2 images x 2 000 rows (1 pair)
  ring8    8 images x 2 000 rows (28 pairs)
each at cols = 64 and 128.  Descriptors with planted matches (tools/fuzz_match_f32.py's builder on the first pairs; the search's cost does
not depend on the content).  Two clocks, since the call never synchronises on device mats: the host clock around a call + a stream
synchronise (median and minimum of --iters after --warmup) and HIP events around --events calls enqueued back to back.  A candidate
(query, train) pair costs 3 W VALU operations - W subtractions, multiplications and additions, W the padded width -, which gives the
operations per second of the event time.  One JSON line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fuzz_match_f32  # noqa: E402
from imagestitch_amd import matcher  # noqa: E402


def workloads(rows, widths):
    for cols in widths:
        for name, n in (("pair2k", 2), ("ring8", 8)):
            rng = np.random.default_rng(n)
            pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
            descs, _ = fuzz_match_f32.build(rng, [rows] * n, pairs, cols, "cloud")
            yield name, cols, [torch.from_numpy(d).cuda() for d in descs], pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--cols", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=100)
    a = ap.parse_args()
    st = torch.cuda.current_stream()
    for name, cols, descs, pairs in workloads(a.rows, a.cols):
        ms = [torch.empty((2 * a.rows, 3), dtype=torch.int32, device="cuda") for _ in pairs]
        cnt = torch.empty((1, len(pairs)), dtype=torch.int32, device="cuda")
        info = None
        ts = []
        for k in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = matcher.match_features_f32(descs, pairs, 0.3, ms, cnt, stream=st)
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.events):
            matcher.match_features_f32(descs, pairs, 0.3, ms, cnt, stream=st)
        e1.record()
        torch.cuda.synchronize()
        ev = e0.elapsed_time(e1) / a.events
        comparisons = 2.0 * a.rows * a.rows * len(pairs)
        width = 64 if cols <= 64 else 128
        print(json.dumps(dict(workload=name, cols=cols, images=len(descs), rows=a.rows, pairs=len(pairs), launches=info[1], ms_median=round(float(np.median(ts)), 4),
                              ms_min=round(min(ts), 4), ms_events=round(ev, 4), comparisons=comparisons,
                              comparisons_per_s_events=round(comparisons / (ev * 1e-3), 1), valu_ops_per_s_events=round(comparisons * 3 * width / (ev * 1e-3), 1),
                              matches=[int(v) for v in cnt.cpu().numpy()[0][:4]], device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
