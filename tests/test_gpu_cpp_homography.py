"""The C++ mirror of the homography stage: tests/cpp/homography_demo.cpp through isx::BestOf2NearestMatcher (operator() on ImageFeatures),
plain g++ against the C-ABI library, compared with the NumPy models - matches by count, H and confidence by their bits, masks and
num_inliers exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import homography_np as hm  # noqa: E402
from helpers import match_np as M  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cpp_homography_demo(gpu, tmp_path):
    from test_gpu_homography import _synthetic_features
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    exe = str(tmp_path / "homography_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "homography_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip", "-Wl,-rpath," + lib_dir])
    rows = [60, 0, 45, 8]
    descs, kps, sizes = _synthetic_features(21, rows, 30)
    pairs = M.near_pairs(rows)
    want_m = M.match_model(descs, pairs, 0.3, kps, sizes)
    d = tmp_path / "in"
    d.mkdir()
    args = [exe, str(d), "0.3"]
    for k in range(len(rows)):
        descs[k].tofile(str(d / ("desc%d.bin" % k)))
        kps[k].tofile(str(d / ("kp%d.bin" % k)))
        args += [str(rows[k]), str(sizes[k][0]), str(sizes[k][1])]
    out = subprocess.check_output(args, text=True, timeout=300)
    lines = out.split("\n")
    assert "launches 1" in lines, out
    got = [ln.split()[1:] for ln in lines if ln.startswith("pair")]
    assert len(got) == len(pairs), out
    seen_h = 0
    for (i, j), w, g in zip(pairs, want_m, got):
        want = hm.find_homography_np(w["points"])
        assert want["margin"] >= 1e-9
        assert [int(v) for v in g] == [i, j, w["count"], int(want["stats"][1]), int(want["stats"][0]), int(np.float64(want["conf"]).view(np.uint64))], (g, want["stats"])
        H = np.fromfile(str(d / ("H_%d_%d.bin" % (i, j))), np.float64)
        mask = np.fromfile(str(d / ("mask_%d_%d.bin" % (i, j))), np.uint8)
        if want["stats"][0] & hm.ST_H:
            seen_h += 1
            assert np.array_equal(H.view(np.uint64), want["H"].reshape(9).view(np.uint64))
        else:
            assert H.size == 0
        assert np.array_equal(mask, want["mask"] if want["mask"] is not None else np.zeros(0, np.uint8))
    assert seen_h >= 1
