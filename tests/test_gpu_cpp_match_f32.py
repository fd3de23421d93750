"""The C++ mirror on float descriptors: tests/cpp/matcher_f32_demo.cpp through isx::BestOf2NearestMatcher (operator() on ImageFeatures
whose descriptors are CV_32FC1), plain g++ against the C-ABI library, compared with the NumPy models - matches and their float32 distances
exactly, H and confidence by their bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import homography_np as hm  # noqa: E402
from helpers import match_f32_np as MF  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cpp_matcher_f32_demo(gpu, tmp_path):
    from test_gpu_match_f32_chain import features
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    exe = str(tmp_path / "matcher_f32_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "matcher_f32_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip", "-Wl,-rpath," + lib_dir])
    d2, k2, s2, _ = features(33, 70, 45)
    descs = [d2[0], np.zeros((0, 64), np.float32), d2[1]]          # an image without features between the two
    kps, sizes, rows = [k2[0], np.zeros((0, 2), np.float32), k2[1]], [s2[0], (640, 480), s2[1]], [70, 0, 70]
    pairs = MF.near_pairs(rows)
    assert pairs == [(0, 2)]
    want_m = MF.match_model(descs, pairs, 0.3, kps, sizes)
    d = tmp_path / "in"
    d.mkdir()
    args = [exe, str(d), "0.3", "64"]
    for k in range(len(rows)):
        descs[k].tofile(str(d / ("desc%d.bin" % k)))
        kps[k].tofile(str(d / ("kp%d.bin" % k)))
        args += [str(rows[k]), str(sizes[k][0]), str(sizes[k][1])]
    out = subprocess.check_output(args, text=True, timeout=300)
    lines = out.split("\n")
    assert "launches 2" in lines and "mixed 2" in lines, out       # host mats: search and finalise; mixed types: ISX_ERR_TYPE
    got = [ln.split()[1:] for ln in lines if ln.startswith("pair")]
    assert len(got) == 1, out
    (i, j), w, g = pairs[0], want_m[0], got[0]
    want = hm.find_homography_np(w["points"])
    assert want["margin"] >= 1e-9 and w["count"] >= 40 and want["stats"][0] & hm.ST_H
    assert [int(v) for v in g] == [i, j, w["count"], int(want["stats"][1]), int(want["stats"][0]), int(np.float64(want["conf"]).view(np.uint64))], (g, want["stats"])
    assert np.array_equal(np.fromfile(str(d / ("matches_%d_%d.bin" % (i, j))), np.int32).reshape(-1, 3), w["matches"])
    H = np.fromfile(str(d / ("H_%d_%d.bin" % (i, j))), np.float64)
    assert np.array_equal(H.view(np.uint64), want["H"].reshape(9).view(np.uint64))
