"""isx::OrbFeaturesFinder through the OpenCV-free C++ mirror (include/imagestitch.hpp; tests/cpp/orb_demo.cpp), compiled with plain g++
against the C-ABI library: the keypoints and descriptors the demo dumps equal the NumPy model's (tests/helpers/orb_np.py) bit for bit, and
the matcher takes them as they come."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_cases as cases  # noqa: E402
from helpers import match_np  # noqa: E402
from helpers import orb_np as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_orb_demo_matches_the_model(gpu, tmp_path):
    exe = str(tmp_path / "orb_demo")
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-Wsuggest-override", "-Woverloaded-virtual", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "orb_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    scene = cases.scene(200, 420, 41, 3)
    imgs = [np.ascontiguousarray(scene[:, 0:360]), np.ascontiguousarray(scene[:, 60:420])]
    for i, im in enumerate(imgs):
        im.tofile(str(tmp_path / ("img%d.raw" % i)))
    out = subprocess.check_output([exe, "360", "200", "3", str(tmp_path / "img0.raw"), str(tmp_path / "img1.raw"), str(tmp_path / "o")], text=True)
    lines = out.splitlines()
    want = [M.find(im, M.Params()) for im in imgs]
    rec = np.dtype([("f", np.float32, 6), ("d", np.uint8, 32)])
    for i, w in enumerate(want):
        assert lines[i] == "image %d keypoints %d status %d size 360 200" % (i, w.count, w.status), lines[i]
        got = np.fromfile(str(tmp_path / ("o_%d.raw" % i)), rec)
        assert w.count > 50 and len(got) == w.count
        assert np.array_equal(got["f"][:, 0:2], w.keypoints) and np.array_equal(got["f"][:, 2:6], w.meta) and np.array_equal(got["d"], w.descriptors)
    m = match_np.match_pair(want[0].descriptors, want[1].descriptors, 0.3)[0]
    assert lines[2] == "matches %d" % len(m) and len(m) > 0
    assert lines[-2:] == ["throws 1", "throws 1"]          # ISX_ERR_INVALID: a pattern point outside the patch, nlevels = 9
