"""The plane projector through the C++ host side, compiled with plain g++ against the C-ABI library: the OpenCV-free mirror
(include/imagestitch.hpp: isx::PlaneWarper, RotationWarper::setTranslation / warpPoint; tests/cpp/plane_demo.cpp) and the OpenCV adapter
(include/imagestitch_cv_plane.hpp: isx_cv::HipPlaneWarper with cv::detail::PlaneWarper's T overloads; tests/cpp/cv_plane_demo.cpp, against
tests/cpp/opencv_stub_plane in front of tests/cpp/opencv_stub).  Their dumps - warped tiles, masks, maps, corners, warped points - equal
the NumPy model's (tests/helpers/plane_np.py) bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import plane_np as P  # noqa: E402

from imagestitch_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("demo", ["plane_demo", "cv_plane_demo"])
def test_cpp_plane_demo_matches_the_model(gpu, oracle, tmp_path, demo):
    exe = str(tmp_path / demo)
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    inc = ["-I", os.path.join(ROOT, "include")]
    if demo == "cv_plane_demo":
        inc = ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub_plane"), "-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub")] + inc
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-Wsuggest-override", "-Woverloaded-virtual"] + inc +
                          [os.path.join(ROOT, "tests", "cpp", demo + ".cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, F = 420, 260, 330.0
    T = np.array([0.125, -0.0625, 0.03125], np.float32)           # exact in decimal: the demo parses the same floats
    imgs = [synth.make_tile(H, W, 50 + i) for i in range(2)]
    for i in range(2):
        imgs[i].tofile(str(tmp_path / ("in%d.raw" % i)))
    out = subprocess.check_output([exe, str(W), str(H), str(F), str(tmp_path / "in0.raw"), str(tmp_path / "in1.raw"), str(tmp_path / "o")] +
                                  [repr(float(t)) for t in T], text=True)
    corners, points = {}, {}
    for line in out.splitlines():
        t = line.split()
        if t[0] == "corner":
            corners[int(t[1])] = (int(t[2]), int(t[3]))
        elif t[0] == "point":
            points[int(t[1])] = (np.float32(t[2]), np.float32(t[3]))
    assert "throws 6" in out          # setTranslation on a cylindrical warper -> ISX_ERR_UNSUPPORTED
    K, Rs = synth.camera_pair(W, H, F, yaw=0.2)
    for i in range(2):
        m = P.from_rig(oracle, F, K, Rs[i], None if i == 0 else T)
        c, wi, roi = m.warp(imgs[i], oracle.LINEAR, oracle.BORDER_REFLECT)
        _, wm, _ = m.warp(np.full((H, W), 255, np.uint8), oracle.NEAREST, oracle.BORDER_CONSTANT)
        xm, ym = m.build_maps(roi)
        assert corners[i] == c
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_warped%d.raw" % i)), np.uint8).reshape(wi.shape), wi)
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_mask%d.raw" % i)), np.uint8).reshape(wm.shape), wm)
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_xmap%d.raw" % i)), np.float32).reshape(xm.shape), xm)
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_ymap%d.raw" % i)), np.float32).reshape(ym.shape), ym)
        u, v = m.map_forward(np.float32(W - 1.0), np.float32(0.25 * H))
        assert points[i] == (u, v), (points[i], u, v)
