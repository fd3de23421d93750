"""The fisheye and stereographic projectors through the C++ host side, compiled with plain g++ against the C-ABI library: the OpenCV-free
mirror (include/imagestitch.hpp: isx::FisheyeWarper, isx::StereographicWarper; tests/cpp/polar_demo.cpp).  Its dumps - warped tiles, masks,
maps, corners, warped points - equal the NumPy model's (tests/helpers/polar_np.py) bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import polar_np as P  # noqa: E402

from imagestitch_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_polar_demo_matches_the_model(gpu, oracle, tmp_path):
    exe = str(tmp_path / "polar_demo")
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-Wsuggest-override", "-Woverloaded-virtual", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "polar_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    W, H, F = 210, 130, 165.0
    imgs = [synth.make_tile(H, W, 50 + i) for i in range(2)]
    for i in range(2):
        imgs[i].tofile(str(tmp_path / ("in%d.raw" % i)))
    out = subprocess.check_output([exe, str(W), str(H), str(F), str(tmp_path / "in0.raw"), str(tmp_path / "in1.raw"), str(tmp_path / "o")], text=True)
    corners, points = {}, {}
    for line in out.splitlines():
        t = line.split()
        if t[0] == "corner":
            corners[int(t[1])] = (int(t[2]), int(t[3]))
        elif t[0] == "point":
            points[int(t[1])] = (np.float32(t[2]), np.float32(t[3]))
    assert "throws 6" in out          # setTranslation on a fisheye warper -> ISX_ERR_UNSUPPORTED
    K, Rs = synth.camera_pair(W, H, F, yaw=0.2)
    for i, kind in enumerate((P.FISHEYE, P.STEREOGRAPHIC)):
        m = P.from_rig(kind, F, K, Rs[i])
        roi, _ = m.detect_roi(W, H)
        xm, ym = m.build_maps(roi)
        wi = oracle.remap(imgs[i], xm, ym, oracle.LINEAR, oracle.BORDER_REFLECT)
        wm = oracle.remap(np.full((H, W), 255, np.uint8), xm, ym, oracle.NEAREST, oracle.BORDER_CONSTANT)
        assert corners[i] == (int(roi[0]), int(roi[1]))
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_warped%d.raw" % i)), np.uint8).reshape(wi.shape), wi)
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_mask%d.raw" % i)), np.uint8).reshape(wm.shape), wm)
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_xmap%d.raw" % i)), np.float32).reshape(xm.shape), xm)
        assert np.array_equal(np.fromfile(str(tmp_path / ("o_ymap%d.raw" % i)), np.float32).reshape(ym.shape), ym)
        u, v = m.map_forward(np.float32(W - 1.0), np.float32(0.25 * H))
        assert points[i] == (u, v), (points[i], u, v)
