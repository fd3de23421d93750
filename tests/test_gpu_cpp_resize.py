"""isx::resize and isx::dilateResizeAnd through the OpenCV-free C++ mirror (include/imagestitch.hpp; tests/cpp/resize_demo.cpp), compiled with
plain g++ against the C-ABI library: the files the demo dumps equal the NumPy model's (tests/helpers/resize_np.py) byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import resize_np as R  # noqa: E402

from imagestitch_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_resize_demo_matches_the_model(gpu, tmp_path):
    exe = str(tmp_path / "resize_demo")
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-Wsuggest-override", "-Woverloaded-virtual", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "resize_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H = 150, 94                                  # 0.5 -> 75 x 47 (the area rule), 0.4 -> 60 x 38 (37.6 rounds up)
    rng = np.random.default_rng(77)
    img = synth.make_tile(H, W, 3)
    seam = np.where(rng.random((23, 31)) < 0.2, 255, 0).astype(np.uint8)
    warped = np.where(rng.random((91, 127)) < 0.8, 255, 0).astype(np.uint8)
    img.tofile(str(tmp_path / "img.raw"))
    seam.tofile(str(tmp_path / "seam.raw"))
    warped.tofile(str(tmp_path / "warped.raw"))
    out = subprocess.check_output([exe, str(W), str(H), str(tmp_path / "img.raw"), "31", "23", str(tmp_path / "seam.raw"), "127", "91",
                                   str(tmp_path / "warped.raw"), str(tmp_path / "o")], text=True)
    shapes = {t[0]: (int(t[1]), int(t[2]), int(t[3])) for t in (line.split() for line in out.splitlines()) if len(t) == 4}
    assert out.splitlines()[-2:] == ["throws 6", "throws 7"]          # ISX_ERR_UNSUPPORTED for INTER_CUBIC, ISX_ERR_SIZE for an empty dsize

    def got(name, dtype, shape):
        assert shapes[name][:2] == shape[:2], (name, shapes[name])
        return np.fromfile(str(tmp_path / ("o_%s.raw" % name)), dtype).reshape(shape)

    assert np.array_equal(got("half", np.uint8, (47, 75, 3)), R.resize(img, (75, 47)))
    assert np.array_equal(got("small", np.uint8, (38, 60, 3)), R.resize(img, (60, 38)))
    assert np.array_equal(got("nearest", np.uint8, (H - 5, W + 7, 3)), R.resize(img, (W + 7, H - 5), R.NEAREST))
    assert np.array_equal(got("small_f", np.float32, (38, 60, 3)), R.resize(img.astype(np.float32), (60, 38)))
    assert np.array_equal(got("grey", np.uint8, (91, 127)), R.dilate_resize_and(seam, None, 3, 3, (127, 91)))
    assert np.array_equal(got("composed", np.uint8, (91, 127)), R.dilate_resize_and(seam, warped, 3, 3))
    assert np.array_equal(got("inplace", np.uint8, (91, 127)), R.dilate_resize_and(seam, warped, 20, 20))
