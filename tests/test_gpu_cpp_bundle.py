"""The C++ mirror of the bundle adjuster: tests/cpp/bundle_demo.cpp through isx::BundleAdjusterRay (setConfThresh, operator() on features,
pairwise_matches and cameras, the reference's shape), plain g++ against the C-ABI library, compared with the model - cameras, the float32 K
and R and the two error norms by their bits, the rig's stats exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_cases as cases  # noqa: E402
import fuzz_bundle as fz  # noqa: E402
from helpers import bundle_np as bm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    path = str(tmp_path_factory.mktemp("bundle") / "bundle_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bundle_demo.cpp"), "-o", path, "-L", lib_dir, "-limagestitch_hip", "-Wl,-rpath," + lib_dir])
    return path


@pytest.mark.parametrize("name", ["two_images_8_inliers", "tiles_5", "camera_without_edge", "rig_without_edge", "nan_focal_in"])
def test_cpp_bundle_demo(gpu, exe, tmp_path, name):
    c = cases.named()[name]
    n, npairs = len(c["sizes"]), len(c["pairs"])
    np.concatenate(c["keypoints"]).astype(np.float32).tofile(str(tmp_path / "keypoints.bin"))
    np.array([[i, j, int(s[0]), m.shape[0]] for (i, j), s, m in zip(c["pairs"], c["stats"], c["matches"])], np.int32).tofile(str(tmp_path / "pairs.bin"))
    np.ascontiguousarray(c["conf"], np.float64).tofile(str(tmp_path / "conf.bin"))
    np.concatenate(c["matches"]).astype(np.int32).tofile(str(tmp_path / "matches.bin"))
    np.concatenate(c["masks"]).astype(np.uint8).tofile(str(tmp_path / "masks.bin"))
    np.ascontiguousarray(c["cameras_in"], np.float64).tofile(str(tmp_path / "cameras_in.bin"))
    np.ascontiguousarray(c["est_rig_stats"][0], np.int32).tofile(str(tmp_path / "est.bin"))
    args = [exe, str(tmp_path), repr(c["conf_thresh"]), str(c["max_iter"]), str(npairs)]
    for s, k in zip(c["sizes"], c["keypoints"]):
        args += [str(s[0]), str(s[1]), str(k.shape[0])]
    out = subprocess.check_output(args, text=True, timeout=300)
    lines = out.split("\n")
    assert "launches 1" in lines, out
    want = fz.run_model(c)
    assert [int(v) for v in [ln for ln in lines if ln.startswith("rig")][0].split()[1:]] == want[2][0].tolist(), out
    passes = bool(want[2][0, 0] & (bm.ST_NAN | bm.ST_NO_EDGES | bm.ST_EST_ASSERT))
    assert ("ok 0" if passes else "ok 1") in lines, out
    cams = np.fromfile(str(tmp_path / "cameras.bin"), np.float64).reshape(n, 16)
    kr = np.fromfile(str(tmp_path / "kr32.bin"), np.float32).reshape(n, 18)
    err = np.fromfile(str(tmp_path / "err.bin"), np.float64).reshape(1, 2)
    assert fz.same(cams, want[0]) and fz.same(kr, want[1]) and fz.same(err, want[3])
