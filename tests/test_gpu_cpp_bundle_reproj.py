"""The C++ mirrors of the reprojection adjuster and the wave correction: tests/cpp/bundle_reproj_demo.cpp through isx::BundleAdjusterReproj
(setConfThresh, setRefinementMask, operator() on features, pairwise_matches and cameras) and isx::waveCorrect, plain g++ against the C-ABI
library, compared with the Python path on the same case - cameras, the float32 K and R and the two error norms by their bits, the rig's
stats exactly - and with the model."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_reproj_cases as cases  # noqa: E402
import fuzz_bundle_reproj as fz  # noqa: E402
from helpers import bundle_reproj_np as rp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    path = str(tmp_path_factory.mktemp("bundle_reproj") / "bundle_reproj_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bundle_reproj_demo.cpp"), "-o", path, "-L", lib_dir, "-limagestitch_hip", "-Wl,-rpath," + lib_dir])
    return path


@pytest.mark.parametrize("name,kind", [("two_images_8_inliers", 0), ("tiles_5", 1), ("camera_without_edge", 0), ("rig_without_edge", 0),
                                       ("nan_focal_in", 1), ("refine_flags_1", 0)])
def test_cpp_bundle_reproj_demo(gpu, exe, tmp_path, name, kind):
    from imagestitch_amd import adjuster as adj
    c = cases.named()[name]
    n, npairs = len(c["sizes"]), len(c["pairs"])
    np.concatenate(c["keypoints"]).astype(np.float32).tofile(str(tmp_path / "keypoints.bin"))
    np.array([[i, j, int(s[0]), m.shape[0]] for (i, j), s, m in zip(c["pairs"], c["stats"], c["matches"])], np.int32).tofile(str(tmp_path / "pairs.bin"))
    np.ascontiguousarray(c["conf"], np.float64).tofile(str(tmp_path / "conf.bin"))
    np.concatenate(c["matches"]).astype(np.int32).tofile(str(tmp_path / "matches.bin"))
    np.concatenate(c["masks"]).astype(np.uint8).tofile(str(tmp_path / "masks.bin"))
    np.ascontiguousarray(c["cameras_in"], np.float64).tofile(str(tmp_path / "cameras_in.bin"))
    np.ascontiguousarray(c["est_rig_stats"][0], np.int32).tofile(str(tmp_path / "est.bin"))
    args = [exe, str(tmp_path), repr(c["conf_thresh"]), str(c["max_iter"]), str(npairs), str(c["refine_flags"]), str(kind)]
    for s, k in zip(c["sizes"], c["keypoints"]):
        args += [str(s[0]), str(s[1]), str(k.shape[0])]
    out = subprocess.check_output(args, text=True, timeout=300)
    lines = out.split("\n")
    assert "launches 1" in lines, out
    py, info = fz.run_library(c, "host")                           # the Python path on host mats, as the C++ class calls the library
    want = fz.run_model(c)
    assert info == (1, 1) and all(fz.same(a, b) for a, b in zip(py, want))
    assert [int(v) for v in [ln for ln in lines if ln.startswith("rig")][0].split()[1:]] == py[2][0].tolist(), out
    passes = bool(py[2][0, 0] & (rp.ST_NAN | rp.ST_NO_EDGES | rp.ST_EST_ASSERT))
    assert ("ok 0" if passes else "ok 1") in lines, out
    cams = np.fromfile(str(tmp_path / "cameras.bin"), np.float64).reshape(n, 16)
    kr = np.fromfile(str(tmp_path / "kr32.bin"), np.float32).reshape(n, 18)
    err = np.fromfile(str(tmp_path / "err.bin"), np.float64).reshape(1, 2)
    assert fz.same(cams, py[0]) and fz.same(kr, py[1]) and fz.same(err, py[3])
    wouts = (np.zeros((n, 16)), np.zeros((n, 18), np.float32), np.zeros((1, 2), np.int32))
    assert adj.wave_correct(py[0], *wouts, kind=kind) == (1, 1)
    wc = np.fromfile(str(tmp_path / "wave_cameras.bin"), np.float64).reshape(n, 16)
    wk = np.fromfile(str(tmp_path / "wave_kr32.bin"), np.float32).reshape(n, 18)
    assert fz.same(wc, wouts[0]) and fz.same(wk, wouts[1]) and ("wave %d" % (wouts[2][0, 0] == 0)) in lines, out
    assert all(fz.same(a, b) for a, b in zip(wouts, rp.wave_correct(py[0], None, kind)))
