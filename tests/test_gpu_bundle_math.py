"""imagestitch_amd/csrc/bundle_math.hpp as the device compiler builds it: isx_selftest_bundle_math_device runs one thread per item through
the same bm_* function that isx_selftest_bundle_math runs on the host, and both are held to the bits of the Python model
(tests/helpers/bundle_np.py, bundle_reproj_np.py) over the sweeps of tests/bundle_math_cases.py - every quadrant of the reduction with the
neighbours of its switches, the three branches of acos, cvRodrigues2 both ways at the identity, the half turn and the 1e-5 threshold, the polar
factor with det < 0, the 3 x 3 Jacobi in float64 and float32, and the camera matrices and residuals of rigs that go round.  NaNs compare by
position.  The adjusters' own suites reach these functions only through rigs; a narrow rig leaves most of their branches untaken
(tests/test_bundle_model.py::test_which_branches_the_named_cases_take)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundle_math_cases as mc  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
_DP = C.POINTER(C.c_double)


def _run(entry, name, rows):
    a = np.ascontiguousarray(rows, np.float64)
    out = np.full((a.shape[0], mc.N_OUT[name]), -7777.25)
    _lib.check(getattr(_lib.load(), entry)(mc.FN[name], a.shape[0], a.ctypes.data_as(_DP), out.ctypes.data_as(_DP)))
    return out


def _same(got, want):
    """Per row: equal bits, or a NaN in both."""
    return ((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all(axis=1)


@pytest.mark.parametrize("name", sorted(mc.FN, key=mc.FN.get))
def test_device_host_and_model_give_the_same_bits(gpu, name):
    rows, want = mc.sweeps()[name], mc.model(name)
    host, dev = _run("isx_selftest_bundle_math", name, rows), _run("isx_selftest_bundle_math_device", name, rows)
    assert host.shape == dev.shape == want.shape
    for who, got in (("host", host), ("device", dev)):
        bad = np.flatnonzero(~_same(got, want))
        assert bad.size == 0, (name, who, "%d of %d rows differ" % (bad.size, rows.shape[0]),
                               [(rows[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]])


def test_the_device_entry_refuses_what_the_host_entry_refuses(gpu):
    lib = _lib.load()
    a, out = np.zeros(14), np.full(14, -7777.25)
    for fn, n, pin, pout in ((-1, 1, a, out), (12, 1, a, out), (0, -1, a, out), (0, 1, None, out), (0, 1, a, None)):
        args = (fn, n, None if pin is None else pin.ctypes.data_as(_DP), None if pout is None else pout.ctypes.data_as(_DP))
        assert lib.isx_selftest_bundle_math(*args) == lib.isx_selftest_bundle_math_device(*args) != 0, (fn, n)
    assert lib.isx_selftest_bundle_math_device(0, 0, None, None) == 0 and (out == -7777.25).all()
