"""csrc/proj_math.hpp as the device compiler builds it: isx_selftest_proj_math_device runs one thread per item through the same function
isx_selftest_proj_math runs on the host, on the sweep tests/test_polar_model.py holds against the NumPy model - bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from test_polar_model import _fp, run_math  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fn", sorted(PC.NAMES))
def test_device_math_equals_the_host_bit_for_bit(gpu, fn):
    a, b = PC.sweep(fn)
    host, dev = run_math("isx_selftest_proj_math", fn, a, b), run_math("isx_selftest_proj_math_device", fn, a, b)
    bad = np.flatnonzero(~((host.view(np.uint32) == dev.view(np.uint32)) | (np.isnan(host) & np.isnan(dev))))
    assert bad.size == 0, (PC.NAMES[fn], a[bad[:4]], None if b is None else b[bad[:4]], host[bad[:4]], dev[bad[:4]])


def test_device_entry_checks_its_arguments(gpu):
    lib = gpu.load()
    a = np.zeros(4, np.float32)
    for args in ((5, 4, _fp(a), None, _fp(a)), (-1, 4, _fp(a), None, _fp(a)), (PC.ATAN2, 4, _fp(a), None, _fp(a)), (0, 4, None, None, _fp(a)), (0, -1, _fp(a), None, _fp(a))):
        assert lib.isx_selftest_proj_math(*args) == lib.isx_selftest_proj_math_device(*args) == 1, args
    out = np.full(4, -7777.25, np.float32)
    assert lib.isx_selftest_proj_math_device(0, 0, None, None, None) == 0 and (out == -7777.25).all()
