"""CPU-side checks of the boundary: the C-ABI library loads without a GPU and exports every symbol
include/imagestitch_hip.h declares, fails loudly (no CPU fallback), and the host-side geometry /
byte-model helpers agree with the oracle and SURVEY §8(d)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "imagestitch_hip.h")


@pytest.fixture(scope="module")
def libpath():
    from imagestitch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["bash", os.path.join(ROOT, "imagestitch_amd", "csrc", "build.sh")])
    return _lib.LIB_PATH


def test_header_is_valid_c_and_cpp():
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", HEADER])
    subprocess.check_call(["g++", "-fsyntax-only", "-x", "c++", "-std=c++11", "-Wall", "-Werror", HEADER])


def test_library_exports_every_declared_symbol(libpath):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(isx_[a-z0-9_]+)\s*\(", text)))
    assert len(declared) >= 30
    lib = C.CDLL(libpath)
    missing = [n for n in declared if not hasattr(lib, n)]
    assert not missing, missing
    from imagestitch_amd import _lib
    assert sorted(_lib.declared_symbols()) == declared, set(declared) ^ set(_lib.declared_symbols())


def test_no_cpu_fallback_without_gpu(libpath):
    """On a box without a GPU every compute entry point must fail with ISX_ERR_HIP, never compute."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import imagestitch_amd as I
    with pytest.raises(I.IsxError) as e:
        I.CylindricalWarper().create(100.0)
    assert e.value.code == 4
    with pytest.raises(I.IsxError) as e:
        I.MultiBandBlender(False, 5, I.PREC_I16)
    assert e.value.code == 4


def test_every_entry_is_behind_the_exception_barrier(libpath):
    """SURVEY §5 "no exceptions across the boundary": (1) every `int isx_*` definition under csrc/ is a function-try-block
    (ISX_ENTRY ... ISX_EXIT("its own name")), bar the three one-liners that cannot throw; (2) the barrier works: exceptions thrown inside a
    guarded entry - incl. two REAL allocation failures of std::vector - come back as ISX_ERR_NOMEM / ISX_ERR_INTERNAL with a message, in a
    child process that would otherwise die of std::terminate."""
    csrc = os.path.join(ROOT, "imagestitch_amd", "csrc")
    entries, bad = 0, []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".cpp", ".hip")):
            continue
        src = open(os.path.join(csrc, f), errors="replace").read()
        for m in re.finditer(r"^(?:int|void|const char\*) (isx_\w+)\(", src, re.M):
            name = m.group(1)
            head = src[m.start():src.index("{", m.start()) + 1]
            if name in ("isx_last_error", "isx_version", "isx_profile_enable"):
                continue
            entries += 1
            if "ISX_ENTRY" not in head or ('} ISX_EXIT("%s")' % name) not in src:
                bad.append((f, name))
    assert entries >= 80 and not bad, bad
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
lib.isx_last_error.restype = C.c_char_p
out = []
for kind in range(7):
    rc = lib.isx_selftest_exception_barrier(kind)
    out.append((kind, rc, lib.isx_last_error().decode()))
for o in out: print(o)
want = {0: 5, 1: 5, 2: 5, 3: 9, 4: 9, 5: 9, 6: 0}
assert all(rc == want[k] for k, rc, _ in out), out
assert all(("isx_selftest_exception_barrier" in msg) == (k < 6) for k, _, msg in out), out
print("BARRIER OK")
"""
    r = subprocess.run([os.sys.executable, "-c", code, libpath], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "BARRIER OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under imagestitch_amd/ may reference it."""
    pkg = os.path.join(ROOT, "imagestitch_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h", ".sh")):
                src = open(os.path.join(dp, f), errors="replace").read()
                assert "liboracle" not in src and "from oracle" not in src and "import oracle" not in src and "oracle/" not in src.replace("the oracle", ""), f


def test_as_mat_and_enums():
    from imagestitch_amd import _lib
    a = np.zeros((5, 7, 3), np.uint8)
    m = _lib.as_mat(a)
    assert (m.rows, m.cols, m.type, m.step, m.device) == (5, 7, 16, 21, -1)
    m = _lib.as_mat(np.zeros((4, 6), np.float32)[:, :5])
    assert (m.cols, m.type, m.step) == (5, 5, 24)
    # one row: NumPy keeps whatever stride the array's history left on a dimension of length 1 (here 3, on a C-contiguous array); the mat's
    # step is a row's bytes (the fuzz family case_resize met this as "step 3 smaller than a row")
    one = np.broadcast_to(np.zeros((1, 70, 1), np.int64), (1, 70, 3)).astype(np.uint8)
    assert one.flags["C_CONTIGUOUS"] and one.strides[0] == 3
    m = _lib.as_mat(one)
    assert (m.rows, m.cols, m.step) == (1, 70, 210)
    assert _lib.as_mat(np.zeros((1, 9), np.float32)).step == 36
    try:
        import torch
        assert _lib.as_mat(torch.from_numpy(one)).step == 210
    except ImportError:  # pragma: no cover
        pass
    assert _lib.as_mat(np.zeros((2, 2, 3), np.int16)).type == 19 and _lib.as_mat(np.zeros((2, 2, 3), np.float32)).type == 21
    with pytest.raises(_lib.IsxError):
        _lib.as_mat(np.zeros((4, 6, 3), np.uint8)[:, :, ::-1])
    with pytest.raises(_lib.IsxError):
        _lib.as_mat(np.zeros((4, 6, 2), np.uint8))
    text = open(HEADER).read()
    for name, val in (("ISX_8UC3", 16), ("ISX_16SC3", 19), ("ISX_32FC1", 5), ("ISX_32FC3", 21), ("ISX_BORDER_REFLECT", 2), ("ISX_BLEND_MULTI_BAND", 2)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), text), name


def test_geometry_helpers_match_oracle(oracle):
    from imagestitch_amd.pipeline import feed_geometry, prepare_geometry
    rng = np.random.default_rng(2)
    for _ in range(20):
        n = int(rng.integers(1, 4))
        corners = [(int(rng.integers(-50, 200)), int(rng.integers(-40, 60))) for _ in range(n)]
        sizes = [(int(rng.integers(20, 300)), int(rng.integers(20, 200))) for _ in range(n)]
        bands = int(rng.integers(0, 7))
        roi, fin, L = prepare_geometry(corners, sizes, bands)
        ob = oracle.MultiBand(bands, 0)
        ob.prepare(corners, sizes)
        assert L == ob.num_bands and fin == ob.result_size()
        lap, _ = ob.level(0)
        assert lap.shape[:2] == (roi[3], roi[2])
        for c, s in zip(corners, sizes):
            w, h = feed_geometry(roi, L, c, s)
            assert w % (1 << L) == 0 and h % (1 << L) == 0 and w <= roi[2] and h <= roi[3]


def test_byte_model_matches_survey():
    """FEED(F32, L=5) = 76.6 B per tile-base pixel with i16x3 + u8 input (73.6 with the
    fused u8x3 input this build feeds: 3 B less at each of the two level-0 reads... the constant is
    checked with the model's own 7 B input), BLEND(F32, L=5) = 36.3 B per mosaic pixel."""
    from imagestitch_amd.pipeline import model_bytes
    from imagestitch_amd import _lib
    m = model_bytes([0], [0], [1e6], 1e6, _lib.PREC_F32, 5)
    assert abs(m["blend"] / 1e6 - 36.3) < 0.1
    # this build reads u8x3 + u8 (4 B) instead of i16x3 + u8 (7 B) at level 0: 76.6 - 2*3 = 70.6
    assert abs(m["feed"] / 1e6 - 70.6) < 0.1
    m = model_bytes([0], [0], [1e6], 1e6, _lib.PREC_I16, 5)
    assert abs(m["blend"] / 1e6 - 24.3) < 0.1 and abs(m["feed"] / 1e6 - (52.6 - 6.0)) < 0.1
    m = model_bytes([8294400], [7398000], [0], 0, _lib.PREC_F32, 5)
    assert m["warp"] == 3 * 8294400 + 4 * 7398000


def test_the_opencv_ab_probe_never_raises_and_says_what_it_found():
    """tools/opencv_ab.py is called from smoke() on every box: where no cv2 imports it must say so in one line and compare nothing; where one does, it
    must return a verdict per check (strings / dicts), never raise (a probe, not a gate)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import opencv_ab
    res = opencv_ab.run(verbose=False)
    assert isinstance(res.get("opencv"), str) and isinstance(res.get("checks"), dict)
    cv2, what = opencv_ab.probe()
    if cv2 is None:
        assert res["checks"] == {} and what.startswith("no cv2")
    else:
        assert res["checks"], res
