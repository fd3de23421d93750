"""The NumPy model of cv::resize and of the scaled mask stage (tests/helpers/resize_np.py) - the standard of record for isx_resize and
isx_mask_dilate_resize_and - checked on known answers, and the library's host arithmetic (imagestitch_amd/csrc/resize_taps.hpp through
blocks_gain_host.hpp's resize_tables) checked against it.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import resize_np as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_known_answers():
    assert R.resize(np.array([[0, 255]], np.uint8), (4, 1), R.LINEAR).tolist() == [[0, 64, 191, 255]]
    assert R.resize(np.array([[1, 2], [3, 5]], np.uint8), (1, 1), R.LINEAR).tolist() == [[3]]
    rng = np.random.default_rng(1)
    for shape in ((7, 9), (7, 9, 3), (1, 1), (1, 6, 3)):
        u = rng.integers(0, 256, shape, dtype=np.uint8)
        f = (rng.standard_normal(shape) * 1e3).astype(F32)
        for interp in (R.LINEAR, R.NEAREST):
            assert np.array_equal(R.resize(u, (shape[1], shape[0]), interp), u)
            assert np.array_equal(R.resize(f, (shape[1], shape[0]), interp), f)


def test_coefficient_pairs_are_not_normalised():
    """a0 = rint((1 - fx) * 2048) and a1 = rint(fx * 2048) are rounded each on its own.  Over the 19 columns of a 7 -> 19 upscale every sum is
    2048 (the three clamped columns 0, 9 and 18 carry (2048, 0)): 1 - fx is exact in float for fx >= 0.5, and below that its rounding error,
    at most 2^-25, moves (1 - fx) * 2048 by 2^-14, which changes rint only where fx * 2048 lies that close to a half - none of these columns.
    An fx that does lie there gives 2047 or 2049: fx = 513.5 / 2048 - 2^-25 rounds 1 - fx up to a tie that goes to the even 1534 while
    fx * 2048 = 513.4999 goes to 513.  The model computes both roundings and never 2048 - a1."""
    sx, fx = R.col_taps(7, 19)
    a0, a1 = R.coef((F32(1) - fx).astype(F32)), R.coef(fx)
    assert sx.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6]
    assert a1.tolist() == [0, 108, 862, 1617, 323, 1078, 1832, 539, 1293, 0, 755, 1509, 216, 970, 1725, 431, 1186, 1940, 0]
    assert (a0 + a1).tolist() == [2048] * 19
    f = F32(np.float64(513.5) / 2048 - 2.0 ** -25)
    assert (int(R.coef(f)), int(R.coef(F32(1) - f))) == (513, 1534)                  # 2047
    f = F32(np.float64(600.5) / 2048 + 2.0 ** -25)
    assert (int(R.coef(f)), int(R.coef(F32(1) - f))) == (601, 1448)                  # 2049


def test_exact_half_rule_needs_both_ratios():
    rng = np.random.default_rng(2)
    s = rng.integers(0, 256, (8, 12), dtype=np.uint8)
    area = ((s[0::2, 0::2].astype(int) + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(R.resize(s, (6, 4)), area)
    assert R.is_half((8, 12), (4, 6)) and not R.is_half((8, 12), (4, 12)) and not R.is_half((8, 12), (8, 6)) and not R.is_half((4, 6), (8, 12))
    # half in x only: the general path, whose fixed point differs from the two-pixel mean somewhere
    gx = R.resize(s, (6, 8))
    sx, fx = R.col_taps(12, 6)
    assert fx.tolist() == [0.5] * 6 and sx.tolist() == [0, 2, 4, 6, 8, 10]
    si = s.astype(np.int64)
    want = (((2048 * ((si[:, 0::2] * 1024 + si[:, 1::2] * 1024) >> 4)) >> 16) + 2) >> 2
    assert np.array_equal(gx, want.astype(np.uint8))
    f = (rng.standard_normal((8, 12, 3)) * 1e6).astype(F32)
    fa = ((((f[0::2, 0::2] + f[0::2, 1::2]).astype(F32) + f[1::2, 0::2]).astype(F32) + f[1::2, 1::2]).astype(F32) * F32(0.25)).astype(F32)
    assert np.array_equal(R.resize(f, (6, 4)), fa)
    # an upscale by two is not the rule either
    up = R.resize(s, (24, 16))
    assert up.shape == (16, 24) and not np.array_equal(up[0::2, 0::2], s)
    # NEAREST never takes it
    assert np.array_equal(R.resize(s, (6, 4), R.NEAREST), s[0::2, 0::2])


def test_dilate_resize_and_model():
    m = np.zeros((5, 6), np.uint8)
    m[0, 0] = m[4, 5] = m[2, 3] = 255
    d = R.dilate(m, 3, 3)
    assert d[:2, :2].min() == 255 and d[3:, 4:].min() == 255 and d[1:4, 2:5].min() == 255 and d[0, 3] == 0 and d[4, 0] == 0
    assert np.array_equal(R.dilate(m, 1, 1), m)
    # an even element: anchor (kw / 2, kh / 2) reaches one further up and left
    d2 = R.dilate(m, 2, 2)
    assert d2[2, 3] == 255 and d2[3, 4] == 255 and d2[1, 2] == 0 and d2[3, 3] == 255 and d2[2, 4] == 255
    w = np.random.default_rng(3).integers(0, 256, (11, 13), dtype=np.uint8)
    out = R.dilate_resize_and(m, w, 3, 3)
    assert np.array_equal(out, R.resize(d, (13, 11)) & w)
    assert np.array_equal(R.dilate_resize_and(m, None, 3, 3, (13, 11)), R.resize(d, (13, 11)))
    assert len(np.unique(R.resize(d, (13, 11)))) > 2          # the grey ramp stays


def test_resize_tables_give_the_models_taps(tmp_path):
    """blocks_gain_host.hpp's resize_tables, now a loop over resize_taps.hpp's col_tap / row_tap (what the kernels of resize.hip call per pixel),
    built with the host compiler as tests/test_blocks_gain_model.py builds it, on 50 seeded size pairs."""
    exe = str(tmp_path / "blocks_gain_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "blocks_gain_host.cpp"),
                           "-o", exe])
    rng = np.random.default_rng(20261018)
    pairs = [(1, 1, 5, 7), (9, 1, 4, 3), (45, 31, 131, 101), (131, 101, 45, 31), (106, 74, 53, 37), (300, 3, 1100, 5), (7, 7, 19, 19)]
    while len(pairs) < 50:
        pairs.append(tuple(int(v) for v in rng.integers(1, 400, 4)))
    text = "".join("tables %d %d %d %d\n" % p for p in pairs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 50
    for (sw, sh, dw, dh), line in zip(pairs, lines):
        t = line.split()
        sx, fx = R.col_taps(sw, dw)
        sy0, sy1, fy = R.row_taps(sh, dh)
        assert len(t) == 2 * dw + 3 * dh
        assert [int(v) for v in t[0:2 * dw:2]] == sx.tolist(), (sw, dw)
        assert np.array_equal(np.array([float.fromhex(v) for v in t[1:2 * dw:2]], F32), fx), (sw, dw)
        r = t[2 * dw:]
        assert [int(v) for v in r[0::3]] == sy0.tolist() and [int(v) for v in r[1::3]] == sy1.tolist(), (sh, dh)
        assert np.array_equal(np.array([float.fromhex(v) for v in r[2::3]], F32), fy), (sh, dh)


def test_dsize_from_factors_rounds_half_to_even():
    from imagestitch_amd.resize import resize_dsize
    assert resize_dsize(5, 7, 0.5, 0.5) == (2, 4)          # 2.5 -> 2, 3.5 -> 4
    assert resize_dsize(3, 1, 0.5, 0.5) == (2, 0)          # 1.5 -> 2, 0.5 -> 0
    assert resize_dsize(160, 96, 0.4, 0.4) == (64, 38)     # 38.4 -> 38
    assert resize_dsize(3840, 2160, 0.1098, 0.1098) == (422, 237)


def test_header_and_loader_declare_both_entries():
    text = open(os.path.join(ROOT, "include", "imagestitch_hip.h")).read()
    assert re.search(r"int isx_resize\(const isx_mat\* src, isx_mat\* dst, int interpolation, int device, void\* hip_stream\);", text)
    assert re.search(r"int isx_mask_dilate_resize_and\(const isx_mat\* seam_mask, const isx_mat\* warped_mask, int kw, int kh, isx_mat\* out, int device, "
                     r"void\* hip_stream\);", text)
    from imagestitch_amd import _lib
    assert {"isx_resize", "isx_mask_dilate_resize_and"} <= set(_lib.declared_symbols())
    mirror = open(os.path.join(ROOT, "include", "imagestitch.hpp")).read()
    assert "inline void resize(" in mirror and "inline void dilateResizeAnd(" in mirror


def test_resize_kernels_issue_no_flat_access():
    """the taps come through typed global pointers: no FLAT load or store in any kernel of resize.o (tools/isa_flat.py, as tests/test_isa_flat.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_flat
    path = os.path.join(ROOT, "imagestitch_amd", "csrc", "build", "resize.o")
    if not os.path.exists(path):
        subprocess.check_call(["bash", os.path.join(ROOT, "imagestitch_amd", "csrc", "build.sh")])
    res = isa_flat.scan(path)
    names = isa_flat.demangle(list(res))
    assert sum("k_resize<" in names[k] for k in res) == 12 and sum("k_dilate_resize_and<" in names[k] for k in res) == 4, sorted(names.values())
    bad = {names[k]: dict(c) for k, c in res.items() if c["flat_load"] or c["flat_store"] or c["flat_atomic"]}
    assert not bad, bad
    assert all(c["global_store"] for c in res.values())
