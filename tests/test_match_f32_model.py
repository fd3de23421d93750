"""The float features matcher's NumPy model (tests/helpers/match_f32_np.py) and the cases of tests/match_f32_cases.py, without a GPU: each
case does what it is for."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_match_f32  # noqa: E402
import match_f32_cases as cases  # noqa: E402
from helpers import match_f32_np as MF  # noqa: E402
from helpers import match_np as M  # noqa: E402

F32 = np.float32
INF_BITS = 0x7F800000


def test_sqdist_is_the_stated_chain_and_maps_non_finite_to_inf():
    rng = np.random.default_rng(1)
    q, t = rng.standard_normal((5, 37)).astype(F32), rng.standard_normal((6, 37)).astype(F32)
    s = MF.sqdist(q, t)
    assert s.dtype == F32 and all(s[i, j] == cases.s_stated(q[i], t[j]) for i in range(5) for j in range(6))
    q[0, 3], t[1, 5], t[2, 0] = np.nan, np.inf, 3e38
    q[3, 0] = -3e38
    s = MF.sqdist(q, t)
    assert np.isposinf(s[0]).all() and np.isposinf(s[:, 1]).all() and np.isposinf(s[3, 2]) and not np.isnan(s).any()
    assert np.isfinite(s[1, 0]) and (s >= 0).all() and not np.signbit(s).any()


def test_knn_orders_by_s_then_row_whatever_the_blocking(monkeypatch):
    rng = np.random.default_rng(2)
    q, t = rng.integers(-3, 4, (40, 3)).astype(F32), rng.integers(-3, 4, (300, 3)).astype(F32)      # many equal s
    want = MF.knn2(q, t)
    s = MF.sqdist(q, t)
    for i in range(40):
        order = sorted(range(300), key=lambda r: (s[i, r], r))[:2]
        assert list(want[i, [0, 2]]) == order and list(want[i, [1, 3]]) == [cases.bits(np.sqrt(s[i, r])) for r in order]
    monkeypatch.setattr(MF, "BLOCK_ELEMS", 40 * 7)
    assert np.array_equal(MF.knn2(q, t), want)
    one = MF.knn2(q, t[:1])
    assert (one[:, 0] == 0).all() and (one[:, 2:] == -1).all()
    assert (MF.knn2(q, t[:0]) == -1).all() and MF.knn2(q[:0], t).shape == (0, 4)


def test_hand_case():
    a, b, want = cases.hand_case()
    m, k12, k21, kinds = MF.match_pair(a, b, 0.3)
    assert np.array_equal(m, want) and m.shape == (14, 3)
    assert kinds == (10, 2, 2)
    assert k12[20, 1] == k12[20, 3] == cases.bits(3) and k21[20, 1] == k21[20, 3] == cases.bits(4)
    assert np.array_equal(MF.from_bits(m[:, 2]), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 4, 4, 3, 3], F32))


def test_rounding_table():
    descs, pairs = cases.rounding_cases()
    want = MF.match_model(descs, pairs, cases.ROUNDING_CONF)
    for (d0, d1), w in zip(cases.ROUNDING, want):
        assert w["count"] == 1 and list(MF.from_bits(w["knn"][0][0, [1, 3]])) == [d0, d1] and w["matches"][0, 2] == cases.bits(d0)
        assert not Fraction(d0) < Fraction(35, 100) * d1                   # exact arithmetic rejects: 7j = 0.35 * 20j
    assert [w["count"] for w in MF.match_model(descs, pairs, 0.66)] == [0] * 12
    # 0.3 and 0.5 show no difference between float32 and exact arithmetic over the same integer range
    d = np.arange(0, 241, dtype=np.int64)
    d0, d1 = np.meshgrid(d, d, indexing="ij")
    for conf, num, den in ((0.3, 7, 10), (0.5, 1, 2)):
        k = M.ratio_k(conf)
        f32 = d0.astype(F32) < (k * d1.astype(F32)).astype(F32)
        assert np.array_equal(f32, den * d0 < num * d1), conf
    k = M.ratio_k(0.65)
    assert ((d0.astype(F32) < (k * d1.astype(F32)).astype(F32)) != (100 * d0 < 35 * d1)).sum() >= 12


@pytest.mark.parametrize("cols", [64, 128])
def test_order_sensitive_rows(cols):
    """All three reorderings give other bits for the nearest row's s and change which row is nearest: a kernel that reorders shows in knn."""
    a, b, (q, x, y) = cases.order_pair(cols)
    sx, sy = cases.s_stated(q, x), cases.s_stated(q, y)
    assert sx < sy
    for name, fn in cases.VARIANTS:
        assert fn(q, x) != sx, name
        assert fn(q, y) < fn(q, x), name
    assert sum(Fraction(float(v)) ** 2 for v in (q - x)) == sum(Fraction(float(v)) ** 2 for v in (q - y))       # equal in exact arithmetic
    assert cases.round_f32(Fraction(1, 3)) == F32(1 / 3) and cases.round_f32(Fraction(2 ** 24 + 1)) == F32(2 ** 24)   # ties to even
    rec = MF.match_model([a, b], [(0, 1)], 0.3)[0]
    assert list(rec["knn"][0][0, [0, 2]]) == [1, 0] and MF.sqdist(a[:1], b[1:2])[0, 0] == sx


def test_special_values():
    sp = cases.special_cases()
    w = MF.match_model(*sp["ties"])[0]
    k12, k21 = w["knn"]
    assert list(k12[0]) == [0, cases.bits(2), 1, cases.bits(2)]                       # equal s, the lower row first
    assert list(k12[1]) == [2, cases.bits(3), 3, cases.bits(3)] and list(k12[2]) == [4, 0, 5, 0]      # three at 3: rows 2, 3 before 6; s0 = s1 = 0
    got = {(int(r[0]), int(r[1])) for r in w["matches"]}
    assert (3, 7) in got and not MF.accepted(k12, 0.3)[2] and {(2, 4), (2, 5)} <= got       # 0 < k * 0 is false; the duplicates accept from their side
    w = MF.match_model(*sp["zero_nearest"])[0]
    assert [tuple(r) for r in w["matches"][:2]] == [(0, 0, 0), (1, 2, 0)]
    w = MF.match_model(*sp["subnormal"])[0]
    s = MF.sqdist(sp["subnormal"][0][0][:1], sp["subnormal"][0][1][:2])[0]
    assert 0 < s[0] < s[1] < np.finfo(F32).tiny                                       # subnormal squares, kept apart
    assert tuple(w["matches"][0][:2]) == (0, 0) and w["knn"][0][0, 2] == 1
    w = MF.match_model(*sp["overflow"])[0]
    k12 = w["knn"][0]
    assert list(k12[0, [0, 2]]) == [3, 4] and list(k12[1]) == [0, INF_BITS, 1, INF_BITS] and list(k12[2, [0, 2]]) == [0, 2]
    a, big = sp["overflow"][0]
    assert np.isposinf(MF.sqdist(a[:1], big[2:3])[0, 0]) and F32(1.5e19) * F32(1.5e19) < np.finfo(F32).max       # the sum overflows, no term does
    assert np.isposinf(MF.sqdist(a[:1], big[:1])[0, 0]) and np.isposinf(MF.sqdist(a[2:], big[3:])).all()          # e * e overflows
    k21 = w["knn"][1]
    assert list(k21[1]) == [0, INF_BITS, 1, INF_BITS] and k21[0, 1] == cases.bits(1) and k21[0, 3] == INF_BITS
    assert (2, 0) in {(int(r[0]), int(r[1])) for r in w["matches"]}                   # from row 0 of `big`: d0 = 1 < k * inf
    w = MF.match_model(*sp["overflow_all"])[0]
    assert w["count"] == 0 and all(list(r) == [0, INF_BITS, 1, INF_BITS] for r in w["knn"][0])
    ws = MF.match_model(*sp["nonfinite"])
    for w in ws:                                                                      # the queries with a NaN / an inf: every s = +inf, rows 0, 1
        assert all(list(w["knn"][0][q]) == [0, INF_BITS, 1, INF_BITS] for q in (1, 2))
    assert list(ws[0]["knn"][0][0]) == [0, cases.bits(1), 1, INF_BITS] and (0, 0) in {(int(r[0]), int(r[1])) for r in ws[0]["matches"]}      # NaN row second
    assert list(ws[1]["knn"][0][0]) == [0, INF_BITS, 1, INF_BITS] and list(ws[2]["knn"][0][3]) == [0, INF_BITS, 1, INF_BITS]                  # nearest and both
    assert ws[1]["count"] == ws[2]["count"] == 0
    assert list(ws[3]["knn"][0][0, [0, 2]]) == [4, 0] and list(ws[3]["knn"][0][3, [0, 2]]) == [2, 0]
    for w in ws:                                                                      # 2->1: a train row with a NaN / an inf has every s = +inf
        assert not np.isnan(MF.from_bits(w["knn"][1][:, [1, 3]])).any()


@pytest.mark.parametrize("cols", cases.WIDTHS)
def test_widths(cols):
    a, b, planted = cases.planted_pair(100 + cols, 20, 23, cols)
    assert a.shape == (20, cols) and a.dtype == F32
    cases.check_planted(MF.match_model([a, b], [(0, 1)], 0.3)[0], planted)


def test_shapes_sit_on_the_tiling_constants():
    from imagestitch_amd import matcher
    assert (matcher.QUERY_BLOCK, matcher.F32_TRAIN_TILE, matcher.TRAIN_CHUNK, matcher.F32_MAX_COLS) == (128, 32, 256, 128)
    hdr = open(os.path.join(ROOT, "include", "imagestitch_hip.h"), encoding="utf-8").read()
    assert "ISX_MATCH_F32_TRAIN_TILE = %d, ISX_MATCH_F32_MAX_COLS = %d" % (matcher.F32_TRAIN_TILE, matcher.F32_MAX_COLS) in hdr
    sh = cases.shapes()
    assert {127, 128, 129} <= {s[0] for s in sh} and {31, 32, 33, 255, 256, 257} <= {s[1] for s in sh}
    for nf, nt in sh[:3]:
        a, b, planted = cases.planted_pair(1000 * nf + nt, nf, nt, 9)
        cases.check_planted(MF.match_model([a, b], [(0, 1)], 0.3)[0], planted)


def test_degenerate_shapes():
    dg = cases.degenerate_cases()
    for name in ("0x5", "5x0"):
        w = MF.match_model(*dg[name])[0]
        assert w["skipped"] and w["count"] == 0
    assert MF.match_model(*dg["1x5"])[0]["count"] == 1 and MF.match_model(*dg["5x1"])[0]["count"] == 1
    assert MF.match_model(*dg["1x1"])[0]["count"] == 0 and MF.match_model(*dg["1x2"])[0]["count"] == 1
    assert MF.match_model(*dg["2x2"])[0]["count"] == 2
    ws = MF.match_model(*dg["empty_among_live"])
    assert [w["skipped"] for w in ws] == [True, False, True, False, False] and ws[1]["count"] > 10


@pytest.mark.parametrize("cls", fuzz_match_f32.CLASSES[:-1])
def test_fuzz_generator(cls):
    """Every class and a few seeds: shapes as its docstring says, and what is planted - mutual, 1->2 only, 2->1 only - survives in the model."""
    for n in range(3):
        c = fuzz_match_f32.case(fuzz_match_f32.scheduled(5, n)[0], cls)
        assert c["cls"] == cls and 1 <= c["cols"] <= 128 and all(d.dtype == F32 and d.shape[1] == c["cols"] for d in c["descriptors"])
        assert 0.0 <= c["match_conf"] <= 0.9
        want = MF.match_model(c["descriptors"], c["pairs"], c["match_conf"])
        for w, p in zip(want, c["planted"]):
            cases.check_planted(w, p)
    assert [fuzz_match_f32.scheduled(3, n)[1] for n in range(9)] == list(fuzz_match_f32.CLASSES)
    a, b = fuzz_match_f32.case(77, cls), fuzz_match_f32.case(77, cls)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["descriptors"], b["descriptors"]))


def test_fuzz_generator_split_rows():
    c = fuzz_match_f32.case(9, "split")
    rows = sorted(d.shape[0] for d in c["descriptors"])
    assert rows[1] in [8192 * k + e for k in (1, 2) for e in (-1, 0, 1)] and 4 <= rows[0] <= 300


def test_cpp_demo_compiles_against_the_header():
    demo = os.path.join(ROOT, "tests", "cpp", "matcher_f32_demo.cpp")
    subprocess.check_call(["g++", "-fsyntax-only", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), demo])
