"""The features matcher without a GPU: the NumPy model (tests/helpers/match_np.py) on a hand case, the float32 rounding of the ratio test,
the degenerate shapes, the generator of tools/fuzz_match.py, and the ABI (header, Python constants, the C++ demo)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import match_cases as cases  # noqa: E402
from helpers import match_np as M  # noqa: E402

HEADER = os.path.join(ROOT, "include", "imagestitch_hip.h")


def test_hand_case_gives_the_fourteen_matches():
    a, b, want = cases.hand_case()
    m, k12, k21, kinds = M.match_pair(a, b, 0.3)
    assert m.shape == (14, 3) and np.array_equal(m, want)
    assert kinds == (10, 2, 2)                                    # mutual, 1->2 only (the reverse fork), 2->1 only (the fork)
    assert tuple(k12[20]) in ((5, 3, 6, 3),) and tuple(k21[20]) == (30, 4, 31, 4)      # ties: the lower row first
    assert np.array_equal(m[12:], [(20, 5, 3), (20, 6, 3)])


def _exact_accept(d0, d1, conf_num, conf_den):
    return d0 * conf_den < (conf_den - conf_num) * d1            # d0 < (1 - conf) d1 in integers


def test_float32_ratio_test_differs_from_exact_arithmetic_in_twelve_cases_at_065():
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    knn = np.stack([np.zeros(d0.size, np.int32), d0.ravel().astype(np.int32), np.ones(d0.size, np.int32), d1.ravel().astype(np.int32)], axis=1)
    for conf, num, den in ((0.65, 65, 100), (0.3, 3, 10), (0.5, 1, 2)):
        got = M.accepted(knn, conf).reshape(257, 257)
        exact = _exact_accept(d0, d1, num, den)
        diff = sorted(zip(*np.nonzero(got != exact)))
        assert diff == (list(cases.ROUNDING) if conf == 0.65 else []), (conf, diff)
        if conf == 0.65:
            assert all(got[a, b] and not exact[a, b] for a, b in diff)      # float32 accepts all twelve
    k = M.ratio_k(0.65)
    assert k.dtype == np.float32 and float(k) > 0.35 and np.float32(7) < k * np.float32(20)
    assert not (7.0 < (1.0 - 0.65) * 20.0)                        # double rejects


def test_rounding_cases_have_the_distances_they_claim_and_are_accepted():
    descs, pairs = cases.rounding_cases()
    out = M.match_model(descs, pairs, cases.ROUNDING_CONF)
    for (d0, d1), rec in zip(cases.ROUNDING, out):
        assert sorted(rec["knn"][0][0, [1, 3]]) == [d0, d1]
        assert np.array_equal(rec["matches"], [(0, int(rec["knn"][0][0, 0]), d0)]), rec["matches"]
    assert all(r["count"] == 0 for r in M.match_model(descs, pairs, 0.66))      # k = 0.34: 6.8 j < 7 j


def test_degenerate_shapes():
    d = cases.degenerate_cases()
    r = {name: M.match_model(*c)[0] for name, c in d.items()}
    # 1 x 5: 1->2 has five candidates (2 and 9 bits away: 2 < 0.7 * 9), 2->1 one candidate: nothing
    assert np.array_equal(r["1x5"]["matches"], [(0, 0, 2)]) and tuple(r["1x5"]["knn"][1][0]) == (0, 2, -1, -1)
    # 5 x 1: n_to = 1 gives no 1->2 match; 2->1 runs against 5 candidates
    assert np.array_equal(r["5x1"]["matches"], [(0, 0, 2)]) and (r["5x1"]["knn"][0][:, 2:] == -1).all()
    for name in ("0x5", "5x0"):
        assert r[name]["skipped"] and r[name]["count"] == 0
    assert r["0x5"]["knn"][0].shape == (0, 4) and (r["0x5"]["knn"][1] == -1).all()
    assert np.array_equal(r["2x2"]["matches"], [(0, 0, 1), (1, 1, 2)]) and r["2x2"]["kinds"] == (2, 0, 0)
    assert r["identical"]["count"] == 0 and (r["identical"]["knn"][0][:, [1, 3]] == 0).all()
    assert np.array_equal(r["identical"]["knn"][0][:, [0, 2]], [[0, 1]] * 6)
    # match_conf = 0: k = 1, every unique nearest neighbour is accepted - the fork's tie still is not
    c0, planted = r["conf0"], cases.planted_pair(11, 24, 23)[2]
    assert c0["count"] > M.match_model(d["conf0"][0], [(0, 1)], 0.3)[0]["count"]
    assert planted["fork"][0] not in c0["matches"][: c0["kinds"][0] + c0["kinds"][1], 0]
    with np.errstate(all="raise"):
        assert M.ratio_k(0.0) == np.float32(1.0)


def test_knn_orders_ties_by_row_and_matches_do_not_depend_on_it():
    a, b, _ = cases.planted_pair(3, 30, 40, "duplicates")
    m, k12, _, _ = M.match_pair(a, b, 0.3)
    d = M.hamming(a, b)
    for q in range(a.shape[0]):
        i0, d0, i1, d1 = k12[q]
        assert (d0, i0) < (d1, i1) and d[q, i0] == d0 and d[q, i1] == d1
        rest = np.delete(np.arange(b.shape[0]), [i0, i1])
        assert all((d1, i1) < (d[q, r], r) for r in rest)
    perm = np.random.default_rng(5).permutation(b.shape[0])      # b2[r] = b[perm[r]]
    m2 = M.match_pair(a, b[perm], 0.3)[0]
    back = m2.copy()
    back[:, 1] = perm[m2[:, 1]]
    n12 = int(M.accepted(k12, 0.3).sum())
    assert np.array_equal(back[:n12], m[:n12])                    # 1->2: in query order either way
    assert sorted(map(tuple, back[n12:])) == sorted(map(tuple, m[n12:]))      # 2->1: in order of the permuted rows


def test_every_generator_class_appears_and_every_case_exercises_the_three_kinds():
    import fuzz_match
    seen = {}
    for seed in range(200):
        c = fuzz_match.case(seed)
        seen[c["cls"]] = seen.get(c["cls"], 0) + 1
        assert c["pairs"] and 0.0 <= c["match_conf"] < 1.0
        for rec, planted in zip(M.match_model(c["descriptors"], c["pairs"], c["match_conf"]), c["planted"]):
            assert min(rec["kinds"]) >= 1, (seed, c["cls"], rec["kinds"])
            got = {tuple(r) for r in rec["matches"]}
            fa, fb1, fb2 = planted["fork"]
            rb, ra1, ra2 = planted["reverse_fork"]
            assert {(fa, fb1, 3), (fa, fb2, 3), (ra1, rb, 4), (ra2, rb, 4), planted["mutual"][0]} <= got, (seed, c["cls"])
    assert sorted(seen) == sorted(fuzz_match.CLASSES), seen
    for cls in fuzz_match.CLASSES:
        assert fuzz_match.case(1, cls)["cls"] == cls


def test_header_declares_the_entries_and_the_constants_match_python():
    from imagestitch_amd import _lib, matcher
    text = open(HEADER).read()
    for name, val in (("ISX_MATCH_QUERY_BLOCK", matcher.QUERY_BLOCK), ("ISX_MATCH_TRAIN_TILE", matcher.TRAIN_TILE),
                      ("ISX_MATCH_TRAIN_CHUNK", matcher.TRAIN_CHUNK)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), text), name
    assert re.search(r"ISX_MATCH_MAX_ROWS\s*=\s*1 << 20\b", text) and matcher.MAX_ROWS == 1 << 20
    assert re.search(r"ISX_MATCH_MAX_TOTAL_ROWS\s*=\s*1 << 22\b", text) and matcher.MAX_TOTAL_ROWS == 1 << 22
    assert matcher.TRAIN_CHUNK % matcher.TRAIN_TILE == 0 and matcher.TRAIN_TILE == matcher.QUERY_BLOCK
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+isx_match_features\s*\(([^;]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == len(_lib._SIGS["isx_match_features"]) == 14
    assert re.search(r"int\s+isx_match_release\s*\(\s*void\s*\)\s*;", code) and _lib._SIGS["isx_match_release"] == []
    src = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "match.hip")).read()
    assert "MT_Q = ISX_MATCH_QUERY_BLOCK" in src and "MT_T = ISX_MATCH_TRAIN_TILE" in src and "MT_CHUNK = ISX_MATCH_TRAIN_CHUNK" in src
    import imagestitch_amd
    assert imagestitch_amd.FeaturesMatcher is matcher.FeaturesMatcher


def test_near_pairs_follow_the_reference():
    from imagestitch_amd.matcher import FeaturesMatcher
    rows = [5, 0, 7, 3]
    assert FeaturesMatcher.near_pairs(rows) == [(0, 2), (0, 3), (2, 3)] == M.near_pairs(rows)
    mask = np.ones((4, 4), np.uint8)
    mask[0, 3] = 0
    mask[3, 2] = 0                                                # below the diagonal: never read
    assert FeaturesMatcher.near_pairs(rows, mask) == [(0, 2), (2, 3)] == M.near_pairs(rows, mask)


def test_cpp_demo_compiles_against_the_header():
    demo = os.path.join(ROOT, "tests", "cpp", "matcher_demo.cpp")
    subprocess.check_call(["g++", "-fsyntax-only", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), demo])
