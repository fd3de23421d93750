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


def _hamming_whole(q, t):
    """hamming as it was before it blocked over train rows: one lookup table, one temporary per 256 queries."""
    q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
    out = np.zeros((q.shape[0], t.shape[0]), np.int32)
    for r0 in range(0, q.shape[0], 256):
        out[r0:r0 + 256] = M._POP[q[r0:r0 + 256, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)
    return out


def _knn2_whole(q, t):
    """knn2 as it was: a stable argsort of every whole row of distances."""
    nq, nt = q.shape[0], t.shape[0]
    out = np.full((nq, 4), -1, np.int32)
    if nq == 0 or nt == 0:
        return out
    d = _hamming_whole(q, t)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    rows = np.arange(nq)
    out[:, 0], out[:, 1] = order[:, 0], d[rows, order[:, 0]]
    if nt >= 2:
        out[:, 2], out[:, 3] = order[:, 1], d[rows, order[:, 1]]
    return out


def test_blocked_hamming_and_knn2_equal_the_whole_row_forms(monkeypatch):
    """On the hand case, the degenerate cases (0, 1 and 2 rows, all rows identical) and a 300 x 700 random case with duplicated rows - at
    the module's block size (one block) and at blocks of 7 queries x 9 and 1 train rows, so that ties and both neighbours cross blocks."""
    a, b, _ = cases.hand_case()
    pairs = [(a, b)] + [(c[0][0], c[0][1]) for c in cases.degenerate_cases().values()]
    rng = np.random.default_rng(300700)
    big_q, big_t = cases.random_rows(rng, 300), cases.random_rows(rng, 700)
    big_t[rng.integers(0, 700, 120)] = big_t[rng.integers(0, 700, 120)]      # duplicates: ties of the first and of the second neighbour
    big_q[:40] = big_t[rng.integers(0, 700, 40)]
    pairs.append((big_q, big_t))
    for q_block, block_bytes in ((M._Q_BLOCK, M.BLOCK_BYTES), (7, 32 * 7 * 9), (7, 32 * 7)):
        monkeypatch.setattr(M, "_Q_BLOCK", q_block)
        monkeypatch.setattr(M, "BLOCK_BYTES", block_bytes)
        for x, y in pairs:
            for q, t in ((x, y), (y, x)):
                q, t = q.reshape(-1, 32), t.reshape(-1, 32)
                assert np.array_equal(M.hamming(q, t), _hamming_whole(q, t))
                got, want = M.knn2(q, t), _knn2_whole(q, t)
                assert got.dtype == want.dtype and np.array_equal(got, want), (q.shape, t.shape, block_bytes)
    assert M.BLOCK_BYTES <= 64 << 20


def test_chunk_plan_of_the_split_shapes():
    """The host's plan (csrc/match.hip: chunk_rows = TRAIN_CHUNK * ceil(nt / (TRAIN_CHUNK * 32))) for every train-row count
    tests/test_gpu_match_split.py names: if the rule is retuned, those shapes stop meaning what their names say."""
    want = {8191: (256, 32), 8192: (256, 32), 8193: (512, 17), 16384: (512, 32), 16385: (768, 22), 1 << 20: (32768, 32)}
    assert {nt: cases.chunk_plan(nt) for nt in want} == want
    src = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "match.hip")).read()
    assert "MT_MAX_SPLIT = %d;" % cases.MAX_SPLIT in src and "MT_CHUNK * cdiv(nt, MT_CHUNK * MT_MAX_SPLIT)" in src


@pytest.mark.parametrize("n_from,n_to", [(200, 8193), (8193, 140), (130, 16385)])
def test_split_pair_plants_what_it_says(n_from, n_to):
    a, b, planted = cases.split_pair(7, n_from, n_to)
    want = M.match_model([a, b], [(0, 1)], 0.3)[0]
    cases.check_split_planted(want, planted)
    assert planted["rows"]["roomy"] == (max(n_from, n_to) != 8193)


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
    assert sorted(seen) == sorted(fuzz_match.BASE_CLASSES), seen      # case(seed) alone draws the six it drew before `split`
    for cls in fuzz_match.CLASSES:
        assert fuzz_match.case(1, cls)["cls"] == cls


def _case_digest(c):
    import hashlib
    h = hashlib.sha256()
    for a in c["descriptors"] + c["keypoints"]:
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(repr((c["cls"], c["pairs"], c["img_sizes"], c["match_conf"], c["layout_seed"], None if c["mask"] is None else c["mask"].tolist())).encode())
    return h.hexdigest()[:16]


def test_the_split_class_is_drawn_and_the_older_classes_draw_what_they_drew():
    """A soak's first 200 cases (scheduled(): the classes in turn) hold the `split` class at every k and on either side, so chunks of 512
    and 768 rows and the cap of 32 chunks; its planted structure is found by the model; and case(seed, cls) of the six older classes gives
    the bytes it gave before `split` was added (digests taken from the generator as it was)."""
    import fuzz_match
    plans, orders, fillers = set(), set(), 0
    for n in range(200):
        s, cls = fuzz_match.scheduled(20261119, n)
        if cls != "split":
            continue
        c = fuzz_match.case(s, cls)
        rows = [d.shape[0] for d in c["descriptors"]]
        big, small = max(rows), min(rows)
        assert c["cls"] == "split" and c["pairs"] == [(0, 1)] and 4 <= small <= 300 and big % 8192 in (0, 1, 8191) and 8191 <= big <= 3 * 8192 + 1
        plans.add(cases.chunk_plan(big))
        orders.add(rows[0] > rows[1])
        if n < 60:                                                    # the model on a few: every kind of match is there
            rec = M.match_model(c["descriptors"], c["pairs"], c["match_conf"])[0]
            assert min(rec["kinds"]) >= 1 and tuple(c["planted"][0]["mutual"][0]) in {tuple(r) for r in rec["matches"]}, (s, rec["kinds"])
    assert {p[0] for p in plans} == {256, 512, 768, 1024} and {(256, 32), (512, 17), (768, 22)} <= plans and orders == {True, False}, plans
    assert sum(1 for n in range(200) if fuzz_match.scheduled(1, n)[1] == "split") >= 28
    want = {(1, "tiny"): "26878bdf4cb09a3b", (2, "chunk_edges"): "f43082ce0b01939e", (3, "clustered"): "ebcaa54c07e4a270", (4, "many"): "b5b260d59fef53e3",
            (6, "duplicates"): "5366dfb48a2e34f0"}
    assert {k: _case_digest(fuzz_match.case(*k)) for k in want} == want
    assert (fuzz_match.case(0)["cls"], _case_digest(fuzz_match.case(0))) == ("many", "28fb6ae79a4501f0")
    assert (fuzz_match.case(5)["cls"], _case_digest(fuzz_match.case(5))) == ("clustered", "2b27b71ac35dcdb6")


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
