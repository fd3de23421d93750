"""The features matcher (isx_match_features) past the shapes of tests/test_gpu_match.py, against the NumPy model with np.array_equal under
the rules of its check_against_model (sentinels past the count untouched, no tolerance anywhere):
  the split regime   train images past 8 192 rows, where a work item's chunk grows to 512 and 768 rows, the last chunk is not whole tiles
                     (or is a single row) and k_mt_finalise merges up to 32 partials a query; structure planted at the chunk boundaries
                     (match_cases.split_pair), ties and neighbour pairs that straddle chunks
  the row limits     2^20 rows in one image (chunks of 32 768 rows, rows >= 2^16 and 2^20 - 1 in the key distance << 22 | row, 4 096 steps of
                     one finalise block) and 2^22 rows in all (packed offsets 3 * 2^20 and 2^22 - 24), accepted; one row more, refused
  many pairs         64 images, all 2 016 near pairs in one call: a finalise grid of 2 016, a work table of 4 032 items
tests/test_match_model.py pins the chunk plan of every row count named here (match_cases.chunk_plan)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_cases as cases  # noqa: E402
import test_gpu_match as TM  # noqa: E402  (its run_raw and check_against_model)
from helpers import match_np as M  # noqa: E402
from imagestitch_amd import matcher  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = TM.SENTINEL
P20 = 1 << 20
SPLIT_SHAPES = [(200, 8191), (200, 8192), (200, 8193), (130, 16384), (130, 16385), (8193, 140)]
HOST_TOO = [(200, 8193), (8193, 140)]


@pytest.fixture(scope="module", autouse=True)
def release_the_large_buffers():
    yield
    import torch
    matcher.FeaturesMatcher.release()
    torch.cuda.empty_cache()


def _room(need):
    """The rule of tests/test_gpu_addressing_limits.py: skip only when the device has less free memory than the test holds plus 2 GiB."""
    import torch
    if torch.cuda.mem_get_info()[0] < need + (2 << 30):
        torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need + (2 << 30):
        pytest.skip("needs %.1f GiB + 2 GiB, the device has %.1f GiB free" % (need / 2.0**30, free / 2.0**30))


@pytest.mark.parametrize("n_from,n_to", SPLIT_SHAPES)
def test_split_shapes(gpu, n_from, n_to):
    """0.05 - 0.3 s a case on an MI355X box, the model included (0.6 s for 200 x 8 193 on a slower CPU)."""
    a, b, planted = cases.split_pair(1000 * n_from + n_to, n_from, n_to)
    rows = planted["rows"]
    assert (rows["crows"], rows["nch"]) == cases.chunk_plan(max(n_from, n_to)) and planted["big_is_from"] == (n_from > n_to)
    kps, sizes = cases.keypoints_for(n_from + n_to, [n_from, n_to])
    want = M.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    cases.check_split_planted(want[0], planted)
    for device in [True, False] if (n_from, n_to) in HOST_TOO else [True]:
        got, info = TM.run_raw([a, b], [(0, 1)], 0.3, kps, sizes, device=device)
        TM.check_against_model(got, want, "device" if device else "host")
        assert info == (1, 3 if device else 2)


def test_one_image_at_the_row_limit(gpu):
    """24 x 2^20 rows on device mats: chunks of 32 768 rows, 32 of them; mutual matches at train rows 32 767 / 32 768 (the first chunk
    boundary), 65 535 / 65 536 (the first rows past 16 bits) and 2^20 - 1 (every bit of a 20-bit row set, the last row of the last chunk: a
    query whose nearest row is the last and whose other train rows are random); one query is the complement of train row 2^20 - 1, so the key
    256 << 22 | 2^20 - 1 is formed - and must lose: a distance of 256 cannot show in knn at a high row, since it is the second smallest key
    only where every row is 256 away, and then rows 0 and 1 win the tie.  2->1 has 2^20 queries: 4 096 steps of the one finalise block,
    2^20 entries of acc.  1.2 s on an MI355X box (the model 2.2 s on a slower CPU); holds 0.3 GB."""
    _room(512 << 20)
    mutual = [32767, 32768, 65535, 65536, P20 - 1]
    a, b, planted = cases.planted_at(20, 24, P20, mutual)
    assert cases.chunk_plan(P20) == (32768, 32) and [r // 32768 for r in mutual] == [0, 1, 1, 2, 31]
    comp = int(planted["free"].pop())
    a[comp] = ~b[P20 - 1]
    kps, sizes = cases.keypoints_for(20, [24, P20])
    want = M.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    cases.check_planted_at(want[0], planted)
    k12, k21 = want[0]["knn"]
    assert int(M.hamming(a[comp:comp + 1], b[P20 - 1:])[0, 0]) == 256 and k12[comp, 1] > 64      # formed, and far from winning
    last = [s for s, r, _ in planted["mutual"] if r == P20 - 1][0]
    assert tuple(k12[last][:2]) == (P20 - 1, 4) and k12[last, 3] > 64 and k21.shape == (P20, 4)
    assert (k12[:, [0, 2]] >= 1 << 16).any() and want[0]["count"] >= 5
    got, info = TM.run_raw([a, b], [(0, 1)], 0.3, kps, sizes)
    TM.check_against_model(got, want)
    assert info == (1, 3)


def test_total_rows_at_the_cap_and_one_past_it(gpu):
    """Five device images of 2^20, 2^20, 2^20, 2^20 - 24 and 24 rows, 2^22 in all, and the one pair (3, 4): the searched images are packed
    at rows 3 * 2^20 and 2^22 - 24.  The same bytes as matching the two alone, and the model's.  Then a fifth image of 25 rows:
    ISX_ERR_UNSUPPORTED with every output at its sentinel.  1.3 s on an MI355X box (the model 2.2 s on a slower CPU); holds 0.5 GB."""
    import torch
    _room(640 << 20)
    n3 = P20 - 24
    assert 3 * P20 + n3 + 24 == matcher.MAX_TOTAL_ROWS
    b, a, planted = cases.planted_at(22, n3, 24, [0, 32767, 32768, n3 - 1])      # the big image first: pair (3, 4) is (big, small)
    assert planted["big_is_from"]
    zeros = np.zeros((P20, 32), np.uint8)                             # packed, never searched
    kps, sizes = cases.keypoints_for(22, [n3, 24])
    want = M.match_model([b, a], [(0, 1)], 0.3, kps, sizes)
    cases.check_planted_at(want[0], planted)
    alone, info = TM.run_raw([b, a], [(0, 1)], 0.3, kps, sizes)
    TM.check_against_model(alone, want, "alone")
    zk = np.zeros((P20, 2), np.float32)
    got, info5 = TM.run_raw([zeros, zeros, zeros, b, a], [(3, 4)], 0.3, [zk, zk, zk] + kps, [(8, 8)] * 3 + sizes)
    TM.check_against_model(got, want, "at the cap")
    for key in ("matches", "points"):
        assert np.array_equal(got[0][key], alone[0][key]), key
    assert all(np.array_equal(got[0]["knn"][d], alone[0]["knn"][d]) for d in range(2)) and info == info5 == (1, 3)
    # one row more
    dz = TM._dev(zeros)
    a25 = np.r_[a, a[:1]]
    outs = [TM._dev(np.full((n3 + 25, 3), SENTINEL, np.int32)), TM._dev(np.full((1, 1), SENTINEL, np.int32)), TM._dev(np.full((n3, 4), SENTINEL, np.int32)),
            TM._dev(np.full((25, 4), SENTINEL, np.int32))]
    TM._expect(TM.ERR_UNSUPPORTED, lambda: matcher.match_features([dz, dz, dz, TM._dev(b), TM._dev(a25)], [(3, 4)], 0.3, [outs[0]], outs[1], knn=outs[2:]))
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)


N_IMAGES, N_PAIRS = 64, 2016


def many_pairs_case():
    """64 images of 40 - 70 rows and their 2 016 near pairs; structure (fuzz_match.plant) in the 63 chain pairs (i, i + 1) - the first and
    the last pair of the list among them - and in 16 more spread over the list, random filler elsewhere."""
    import fuzz_match
    rng = np.random.default_rng(2016)
    rows = [int(rng.integers(40, 71)) for _ in range(N_IMAGES)]
    pairs = M.near_pairs(rows)
    assert len(pairs) == N_PAIRS and pairs[0] == (0, 1) and pairs[-1] == (62, 63)
    chain = [(i, i + 1) for i in range(N_IMAGES - 1)]
    more = []
    for k in range(1, 17):
        at = k * N_PAIRS // 17
        while pairs[at] in chain or pairs[at] in more:
            at += 1
        more.append(pairs[at])
    plant = sorted(chain + more)
    descs, planted = fuzz_match.build(rng, rows, plant)
    kps, sizes = cases.keypoints_for(2016, rows)
    return rows, pairs, plant, descs, planted, kps, sizes


def test_2016_pairs_in_one_call(gpu):
    """The whole call equals the model; 8 of the pairs matched alone give identical bytes.  The model takes 0.65 s of CPU for the 2 016 pairs,
    the test 0.7 s on an MI355X box."""
    rows, pairs, plant, descs, planted, kps, sizes = many_pairs_case()
    want = M.match_model(descs, pairs, 0.3, kps, sizes)
    assert len(plant) == 79 and pairs[0] in plant and pairs[-1] in plant
    for p, pl in zip(plant, planted):
        w = want[pairs.index(p)]
        assert min(w["kinds"]) >= 1 and tuple(pl["mutual"][0]) in {tuple(r) for r in w["matches"]}, p
    got, info = TM.run_raw(descs, pairs, 0.3, kps, sizes)
    TM.check_against_model(got, want)
    assert info == (N_PAIRS, 3)
    for k in (0, 1, 255, 256, 1023, pairs.index(plant[40]), 2014, 2015):
        i, j = pairs[k]
        alone, _ = TM.run_raw([descs[i], descs[j]], [(0, 1)], 0.3, [kps[i], kps[j]], [sizes[i], sizes[j]])
        for key in ("count", "matches", "points"):
            assert np.array_equal(alone[0][key], got[k][key]), (k, key)
        assert all(np.array_equal(alone[0]["knn"][d], got[k]["knn"][d]) for d in range(2)), k
