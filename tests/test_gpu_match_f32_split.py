"""The float features matcher past one chunk plan and past 2^31 bytes of packed rows: train images on both sides of 8 192 and 16 384 rows
(chunks of 512 and 768 rows) with matches planted at the chunk boundaries, and a searched pair packed behind device filler images that
bring the call to its row cap - 2^22 rows of 128 floats, a packed array of 2^31 bytes (the row cap lets it grow no further, so no byte of
it lies past 2^32; the offsets that pass 2^31 are those of its last rows, of the partials and of the accepted-row table behind it)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_cases as hamming_cases  # noqa: E402
import match_f32_cases as cases  # noqa: E402
import test_gpu_match_f32 as TM  # noqa: E402
from helpers import match_f32_np as MF  # noqa: E402
from imagestitch_amd import matcher  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
P20 = 1 << 20
SPLIT_SHAPES = [(40, 8191), (40, 8192), (40, 8193), (33, 16384), (33, 16385), (8193, 36)]


@pytest.fixture(scope="module", autouse=True)
def release_the_large_buffers():
    yield
    import torch
    matcher.FeaturesMatcher.release()
    torch.cuda.empty_cache()


def split_pair(seed, n_from, n_to, cols):
    """Isolated filler, and in the big image mutual matches at rows 0, crows - 1, crows, the first row of the middle and of the last chunk
    and the last row; one query of the small image with its nearest row at the end of chunk 0 and its second nearest at the start of the
    last chunk (a unit and two units away in one column); one with both in chunk 1 at one distance (a tie: rejected from its side)."""
    big_n, small_n = max(n_from, n_to), min(n_from, n_to)
    crows, nch = hamming_cases.chunk_plan(big_n)
    last = (nch - 1) * crows
    rng = np.random.default_rng(seed)
    big = (rng.random((big_n, cols)) * 2.0 - 1.0)
    big[:, 0] += 64.0 * (100 + np.arange(big_n))
    small = (rng.random((small_n, cols)) * 2.0 - 1.0)
    small[:, 0] -= 64.0 * (1 + np.arange(small_n))
    big, small = big.astype(F32), small.astype(F32)
    mutual = [0, crows - 1, crows, nch // 2 * crows, last] + ([big_n - 1] if big_n - 1 != last else [])
    free = list(rng.permutation(small_n))
    planted = dict(mutual=[], crows=crows, nch=nch)
    for t, r in enumerate(mutual):
        s = int(free.pop())
        big[r] = small[s]
        big[r, cols - 1] += F32(t / 8.0)
        planted["mutual"].append((s, r))
    unit = np.zeros(cols, F32)
    unit[cols - 1] = 1.0
    s = int(free.pop())
    base = np.round(small[s] * 1024) / 1024
    small[s] = base
    big[crows - 2], big[last + 1 if big_n - last > 2 else last - 1] = base + unit, base - 2 * unit
    planted["apart"] = (s, crows - 2, last + 1 if big_n - last > 2 else last - 1)
    s = int(free.pop())
    base = np.round(small[s] * 1024) / 1024
    small[s] = base
    big[crows + 3], big[crows + 9] = base + unit, base - unit
    planted["tie"] = (s, crows + 3, crows + 9)
    return (small, big, planted) if n_from < n_to else (big, small, planted)


def check_split(rec, planted, big_is_from):
    knn = rec["knn"][1 if big_is_from else 0]                  # the direction whose train rows are the big image's
    got = {(int(r[1]), int(r[0])) if big_is_from else (int(r[0]), int(r[1])) for r in rec["matches"]}
    for s, r in planted["mutual"]:
        assert (s, r) in got and knn[s, 0] == r, (s, r)
    s, r0, r1 = planted["apart"]
    assert list(knn[s]) == [r0, cases.bits(1), r1, cases.bits(2)] and (s, r0) in got and r0 // planted["crows"] == 0 and r1 // planted["crows"] >= planted["nch"] - 2
    s, r0, r1 = planted["tie"]
    assert list(knn[s]) == [r0, cases.bits(1), r1, cases.bits(1)]
    assert {(s, r0), (s, r1)} <= got                           # (accepted from the big side: each of the two has one near row)


@pytest.mark.parametrize("n_from,n_to", SPLIT_SHAPES)
def test_split_shapes(gpu, n_from, n_to):
    cols = 48 if (n_from + n_to) % 2 else 72
    a, b, planted = split_pair(1000 * n_from + n_to, n_from, n_to, cols)
    assert (planted["crows"], planted["nch"]) == ((256, 32) if max(n_from, n_to) <= 8192 else (512, 17) if max(n_from, n_to) == 8193 else
                                                  (512, 32) if max(n_from, n_to) == 16384 else (768, 22))
    kps, sizes = cases.keypoints_for(n_from + n_to, [n_from, n_to])
    want = MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    check_split(want[0], planted, n_from > n_to)
    for device in [True, False] if n_to == 8193 else [True]:
        got, info = TM.run_raw([a, b], [(0, 1)], 0.3, kps, sizes, device=device)
        TM.check_against_model(got, want, "device" if device else "host")
        assert info == (1, 3 if device else 2)


def test_the_packed_array_reaches_two_gib(gpu):
    """Six device images of 2^20, 2^20, 2^20, 2^20 - 700, 400 and 300 rows of 128 floats, 2^22 in all, and the one pair (4, 5): the
    searched images are packed in the last 358 400 bytes below 2^31.  The four fillers are ONE torch tensor made on the device (never on
    the host), packed four times and never searched.  The same bytes as matching the two alone, and the model's.  One row more:
    ISX_ERR_UNSUPPORTED with every output at its sentinel.  Holds 0.5 GiB of filler and a scratch of 2 GiB."""
    import torch
    need = P20 * 512 + (2 << 30) + (256 << 20)
    if torch.cuda.mem_get_info()[0] < need + (2 << 30):
        torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need + (2 << 30):
        pytest.skip("needs %.1f GiB + 2 GiB for the filler and the scratch; torch.cuda.mem_get_info shows %.1f GiB free" % (need / 2.0**30, free / 2.0**30))
    n4, n5, cols = 400, 300, 128
    assert 3 * P20 + (P20 - 700) + n4 + n5 == matcher.MAX_TOTAL_ROWS and matcher.MAX_TOTAL_ROWS * cols * 4 == 1 << 31
    filler = torch.full((P20, cols), 7.0, dtype=torch.float32, device="cuda")
    zk = torch.zeros((P20, 2), dtype=torch.float32, device="cuda")
    a, b, planted = cases.planted_pair(22, n4, n5, cols, "cloud")
    kps, sizes = cases.keypoints_for(22, [n4, n5])
    want = MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    cases.check_planted(want[0], planted)
    alone, info = TM.run_raw([a, b], [(0, 1)], 0.3, kps, sizes)
    TM.check_against_model(alone, want, "alone")

    def outputs():
        return ([TM._dev(np.full((n4 + n5, 3), TM.SENTINEL, np.int32))], TM._dev(np.full((1, 1), TM.SENTINEL, np.int32)),
                [TM._dev(np.full((n4 + n5, 4), TM.SENTINEL, np.float32))], [TM._dev(np.full((n, 4), TM.SENTINEL, np.int32)) for n in (n4, n5)])
    ms, cnt, ps, ks = outputs()
    d6 = [filler, filler, filler, filler[:P20 - 700], TM._dev(a), TM._dev(b)]
    k6 = [zk, zk, zk, zk[:P20 - 700], TM._dev(kps[0]), TM._dev(kps[1])]
    info6 = matcher.match_features_f32(d6, [(4, 5)], 0.3, ms, cnt, k6, [(8, 8)] * 4 + sizes, ps, ks)
    torch.cuda.synchronize()
    got = [dict(count=int(TM._np(cnt)[0, 0]), matches=TM._np(ms[0]), points=TM._np(ps[0]), knn=(TM._np(ks[0]), TM._np(ks[1])))]
    TM.check_against_model(got, want, "at the cap")
    for key in ("matches", "points"):
        assert np.array_equal(got[0][key], alone[0][key]), key
    assert all(np.array_equal(got[0]["knn"][d], alone[0]["knn"][d]) for d in range(2)) and info == info6 == (1, 3)
    assert bool((filler == 7.0).all())
    # one row more
    ms, cnt, ps, ks = outputs()
    d6[3], k6[3] = filler[:P20 - 699], zk[:P20 - 699]
    TM._expect(TM.ERR_UNSUPPORTED, lambda: matcher.match_features_f32(d6, [(4, 5)], 0.3, ms, cnt, k6, [(8, 8)] * 4 + sizes, ps, ks))
    torch.cuda.synchronize()
    assert all(bool((t == TM.SENTINEL).all()) for t in ms + [cnt] + ps + ks)
