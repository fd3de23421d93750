"""Cases of the features matcher shared by tests/test_match_model.py (CPU: the model) and tests/test_gpu_match.py (the library against the
model).  A flip is an XOR of the named bit positions of a 256-bit row."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_match  # noqa: E402
from fuzz_match import flip, random_rows  # noqa: E402,F401


def hand_case():
    """Two 40-row images; match_conf = 0.3 gives 14 matches: 12 from 1->2 and then (20, 5, 3), (20, 6, 3).
    b[39 - t] = a[t] with bits 0 .. t-1 flipped, t = 0 .. 9 (mutual; t = 0 identical); a fork: b[5], b[6] = a[20] with bits {0, 1, 2} /
    {3, 4, 5} flipped (1->2 rejected with d0 = d1 = 3, both 2->1 matches appended); a reverse fork: a[30], a[31] = b[20] with bits {0 .. 3} /
    {4 .. 7} flipped (two 1->2 matches to one train row, 2->1 rejected).  The other rows are random."""
    rng = np.random.default_rng(20261119)
    a, b = random_rows(rng, 40), random_rows(rng, 40)
    for t in range(10):
        b[39 - t] = flip(a[t], range(t))
    b[5], b[6] = flip(a[20], (0, 1, 2)), flip(a[20], (3, 4, 5))
    a[30], a[31] = flip(b[20], (0, 1, 2, 3)), flip(b[20], (4, 5, 6, 7))
    want = [(t, 39 - t, t) for t in range(10)] + [(30, 20, 4), (31, 20, 4), (20, 5, 3), (20, 6, 3)]
    return a, b, np.array(want, np.int32)


ROUNDING_CONF = 0.65
ROUNDING = [(7 * j, 20 * j) for j in range(1, 13)]


def rounding_cases():
    """The twelve (d0, d1) = (7j, 20j) at match_conf = 0.65, where float32 accepts (k = 0.35000002..., k * 20j rounds above 7j) and exact
    arithmetic rejects.  24 images, pair j = (2j - 2, 2j - 1): one query row against the two train rows 7j and 20j flips away, so the two
    neighbours are exactly those whatever else is there.  Each pair yields the single match (0, 0, 7j); 2->1 has one candidate only.
    (All twelve cannot live in ONE image pair, so they run in one call instead.  For j = 12 every train row but the nearest is at least
    240 bits from the query, that is within 16 bits of its complement: all rows of the other image but one lie in a ball of radius 16, and
    so, by j = 11 in either direction, do those of the query's own image within 52.  A query of a small j then has its nearest row within
    32 + 7j bits of every other query beside it, nearer than the 20j' their second neighbours must keep; sharing one nearest row among
    queries j < j' needs 7j' >= 13.5 (j' - j) bits, which fails from j' = 12 down to j = 5.)"""
    rng = np.random.default_rng(65)
    descs, pairs = [], []
    for j, (d0, d1) in enumerate(ROUNDING):
        q = random_rows(rng, 1)
        bits = rng.permutation(256)
        t = np.stack([flip(q[0], bits[:d1]), flip(q[0], bits[256 - d0:])]) if j % 2 else np.stack([flip(q[0], bits[256 - d0:]), flip(q[0], bits[:d1])])
        descs += [q, t]
        pairs.append((2 * j, 2 * j + 1))
    return descs, pairs


def planted_pair(seed, n_from, n_to, filler="random"):
    """(a, b, planted): mutual matches at distances 0 .. 16 on a random permutation of the rows, a fork, a reverse fork, `filler` rows."""
    rng = np.random.default_rng(seed)
    descs, planted = fuzz_match.build(rng, [n_from, n_to], [(0, 1)], filler)
    return descs[0], descs[1], planted[0]


MAX_SPLIT = 32             # chunks per (pair, direction) at most: MT_MAX_SPLIT of csrc/match.hip


def chunk_plan(nt):
    """(chunk_rows, nchunks) of a direction whose train image has nt rows: TRAIN_CHUNK rows a work item until that would make more than
    MAX_SPLIT chunks, whole multiples of TRAIN_CHUNK from there (the host's rule in isx_match_features, restated)."""
    from imagestitch_amd.matcher import TRAIN_CHUNK
    crows = TRAIN_CHUNK * -(-nt // (TRAIN_CHUNK * MAX_SPLIT))
    return crows, -(-nt // crows)


def planted_at(seed, n_from, n_to, mutual_rows, big_first=None):
    """(a, b, planted) like planted_pair, with the structure at rows of the caller's choosing in the larger image (the `big` one: b, or a
    where n_from > n_to or big_first): mutual_rows are its rows of the mutual matches, at distances 0, 1, .. in that order, against rows of
    the small image drawn from a permutation.  planted = dict(big_is_from, mutual=[(small row, big row, distance)], then whatever the caller
    adds with plant_near()).  Everything else is random filler."""
    rng = np.random.default_rng(seed)
    big_is_from = n_from > n_to if big_first is None else bool(big_first)
    a, b = random_rows(rng, n_from), random_rows(rng, n_to)
    big, small = (a, b) if big_is_from else (b, a)
    free = list(rng.permutation(small.shape[0]))
    planted = dict(big_is_from=big_is_from, mutual=[], near=[], free=free, rng=rng)
    assert len(set(mutual_rows)) == len(mutual_rows)
    for t, r in enumerate(mutual_rows):
        s = int(free.pop())
        big[r] = flip(small[s], rng.permutation(256)[:t])
        planted["mutual"].append((s, int(r), t))
    return a, b, planted


def plant_near(a, b, planted, row0, d0, row1, d1):
    """One more query of the small image whose nearest rows of the big one are row0 at d0 flips and row1 at d1 (disjoint bits, so the two
    are d0 + d1 apart); d0 == d1 is a tie, which knn orders by row.  Returns the query's row; planted["near"] gets (query, row0, d0, row1, d1)."""
    big, small = (a, b) if planted["big_is_from"] else (b, a)
    q = int(planted["free"].pop())
    bits = planted["rng"].permutation(256)
    if d0 == d1:                                           # a tie: identical rows
        big[row0] = big[row1] = flip(small[q], bits[:d0])
    else:
        big[row0], big[row1] = flip(small[q], bits[:d0]), flip(small[q], bits[d0:d0 + d1])
    planted["near"].append((q, int(row0), d0, int(row1), d1))
    return q


def split_pair(seed, n_from, n_to):
    """A pair whose larger image has more than one chunk, for tests/test_gpu_match_split.py.  With (crows, nch) = chunk_plan(rows of the
    big image) and `last` the first row of its last chunk, planted in the big image:
      mutual matches at rows 0, crows - 1, crows, nch // 2 * crows, last, nt - 1 (one row where last == nt - 1), distances 0, 1, ..
      tie        two identical rows, 2 flips from one query: one in chunk 0 (row 5), one in the last chunk; the query is rejected
      apart      nearest (3 flips) in chunk 1, second nearest (40 flips) in the last chunk but one
      together   nearest (4 flips) and second nearest (50 flips) both in the last chunk
      reverse    two rows of the small image 4 flips (disjoint) from one row of the big one, at the end of chunk 1: accepted from the small
                 side only - with the tie, which is accepted from the big side only, every kind of match is there
    A last chunk of fewer than 5 rows (8 193 rows: one) cannot hold all of that: the mutual matches keep it, and the far rows of `tie` and
    `together` move to the end of the chunk before.  planted["rows"] names where each landed."""
    big_n = max(n_from, n_to)
    crows, nch = chunk_plan(big_n)
    last = (nch - 1) * crows
    mutual = [0, crows - 1, crows, nch // 2 * crows, last] + ([big_n - 1] if big_n - 1 != last else [])
    a, b, planted = planted_at(seed, n_from, n_to, mutual)
    roomy = big_n - last >= 5
    tie_far, tog0, tog1 = (last + 1, last + 2, big_n - 2) if roomy else (last - 1, last - 3, last - 2)
    rows = dict(crows=crows, nch=nch, last=last, roomy=roomy, tie=(5, tie_far), apart=(crows + 7, last - crows + 9), together=(tog0, tog1),
                reverse=2 * crows - 1)
    plant_near(a, b, planted, 5, 2, tie_far, 2)
    plant_near(a, b, planted, rows["apart"][0], 3, rows["apart"][1], 40)
    plant_near(a, b, planted, tog0, 4, tog1, 50)
    big, small = (a, b) if planted["big_is_from"] else (b, a)
    s1, s2 = int(planted["free"].pop()), int(planted["free"].pop())
    bits = planted["rng"].permutation(256)[:8]
    small[s1], small[s2] = flip(big[rows["reverse"]], bits[:4]), flip(big[rows["reverse"]], bits[4:])
    rows["reverse_small"] = (s1, s2)
    planted["rows"] = rows
    used = mutual + [5, tie_far, tog0, tog1, rows["reverse"]] + list(rows["apart"])
    assert len(set(used)) == len(used), used
    return a, b, planted


def check_planted_at(rec, planted, conf=0.3):
    """On one record of match_model: every mutual match of planted_at is a match, every plant_near query has exactly its two neighbours
    in knn, the lower row first on a tie, and is accepted or rejected as the ratio test says."""
    from helpers import match_np as M
    swap = planted["big_is_from"]
    got = {tuple(int(v) for v in r) for r in rec["matches"]}
    knn = rec["knn"][1 if swap else 0]                     # the direction whose train rows are the big image's
    for s, r, t in planted["mutual"]:
        assert ((r, s, t) if swap else (s, r, t)) in got, (s, r, t)
        assert tuple(knn[s][:2]) == (r, t), (s, r, t, knn[s])
    ok = M.accepted(knn, conf)
    for q, r0, d0, r1, d1 in planted["near"]:
        assert tuple(knn[q]) == (min(r0, r1), d0, max(r0, r1), d1) if d0 == d1 else tuple(knn[q]) == (r0, d0, r1, d1), (q, knn[q])
        assert bool(ok[q]) == (d0 != d1), (q, knn[q])      # (a tie's rows still accept the query from their side)
        assert d0 == d1 or ((r0, q, d0) if swap else (q, r0, d0)) in got, (q, knn[q])


def check_split_planted(rec, planted):
    """check_planted_at, and that the rows of split_pair lie in the chunks its docstring names."""
    check_planted_at(rec, planted)
    assert min(rec["kinds"]) >= 1, rec["kinds"]
    rows = planted["rows"]
    crows, nch, last = rows["crows"], rows["nch"], rows["last"]
    chunk = lambda r: r // crows                            # noqa: E731
    assert crows > 256 or nch == MAX_SPLIT
    assert [chunk(r) for _, r, _ in planted["mutual"]][:5] == [0, 0, 1, nch // 2, nch - 1] and planted["mutual"][-1][1] == max(len(k) for k in rec["knn"]) - 1
    far = nch - 1 if rows["roomy"] else nch - 2
    assert (chunk(rows["tie"][0]), chunk(rows["tie"][1])) == (0, far) and far > 0
    assert chunk(rows["apart"][0]) == 1 and chunk(rows["apart"][1]) == nch - 2 and nch - 2 > 1
    assert chunk(rows["together"][0]) == chunk(rows["together"][1]) == far
    s1, s2 = rows["reverse_small"]
    swap = planted["big_is_from"]
    got = {tuple(int(v) for v in r) for r in rec["matches"]}
    assert {(rows["reverse"], s, 4) if swap else (s, rows["reverse"], 4) for s in (s1, s2)} <= got
    small_side = rec["knn"][0 if swap else 1]              # the big image's rows as queries
    assert tuple(small_side[rows["reverse"]]) == (min(s1, s2), 4, max(s1, s2), 4)
    for r in rows["tie"]:                                  # the tie, seen from the big side: both rows accept the query
        assert ((r, planted["near"][0][0], 2) if swap else (planted["near"][0][0], r, 2)) in got


def keypoints_for(seed, rows):
    """(keypoints, image sizes) for images of the given row counts."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(2, 4000)), int(rng.integers(2, 4000))) for _ in rows]
    return [(rng.random((n, 2)) * np.array(s)).astype(np.float32) for n, s in zip(rows, sizes)], sizes


def degenerate_cases():
    """name -> (descriptors, pairs, match_conf)."""
    rng = np.random.default_rng(7)
    one = random_rows(rng, 1)
    five = np.stack([flip(one[0], range(k)) for k in (2, 9, 30, 60, 100)])      # 2, 9, .. bits from `one`
    two = random_rows(rng, 2)
    same = np.repeat(random_rows(rng, 1), 6, axis=0)
    a, b, _ = planted_pair(11, 24, 23)
    return {
        "1x5": ([one, five], [(0, 1)], 0.3),              # n_to = 5: 1->2 runs; 2->1 has one candidate: nothing
        "5x1": ([five, one], [(0, 1)], 0.3),              # n_to = 1: no 1->2 match; 2->1 still runs against 5 candidates
        "0x5": ([np.zeros((0, 32), np.uint8), five], [(0, 1)], 0.3),
        "5x0": ([five, np.zeros((0, 32), np.uint8)], [(0, 1)], 0.3),
        "2x2": ([two, np.stack([flip(two[0], (3,)), flip(two[1], (5, 6))])], [(0, 1)], 0.3),
        "identical": ([same, same[:4]], [(0, 1)], 0.3),   # every distance 0: 0 < k * 0 is false
        "conf0": ([a, b], [(0, 1)], 0.0),
    }
