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
