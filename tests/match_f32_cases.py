"""Cases of the float features matcher shared by tests/test_match_f32_model.py (CPU: the model) and the tests/test_gpu_match_f32*.py (the
library against the model)."""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_match_f32  # noqa: E402

F32 = np.float32
WIDTHS = fuzz_match_f32.WIDTHS


def bits(x):
    return int(np.array(x, F32).view(np.int32))


def line(values, cols):
    """Rows with only column 0 non-zero: d = |a - b| exactly for small integers."""
    out = np.zeros((len(values), cols), F32)
    out[:, 0] = values
    return out


def hand_case(cols=5):
    """The Hamming hand case's 14 matches on a line: two 40-row images with only column 0 non-zero, match_conf = 0.3.
    a[t] = 100 (t + 1), b[39 - t] = a[t] + t, t = 0 .. 9 (mutual; t = 0 identical); a fork: a[20] = 2000, b[5] = 2003, b[6] = 1997 (1->2
    rejected with d0 = d1 = 3, both 2->1 matches appended); a reverse fork: b[20] = 3000, a[30] = 3004, a[31] = 2996 (two 1->2 matches to one
    train row, 2->1 rejected).  The other rows sit in three heaps, those of a at 5000 / 6000 / 7000 and those of b 50 above: every one of
    them sees at least two rows of the other image at one distance, a tie, and is rejected."""
    a, b = np.zeros(40), np.zeros(40)
    used_a, used_b = set(), set()
    for t in range(10):
        a[t], b[39 - t] = 100 * (t + 1), 100 * (t + 1) + t
        used_a.add(t), used_b.add(39 - t)
    a[20], b[5], b[6] = 2000, 2003, 1997
    b[20], a[30], a[31] = 3000, 3004, 2996
    used_a |= {20, 30, 31}
    used_b |= {5, 6, 20}
    for n, r in enumerate(sorted(set(range(40)) - used_a)):
        a[r] = 5000 + 1000 * (n % 3)
    for n, r in enumerate(sorted(set(range(40)) - used_b)):
        b[r] = 5050 + 1000 * (n % 3)
    want = [(t, 39 - t, bits(t)) for t in range(10)] + [(30, 20, bits(4)), (31, 20, bits(4)), (20, 5, bits(3)), (20, 6, bits(3))]
    return line(a, cols), line(b, cols), np.array(want, np.int32)


ROUNDING_CONF = 0.65
ROUNDING = [(7 * j, 20 * j) for j in range(1, 13)]


def rounding_cases(cols=3):
    """The twelve (d0, d1) = (7j, 20j) at match_conf = 0.65, where float32 accepts (k = 0.35000002..., k * 20j rounds above 7j) and exact
    arithmetic rejects.  24 images, pair j = (2j - 2, 2j - 1): one query row at 0 against train rows at 7j and -20j on the line, in either
    order.  Each pair yields the single match (0, row of 7j, bits(7j)); 2->1 has one candidate only."""
    descs, pairs = [], []
    for j, (d0, d1) in enumerate(ROUNDING):
        descs += [line([0], cols), line([-d1, d0] if j % 2 else [d0, -d1], cols)]
        pairs.append((2 * j, 2 * j + 1))
    return descs, pairs


# ---- order sensitivity ---------------------------------------------------------------------------------------------------------------
def round_f32(x):
    """A Fraction rounded to float32, to nearest, ties to even."""
    f = F32(float(x))
    cands = {float(f), float(np.nextafter(f, F32(-np.inf))), float(np.nextafter(f, F32(np.inf)))}
    best = min(cands, key=lambda c: (abs(Fraction(c) - x), int(np.array(c, F32).view(np.uint32)) & 1))
    return F32(best)


def s_stated(q, t):
    s = F32(0)
    for c in range(len(q)):
        e = F32(q[c] - t[c])
        s = F32(s + F32(e * e))
    return s


def s_reversed(q, t):
    return s_stated(q[::-1], t[::-1])


def s_four_sums(q, t):
    """Four interleaved partial sums (columns c mod 4), added as (p0 + p1) + (p2 + p3): what a vectorised loop computes."""
    p = [s_stated(q[k::4], t[k::4]) for k in range(4)]
    return F32(F32(p[0] + p[1]) + F32(p[2] + p[3]))


def s_fma(q, t):
    """s = fma(e, e, s): the product is not rounded on its own."""
    s = F32(0)
    for c in range(len(q)):
        e = F32(q[c] - t[c])
        s = round_f32(Fraction(float(e)) * Fraction(float(e)) + Fraction(float(s)))
    return s


VARIANTS = (("reversed", s_reversed), ("four_sums", s_four_sums), ("fma", s_fma))


def order_case(cols=64, seed=20261121, tries=4000):
    """(q, x, y): a query row and two train rows, found by search with a fixed seed, such that in the stated order s(q, x) < s(q, y) - x is
    the nearest - while the reversed order, four interleaved partial sums and an FMA each give other bits for s(q, x) AND put y first.
    q holds small integers and x, y = q + r with r the same multiples of 2^-12 in two arrangements, so every e is exact and only the
    squares and the running sum round: the exact sums of x and y are equal, their float32 sums differ by the order alone."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-8, 9, cols).astype(F32)
    r = (rng.integers(1, 1 << 13, cols) / 4096.0).astype(F32)
    rows = np.stack([(q + rng.permutation(r) * rng.choice([-1.0, 1.0], cols)).astype(F32) for _ in range(tries)])
    # the search runs vectorised (the FMA in float64: 48-bit squares are exact there); the chosen rows are then confirmed exactly
    e = (q[None, :] - rows).astype(F32)
    sq = (e * e).astype(F32)

    def chain(cols_order, fused=False):
        s = np.zeros(tries, F32)
        for c in cols_order:
            s = (s.astype(np.float64) + e[:, c].astype(np.float64) ** 2).astype(F32) if fused else (s + sq[:, c]).astype(F32)
        return s
    st = chain(range(cols))
    parts = [chain(range(k, cols, 4)) for k in range(4)]
    var = [chain(range(cols - 1, -1, -1)), ((parts[0] + parts[1]).astype(F32) + (parts[2] + parts[3]).astype(F32)).astype(F32), chain(range(cols), True)]
    moved = (var[0] != st) & (var[1] != st) & (var[2] != st)
    for i in np.flatnonzero(moved):
        for j in np.flatnonzero(st > st[i]):
            if all(v[j] < v[i] for v in var):
                x, y = rows[i], rows[j]
                if all(fn(q, x) != s_stated(q, x) and fn(q, y) < fn(q, x) for _, fn in VARIANTS) and s_stated(q, x) < s_stated(q, y):
                    return q, x, y
    raise AssertionError("no order-sensitive rows among %d tries" % tries)


_ORDER = {}


def order_pair(cols=64):
    """The order case as a pair of images: one query, the train rows y, x (the nearest is row 1) and a far row."""
    if cols not in _ORDER:
        q, x, y = order_case(cols)
        far = (q + F32(100)).astype(F32)
        _ORDER[cols] = (np.stack([q, far]), np.stack([y, x, far]), (q, x, y))
    return _ORDER[cols]


# ---- special values ------------------------------------------------------------------------------------------------------------------
def special_cases():
    """name -> (descriptors, pairs, match_conf); cols = 3 throughout."""
    nan, inf = np.nan, np.inf
    z = [0, 0, 0]
    out = {}
    # equal s on different rows; duplicate train rows; s0 = s1 = 0 (row 2 of `a` equals rows 4 and 5 of `b`)
    a = np.array([[1, 2, 3], [10, 0, 0], [7, 7, 7], [50, 50, 50]], F32)
    b = np.array([[1, 2, 5], [1, 2, 1], [10, 3, 0], [10, 0, 3], [7, 7, 7], [7, 7, 7], [10, -3, 0], [50, 50, 51]], F32)
    out["ties"] = ([a, b], [(0, 1)], 0.3)
    # d0 = 0 < k d1
    out["zero_nearest"] = ([np.array([[4, 5, 6], [40, 50, 60]], F32), np.array([[4, 5, 6], [4, 5, 9], [40, 50, 60], [0, 0, 0]], F32)], [(0, 1)], 0.3)
    # squares of |e| = 1e-20 and 3e-20 are subnormal (1e-40, 9e-40): kept, the match is accepted; flushed to zero they would tie
    out["subnormal"] = ([np.array([z, [1, 1, 1]], F32), np.array([[1e-20, 0, 0], [0, 3e-20, 0], [1, 1, 1 + 1e-3], [1, 1, 5]], F32)], [(0, 1)], 0.3)
    # e * e overflows (2e19 squared), e itself overflows (3e38 - -3e38), s overflows in the sum
    big = np.array([[2e19, 0, 0], [3e38, 0, 0], [1.5e19, 1.5e19, 0], [1, 0, 0], [2, 0, 0]], F32)
    out["overflow"] = ([np.array([z, [-3e38, 0, 0], [2e19, 0, 1]], F32), big], [(0, 1)], 0.3)
    out["overflow_all"] = ([np.array([z, [1, 0, 0]], F32), big[:3]], [(0, 1)], 0.3)                  # every s = +inf: the order is the rows'
    # a NaN and an inf element in a query (rows 1, 2 of `a`) and in a train row: as second (b1), as nearest and both (b2, b3), among finite rows (b4)
    a = np.array([[1, 1, 1], [nan, 1, 1], [1, inf, 1], [2, 2, 2]], F32)
    b1 = np.array([[1, 1, 2], [nan, 0, 0]], F32)
    b2 = np.array([[0, nan, 0], [0, 0, -inf]], F32)
    b3 = np.array([[inf, 0, 0], [nan, nan, nan]], F32)
    b4 = np.array([[1, 1, 3], [inf, 1, 1], [2, 2, 2.5], [nan, 2, 2], [1, 1, 1]], F32)
    out["nonfinite"] = ([a, b1, b2, b3, b4], [(0, 1), (0, 2), (0, 3), (0, 4)], 0.3)
    return out


# ---- widths and shapes ---------------------------------------------------------------------------------------------------------------
def planted_pair(seed, n_from, n_to, cols, filler="isolated"):
    """(a, b, planted): fuzz_match_f32's structure (mutual matches, a fork, a reverse fork) and `filler` rows."""
    rng = np.random.default_rng(seed)
    descs, planted = fuzz_match_f32.build(rng, [n_from, n_to], [(0, 1)], cols, filler)
    return descs[0], descs[1], planted[0]


def shapes():
    """(n_from, n_to) on the tiling constants: query block +- 1, train tile +- 1, chunk +- 1 (257: a last chunk of one row)."""
    from imagestitch_amd.matcher import F32_TRAIN_TILE as T, QUERY_BLOCK as Q, TRAIN_CHUNK as CHUNK
    return [(Q - 1, T - 1), (Q, T), (Q + 1, T + 1), (2 * Q + 1, 2 * T + 1), (T + 3, CHUNK - 1), (Q - 3, CHUNK), (Q + 5, CHUNK + 1), (CHUNK + 1, 2 * CHUNK + 1)]


def degenerate_cases(cols=7):
    """name -> (descriptors, pairs, match_conf): n = 0, 1, 2, and an empty image among live ones."""
    e = np.zeros((0, cols), F32)
    one = line([10], cols)
    two = line([10.5, 40], cols)
    five = line([11, 13, 20, 30, 45], cols)
    a, b, _ = planted_pair(11, 24, 23, cols)
    return {
        "1x5": ([one, five], [(0, 1)], 0.3),
        "5x1": ([five, one], [(0, 1)], 0.3),
        "0x5": ([e, five], [(0, 1)], 0.3),
        "5x0": ([five, e], [(0, 1)], 0.3),
        "1x1": ([one, one], [(0, 1)], 0.3),
        "2x2": ([two, line([11, 38], cols)], [(0, 1)], 0.3),
        "1x2": ([one, two], [(0, 1)], 0.3),
        "empty_among_live": ([a, e, b, five], [(0, 1), (0, 2), (1, 2), (0, 3), (2, 3)], 0.3),
        "conf0": ([a, b], [(0, 1)], 0.0),
    }


def keypoints_for(seed, rows):
    """(keypoints, image sizes) for images of the given row counts."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(2, 4000)), int(rng.integers(2, 4000))) for _ in rows]
    return [(rng.random((n, 2)) * np.array(s)).astype(np.float32) for n, s in zip(rows, sizes)], sizes


def check_planted(rec, planted):
    """On one record of the model: every planted mutual match is a match, the fork's 1->2 is a tie and both its 2->1 matches are there, and
    the reverse fork likewise."""
    got = {(int(r[0]), int(r[1])) for r in rec["matches"]}
    for ra, rb, _ in planted["mutual"]:
        assert (ra, rb) in got, (ra, rb)
    ra, rb1, rb2 = planted["fork"]
    assert rec["knn"][0][ra, 1] == rec["knn"][0][ra, 3] and {(ra, rb1), (ra, rb2)} <= got
    rb, ra1, ra2 = planted["reverse_fork"]
    assert rec["knn"][1][rb, 1] == rec["knn"][1][rb, 3] and {(ra1, rb), (ra2, rb)} <= got
    assert min(rec["kinds"]) >= 1, rec["kinds"]
