"""Randomised parity of the float features matcher (isx_match_features_f32) against its NumPy model (tests/helpers/match_f32_np.py): matches,
counts, points and knn with np.array_equal.

    python tools/fuzz_match_f32.py --seconds 120 --seed 20261121 [--out profiles/fuzz_match_f32_120s.json]

The generator (no GPU needed: tests/test_match_f32_model.py checks it).  case(seed, cls) draws one of CLASSES:
    tiny          4 .. 12 rows an image
    widths        cols on both sides of the padding to 64 / 128: 1, 3, 4, 63, 64, 65, 127, 128
    tile_edges    rows at a multiple of QUERY_BLOCK / F32_TRAIN_TILE, one less, one more
    chunk_edges   rows at a multiple of TRAIN_CHUNK, one less, one more
    duplicates    cloud filler with rows repeated (ties of the first and of the second neighbour)
    clustered     filler rows a few steps of 1/64 from one base row (small distances, exact ties, ratio tests either side of the bound)
    specials      cloud filler with NaN, +-inf, 1e-20 and 3e19 sprinkled in (s becomes +inf, subnormal squares, overflow)
    many          3 .. 5 images, a mask, an image without rows now and then
    split         one image of 8192 k - 1, 8192 k or 8192 k + 1 rows, k = 1 .. 2, against one of 4 .. 300, in either order
cols is one of WIDTHS or 2 .. 128 (one value a case).  Rows live in clusters along column 0 (centre 64 g, the other columns in [-1, 1]), so
what is planted for a pair stays isolated at every width: mutual matches (a row and a copy moved by t / 64 in some columns, t = 0 .. 16 -
accepted both ways), a fork (two rows of `to` one unit either side of a row of `from` whose values are multiples of 2^-10: an exact tie, 1->2
is rejected and both 2->1 matches are appended) and a reverse fork.  Filler: `isolated` (a cluster a row: filler k of one image lies beside
filler k of the other, which gives accepted matches of rounding-sensitive distances), `cloud` (one cluster for all: ratios near 1).
match_conf is drawn from {0, 0.3, 0.5, 0.65} and [0, 0.9]: what is planted passes the ratio test against a second neighbour 62 away
throughout.  Layouts: host or device mats, dense or with padded rows (a step that is a multiple of 4), outputs dense or padded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from fuzz_match import SENTINEL, _place  # noqa: E402
from helpers import match_f32_np as MF  # noqa: E402
from imagestitch_amd.matcher import F32_TRAIN_TILE, QUERY_BLOCK, TRAIN_CHUNK  # noqa: E402

CLASSES = ("tiny", "widths", "tile_edges", "chunk_edges", "duplicates", "clustered", "specials", "many", "split")
WIDTHS = (1, 3, 4, 63, 64, 65, 127, 128)
SPLIT_ROWS = TRAIN_CHUNK * 32
CONFS = (0.0, 0.3, 0.5, 0.65)
ROWS_PER_PAIR = 4
MAX_MUTUAL = 17
SPACING = 64.0             # between cluster centres along column 0
F32 = np.float32


def cluster_row(rng, g, cols, grid=False):
    """A row of cluster g: column 0 at 64 g + u, the others u, u in [-1, 1]; grid: multiples of 2^-10 (a unit step is then exact)."""
    u = rng.random(cols) * 2.0 - 1.0
    if grid:
        u = np.round(u * 1024.0) / 1024.0
    u[0] += SPACING * g
    return u.astype(F32)


def plant(rng, descs, free, i, j, left, groups):
    """Plants one pair's structure into rows of images i and j taken from their free lists; `groups` counts the clusters handed out."""
    fi, fj = free[i], free[j]
    m = int(min(MAX_MUTUAL, len(fi) // left[i] - 3, len(fj) // left[j] - 3))
    left[i] -= 1
    left[j] -= 1
    assert m >= 1, "an image needs %d free rows a pair" % ROWS_PER_PAIR
    a, b = descs[i], descs[j]
    cols = a.shape[1]
    planted = dict(mutual=[], fork=None, reverse_fork=None)
    for t in range(m):
        ra, rb = fi.pop(), fj.pop()
        a[ra] = cluster_row(rng, groups[0], cols)
        move = np.zeros(cols, F32)
        move[rng.permutation(cols)[:max(1, cols // 2)]] = F32(t / 64.0)
        b[rb] = a[ra] + move
        groups[0] += 1
        planted["mutual"].append((ra, rb, t))
    unit = np.zeros(cols, F32)
    unit[int(rng.integers(1, cols)) if cols > 1 else 0] = 1.0      # (beside column 0 where there is one: its values are the large ones)
    ra, rb1, rb2 = fi.pop(), fj.pop(), fj.pop()
    a[ra] = cluster_row(rng, groups[0], cols, True)
    b[rb1], b[rb2] = a[ra] + unit, a[ra] - unit
    planted["fork"] = (ra, rb1, rb2)
    rb, ra1, ra2 = fj.pop(), fi.pop(), fi.pop()
    b[rb] = cluster_row(rng, groups[0] + 1, cols, True)
    a[ra1], a[ra2] = b[rb] + unit, b[rb] - unit
    planted["reverse_fork"] = (rb, ra1, ra2)
    groups[0] += 2
    return planted


SPECIALS = (np.nan, np.inf, -np.inf, 1e-20, -1e-20, 3e19, -3e19, 0.0)


def build(rng, rows, pairs, cols, filler="isolated"):
    """Descriptor arrays (n x cols float32) of the given row counts with every pair's planted structure and `filler` rows elsewhere."""
    descs = [np.zeros((n, cols), F32) for n in rows]
    free = [list(rng.permutation(n)) for n in rows]
    left = [sum(1 for p in pairs if k in p) for k in range(len(rows))]
    groups = [1]
    planted = [plant(rng, descs, free, i, j, left, groups) for i, j in pairs]
    first = groups[0] + 1
    for d, f in zip(descs, free):
        f = [int(r) for r in f]
        if not f:
            continue
        if filler == "isolated":
            u = (rng.random((len(f), cols)) * 2.0 - 1.0)
            u[:, 0] += SPACING * (first + np.arange(len(f)))
            d[f] = u.astype(F32)
        elif filler == "clustered":
            base = cluster_row(rng, -3, cols, True)
            d[f] = base[None, :] + (rng.integers(-2, 3, (len(f), cols)) * (rng.random((len(f), cols)) < 4.0 / cols) / 64.0).astype(F32)
        else:                                                  # cloud, duplicates, specials: one cluster for all
            u = (rng.random((len(f), cols)) * 2.0 - 1.0)
            u[:, 0] -= SPACING * 3
            d[f] = u.astype(F32)
            fa = np.asarray(f)
            if filler == "duplicates" and len(f) >= 2:
                for _ in range(max(1, len(f) // 3)):
                    src, dst = rng.choice(fa, 2, replace=False)
                    d[dst] = d[src]
            if filler == "specials":
                for _ in range(max(1, len(f) // 2)):
                    d[int(rng.choice(fa)), int(rng.integers(cols))] = F32(SPECIALS[int(rng.integers(len(SPECIALS)))])
    return descs, planted


def _edge(rng, unit, most=3):
    return max(ROWS_PER_PAIR, int(unit * rng.integers(1, most + 1) + rng.integers(-1, 2)))


def case(seed, cls=None):
    """One case: dict(cls, cols, descriptors, keypoints, img_sizes, pairs, mask, match_conf, planted, layout_seed)."""
    rng = np.random.default_rng(seed)
    cls = cls or CLASSES[int(rng.integers(len(CLASSES) - 1))]          # (split only when asked for: it is the slow one)
    mask = None
    filler = cls if cls in ("duplicates", "clustered", "specials") else ("isolated", "cloud")[int(rng.integers(2))]
    cols = int(WIDTHS[int(rng.integers(len(WIDTHS)))]) if cls == "widths" or rng.random() < 0.5 else int(rng.integers(2, 129))
    if cls in ("tiny", "widths"):
        rows = [int(rng.integers(4, 13)) for _ in range(2)]
    elif cls == "tile_edges":
        rows = [_edge(rng, QUERY_BLOCK), _edge(rng, F32_TRAIN_TILE, 5)]
    elif cls == "chunk_edges":
        rows = [_edge(rng, TRAIN_CHUNK, 2), _edge(rng, TRAIN_CHUNK, 2)]
    elif cls in ("duplicates", "clustered", "specials"):
        rows = [int(rng.integers(8, 300)) for _ in range(2)]
    elif cls == "split":
        rows = [SPLIT_ROWS * int(rng.integers(1, 3)) + int(rng.integers(-1, 2)), int(rng.integers(4, 301))]
        if rng.random() < 0.5:
            rows.reverse()
        cols = min(cols, 64) if rng.random() < 0.7 else cols
    else:
        n = int(rng.integers(3, 6))
        rows = [int(rng.integers(ROWS_PER_PAIR * (n - 1), 200)) for _ in range(n)]
        if rng.random() < 0.4:
            rows[int(rng.integers(n))] = 0
        mask = (rng.random((n, n)) < 0.75).astype(np.uint8)
        if not any(mask[i, j] for i, j in MF.near_pairs(rows)):
            mask = None
    pairs = MF.near_pairs(rows, mask)
    descs, planted = build(rng, rows, pairs, cols, filler)
    sizes = [(int(rng.integers(1, 5000)), int(rng.integers(1, 5000))) for _ in rows]
    kps = [(rng.random((n, 2)) * np.array(s)).astype(np.float32) for n, s in zip(rows, sizes)]
    conf = float(CONFS[int(rng.integers(len(CONFS)))]) if rng.random() < 0.7 else float(np.float32(rng.random() * 0.9))
    return dict(cls=cls, cols=cols, descriptors=descs, keypoints=kps, img_sizes=sizes, pairs=pairs, mask=mask, match_conf=conf, planted=planted,
                layout_seed=int(rng.integers(1 << 30)))


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
def run_case(c, rng=None):
    """Runs one case through the library in a random layout and compares with the model.  Returns a list of differences (empty: equal)."""
    import torch
    from imagestitch_amd import matcher
    rng = rng or np.random.default_rng(c["layout_seed"])
    pairs, descs = c["pairs"], c["descriptors"]
    if not pairs:
        return []
    want = MF.match_model(descs, pairs, c["match_conf"], c["keypoints"], c["img_sizes"])
    with_points, with_knn = bool(rng.random() < 0.7), bool(rng.random() < 0.7)

    def layout():
        return bool(rng.random() < 0.5), bool(rng.random() < 0.5)
    d_in = [_place(rng, d, *layout())[0] for d in descs]
    k_in = [_place(rng, k, *layout())[0] for k in c["keypoints"]] if with_points else None
    cap = [descs[i].shape[0] + descs[j].shape[0] + int(rng.integers(0, 3)) for i, j in pairs]
    ms = [_place(rng, np.full((n, 3), SENTINEL, np.int32), *layout()) for n in cap]
    ps = [_place(rng, np.full((n, 4), SENTINEL, np.float32), *layout()) for n in cap] if with_points else None
    ks = [_place(rng, np.full((descs[p[d]].shape[0], 4), SENTINEL, np.int32), *layout()) for p in pairs for d in range(2)] if with_knn else None
    cnt = _place(rng, np.full((1, len(pairs)), SENTINEL, np.int32), bool(rng.random() < 0.5), False)
    stream = torch.cuda.current_stream()
    matcher.match_features_f32(d_in, pairs, c["match_conf"], [m[0] for m in ms], cnt[0], k_in, c["img_sizes"] if with_points else None,
                               [p[0] for p in ps] if ps else None, [k[0] for k in ks] if ks else None, 0, stream)
    stream.synchronize()
    bad = []
    counts = cnt[1]()[0]
    for k, w in enumerate(want):
        if counts[k] != w["count"]:
            bad.append("pair %d: count %d, the model %d" % (k, counts[k], w["count"]))
            continue
        got = ms[k][1]()
        if not np.array_equal(got[:w["count"]], w["matches"]) or not (got[w["count"]:] == SENTINEL).all():
            bad.append("pair %d: matches differ (or rows past the count were written)" % k)
        if ps:
            got = ps[k][1]()
            if not np.array_equal(got[:w["count"]], w["points"]) or not (got[w["count"]:] == SENTINEL).all():
                bad.append("pair %d: points differ" % k)
        if ks:
            for d in range(2):
                if not np.array_equal(ks[2 * k + d][1](), w["knn"][d]):
                    bad.append("pair %d: knn of direction %d differs" % (k, d))
    return bad


def scheduled(seed, n, with_split=True):
    """(case seed, class) of a soak's n-th case: the classes in turn."""
    classes = CLASSES if with_split else CLASSES[:-1]
    return int(seed) * 1000003 + n, classes[n % len(classes)]


def run(seconds, seed, verbose=False, progress_path=None, with_split=True):
    """Draws cases (the classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    per, failing, n, pairs, told = {c: 0 for c in CLASSES}, [], 0, 0, t0
    while time.time() - t0 < seconds:
        if progress_path and time.time() - told >= 30.0:
            told = time.time()
            with open(progress_path, "w") as f:
                json.dump(dict(seconds=round(told - t0, 1), cases=n, mismatches=len(failing)), f)
        s, cls = scheduled(seed, n, with_split)
        c = case(s, cls)
        bad = run_case(c)
        per[cls] += 1
        pairs += len(c["pairs"])
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=cls, cols=c["cols"], differences=bad[:4]))
            if verbose:
                print("MISMATCH", s, cls, c["cols"], bad[:4], flush=True)
    return dict(tool="fuzz_match_f32", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, pairs=pairs, mismatches=len(failing), per_class=per,
                failing_seeds=failing[:20], device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261121)
    ap.add_argument("--out", default=None)
    ap.add_argument("--progress", default=None)
    a = ap.parse_args()
    out = run(a.seconds, a.seed, verbose=True, progress_path=a.progress)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(1 if out["mismatches"] else 0)


if __name__ == "__main__":
    main()
